#!/usr/bin/env python3
"""The weight-streaming Linear on MXFP4 codes against what it replaces, on the MI355X.  Per layer matrix of the
Llama-3-8B shape ([6144, 4096] qkv, [4096, 4096] o, [28672, 4096] gate/up, [4096, 14336] down) and M in {1, 4, 16, 32, 128}:
  (i)   lrp_linear_stream_fwd_q on the codes and scales;
  (ii)  the control it replaces: lrp_mxfp4_dequant into a bf16 matrix + lrp_linear_stream_fwd_tk on it;
  (iii) the bf16 stream kernel alone on the dequantised matrix.
Microseconds per call are medians (and minima) of --reps device-event times of a hipGraph of --calls launches, divided by --calls; the three
variants' graphs are alternated replay by replay inside one process, and every launch takes the NEXT of --copies copies of the weight
(together far beyond the 256 MiB Infinity Cache; a replay of another variant runs in between), so the weight comes from HBM.
TB/s = the bytes the variant must read (codes + scales for (i), the bf16 matrix for (iii), codes + scales in, bf16 out and in for (ii)) over
its time; the floor of (i) is its bytes at 6.3 TB/s.  The outputs of (i) and (ii) are compared bit for bit on every cell.
usage: python tools/mxfp4_stream_bench.py [--out FILE] [--reps 30] [--copies N] [--calls 32]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

HBM = 6.3e12
SHAPES = (("qkv", 6144, 4096), ("o", 4096, 4096), ("gate/up", 28672, 4096), ("down", 4096, 14336))
ROWS = (1, 4, 16, 32, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--copies", type=int, default=0, help="copies of each weight to rotate through (0: enough for 1.5 GB of codes)")
    ap.add_argument("--calls", type=int, default=32, help="launches per timed graph replay")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_stream_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"us per call = median (min) over {a.reps} replays of a hipGraph of up to {a.calls} launches, variants alternated replay by replay, weights rotated through "
        "copies; "
        "(i) lrp_linear_stream_fwd_q, (ii) lrp_mxfp4_dequant + lrp_linear_stream_fwd_tk, (iii) lrp_linear_stream_fwd_tk on the bf16 matrix")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, N, K in SHAPES:
        qbytes, wbytes = N * K * 4.25 / 8, N * K * 2.0
        copies = a.copies or max(4, int(1.5e9 // qbytes))
        ncall = min(a.calls, copies)
        W = [(torch.randn(N, K, generator=g, device="cuda") * 0.02).bfloat16() for _ in range(copies)]
        Q = [ops.mxfp4_quantize(w) for w in W]
        for w, (c, s) in zip(W, Q):
            ops.mxfp4_dequant(c, s, w)                     # (iii) runs on the matrix the codes hold
        scratch = torch.empty(N, K, device="cuda", dtype=torch.bfloat16)
        for M in ROWS:
            x = torch.randn(M, K, generator=g, device="cuda").bfloat16()
            served = ops.linear_stream_q_ok(x, *Q[0])
            o1, o2, o3 = (torch.empty(M, N, device="cuda", dtype=torch.bfloat16) for _ in range(3))
            it = [0]

            def v1():
                ops.linear_stream_fwd_q(x, *Q[it[0] % copies], out=o1)

            def v2():
                c, s = Q[it[0] % copies]
                ops.mxfp4_dequant(c, s, scratch)
                ops.linear_stream_fwd(x, scratch, out=o2)

            def v3():
                ops.linear_stream_fwd(x, W[it[0] % copies], out=o3)

            # one hipGraph per variant: --calls launches, each on the next copy of the weight (a single launch between two events times the
            # host's enqueue, not the kernel); a replay's time / --calls is the time of one call, kernel boundary included
            graphs = []
            for fn in (v1, v2, v3):
                it[0] = 0
                fn()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(ncall):
                        fn()
                        it[0] += 1
                graphs.append(gr)
            ts = ([], [], [])
            for r in range(a.reps + 3):
                for k, gr in enumerate(graphs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gr.replay()
                    e1.record()
                    e1.synchronize()
                    if r >= 3:
                        ts[k].append(e0.elapsed_time(e1) * 1e3 / ncall)
            same = torch.equal(o1, o2)
            del graphs
            (m1, b1), (m2, b2), (m3, b3) = ((statistics.median(t), min(t)) for t in ts)
            floor = qbytes / HBM * 1e6
            say(f"  {name:7s} [{N:5d}, {K:5d}] M {M:3d}: (i) {m1:7.1f} us ({b1:7.1f}) {qbytes / m1 / 1e6:5.2f} TB/s   (ii) {m2:7.1f} us ({b2:7.1f}) "
                f"{(qbytes + 2 * wbytes) / m2 / 1e6:5.2f} TB/s   (iii) {m3:7.1f} us ({b3:7.1f}) {wbytes / m3 / 1e6:5.2f} TB/s   "
                f"(i)/(ii) {m1 / m2:5.3f}  (i)/(iii) {m1 / m3:5.3f}  floor of (i) {floor:5.1f} us = {floor / m1:5.3f} of it   "
                f"q_ok {int(served)}  (i) == (ii) bitwise: {same}")
        del W, Q, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
