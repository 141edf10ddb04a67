#!/usr/bin/env python3
"""lrp_moe_wgrad_rel on the MI355X: the per-weight relevance of the routed experts at the Qwen3-30B-A3B layer
(128 experts, top-8, H 2048, moe_intermediate_size 768; gate_up [128, 1536, 2048], down [128, 2048, 768]), T = 2048 and 8192 tokens,
uniform random routing, bf16.  Per mode, weight format (plain / MXFP4) and accumulate off / on, from device events (median over --reps timed
calls after warm-up):
  * the kernel, one launch;
  * the composition a user would write: a per-expert loop out[e] (+)= ((G_e s).T @ X_e).float() * W[e] on rows gathered through the plan
    (the expert row lists are taken to the host once, outside the timing);
  * the time the mandatory bytes take at 6.3 TB/s (the achievable HBM rate): 4 E N K written, the same read when accumulating, plus W
    as held (2 bytes per element, 17 / 32 as MXFP4); the operands G and X (at most 0.3 GB at T = 8192) are not counted;
  * the epilogue's store shape alone: the kernel on a plan without live rows (it then only writes zeros at the accumulator's addresses)
    against a plain fill of the same tensor.
usage: python tools/moe_wgrad_bench.py [--out FILE] [--reps 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

H, I, E, K_SLOTS = 2048, 768, 128, 8
HBM = 6.3e12


def timed(fn, reps):
    """median milliseconds of fn() over reps calls, each between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_wgrad_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}; {E} experts, top-{K_SLOTS}, H {H}, I {I}, bf16, uniform random routing"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(0)
    say("out [E, N, K] fp32 (+)= W (*) sum_p s G^T X per expert; ms = median (min) of device-event times; bytes = 4 E N K written (+ read "
        "when accumulating) + W as held; floor = bytes / 6.3 TB/s")
    for T in (2048, 8192):
        R = T * K_SLOTS
        idx = torch.rand(T, E, device="cuda", generator=g).argsort(1)[:, :K_SLOTS].contiguous()
        w = (torch.rand(T, K_SLOTS, device="cuda", generator=g) / K_SLOTS).bfloat16()
        plan = ops.MoePlan(idx, E)
        cnt, off, perm, _ = (v.tolist() for v in plan.views())
        say(f"T {T}: rows per expert min {min(cnt)} mean {R / E:.0f} max {max(cnt)}")
        for mode, N, K in (("gate_up", 2 * I, H), ("down", H, I)):
            gr, xr = (R, T) if mode == "gate_up" else (T, R)
            G = torch.randn(gr, N, generator=g, device="cuda").bfloat16()
            X = torch.randn(xr, K, generator=g, device="cuda").bfloat16()
            W = (torch.randn(E, N, K, generator=g, device="cuda") * K ** -0.5).bfloat16()
            Wq = ops.MoeQuantWeight(W)
            out = torch.zeros(E, N, K, device="cuda")
            src = [torch.tensor(perm[off[e]:off[e + 1]], device="cuda", dtype=torch.long) for e in range(E)]
            tok = [s // K_SLOTS for s in src]
            half_w = 0.5 * w.flatten()

            def composition(acc):
                for e in range(E):
                    rows = slice(off[e], off[e + 1])
                    if mode == "gate_up":
                        Ge, Xe = G[rows], X[tok[e]]
                    else:
                        Ge, Xe = G[tok[e]] * half_w[src[e]][:, None], X[rows]
                    r = torch.matmul(Ge.T, Xe).float() * W[e]
                    if acc:
                        out[e] += r
                    else:
                        out[e] = r

            for acc in (False, True):
                row = [f"T {T:5d} {mode:8s} N {N:5d} K {K:5d} accumulate {int(acc)}:"]
                for tag, fn, wbytes in (("kernel", lambda: ops.moe_wgrad_rel(G, X, W, plan, mode, w=w, out=out, accumulate=acc), 2.0),
                                        ("kernel mxfp4", lambda: ops.moe_wgrad_rel(G, X, Wq, plan, mode, w=w, out=out, accumulate=acc), 17 / 32),
                                        ("torch per-expert loop", lambda: composition(acc), 2.0)):
                    out.zero_()
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    med, best = timed(fn, a.reps)
                    nbytes = E * N * K * (4.0 * (2 if acc else 1) + wbytes)
                    floor = nbytes / HBM * 1e3
                    row.append(f"{tag} {med:7.3f} ms ({best:7.3f})" + (f" = {med / floor:4.2f} x the floor {floor:.3f} ms" if "kernel" in tag else ""))
                say("  ".join(row))
            del G, X, W, Wq, out
    # the epilogue's store shape alone: a plan whose slots are all skipped leaves every expert without rows, and the kernel then only writes
    # its zeros -- one float4 per lane at the 16 x 16 accumulator's addresses (4 segments of 64 B per wave instruction) -- next to a fill
    say("store shape alone (every expert without rows: the kernel writes exact zeros at the accumulator's addresses), against out.zero_():")
    T = 2048
    none = ops.MoePlan(torch.full((T, K_SLOTS), E, device="cuda", dtype=torch.int64), E)
    for mode, N, K in (("gate_up", 2 * I, H), ("down", H, I)):
        gr, xr = (T * K_SLOTS, T) if mode == "gate_up" else (T, T * K_SLOTS)
        G, X = torch.zeros(gr, N, device="cuda", dtype=torch.bfloat16), torch.zeros(xr, K, device="cuda", dtype=torch.bfloat16)
        W, w = torch.zeros(E, N, K, device="cuda", dtype=torch.bfloat16), torch.zeros(T, K_SLOTS, device="cuda", dtype=torch.bfloat16)
        out = torch.ones(E, N, K, device="cuda")
        row = [f"{mode:8s} [{E}, {N}, {K}] fp32 = {4e-9 * E * N * K:.2f} GB:"]
        for tag, fn in (("kernel", lambda: ops.moe_wgrad_rel(G, X, W, none, mode, w=w, out=out)), ("out.zero_()", lambda: out.zero_())):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            med, best = timed(fn, a.reps)
            row.append(f"{tag} {med:7.3f} ms ({best:7.3f}) = {4e-9 * E * N * K / med:5.2f} TB/s")
        assert not bool(out.any())
        say("  ".join(row))
        del G, X, W, out
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
