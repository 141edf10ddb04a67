#!/usr/bin/env python3
"""lrp_wgrad_rel on the MI355X: the per-weight relevance kernel at the four Llama-3-8B layer shapes
(qkv [6144, 4096], o [4096, 4096], gate_up [28672, 4096], down [4096, 14336]), M = 8192 and M = 2048 tokens, bf16, accumulating into an
fp32 [N, K] result as the dataset-level use does.  Per shape, from device events (median over --reps timed calls after warm-up):
  * the kernel: out += W (*) (G rs)^T X in one launch, time and TFLOP/s (2 M N K);
  * the composition a user would otherwise write: torch.matmul((G * rs).T, X) in bf16 -> fp32, times W, added to out;
  * the same shape's dgrad in this library, c [M, K] = G [M, N] W [N, K] (ops.linear_dgrad): the same FLOPs on the tuned GEMM.
usage: python tools/wgrad_bench.py [--out FILE] [--reps 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

SHAPES = (("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336))


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
        raise SystemExit("wgrad_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(0)
    say("out [N, K] fp32 += W (*) (G rs)^T X, bf16 operands; ms = median (min) of device-event times; TFLOP/s = 2 M N K / median")
    for M in (8192, 2048):
        for name, N, K in SHAPES:
            G = torch.randn(M, N, generator=g, device="cuda").bfloat16()
            X = torch.randn(M, K, generator=g, device="cuda").bfloat16()
            W = (torch.randn(N, K, generator=g, device="cuda") * 0.02).bfloat16()
            rs = torch.rand(M, generator=g, device="cuda") + 0.5
            out = torch.zeros(N, K, device="cuda")
            c = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
            flops = 2.0 * M * N * K

            def kernel():
                ops.wgrad_rel(G, X, W, out=out, rs=rs, accumulate=True)

            def composition():
                out.add_(torch.matmul((G * rs[:, None].to(G.dtype)).T, X).float() * W)

            def dgrad():
                ops.linear_dgrad(G, W, out=c)

            row = [f"M {M:5d} {name:8s} N {N:5d} K {K:5d}:"]
            for tag, fn in (("wgrad_rel", kernel), ("torch composition", composition), ("dgrad", dgrad)):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                med, best = timed(fn, a.reps)
                row.append(f"{tag} {med:7.3f} ms ({best:7.3f}) {flops / med / 1e9:7.1f} TFLOP/s")
            say("  ".join(row))
            del G, X, W, out, c
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
