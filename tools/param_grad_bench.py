#!/usr/bin/env python3
"""lrp_wgrad on the MI355X: the plain weight gradient out [N, K] = G^T X of a trainable Linear under the drop-in patches,
bf16, at the four Llama-3-8B layer shapes (qkv [6144, 4096], o [4096, 4096], gate_up [28672, 4096], down [4096, 14336]), M = 2048 and
M = 8192 tokens.  Per shape, from device events (median over --reps timed calls after warm-up):
  * the kernel: ops.wgrad(G, X, out=out), one launch, time and TFLOP/s (2 M N K);
  * what ATen runs for the same gradient: torch.matmul(G.T, X, out=out) in bf16;
  * the ratio kernel / torch (below 1: the kernel is faster).
usage: python tools/param_grad_bench.py [--out FILE] [--reps 20]"""
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
        raise SystemExit("param_grad_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(0)
    say("out [N, K] bf16 = G^T X, bf16 operands; ms = median (min) of device-event times; TFLOP/s = 2 M N K / median; ratio = lrp_wgrad / torch")
    for M in (2048, 8192):
        for name, N, K in SHAPES:
            G = torch.randn(M, N, generator=g, device="cuda").bfloat16()
            X = torch.randn(M, K, generator=g, device="cuda").bfloat16()
            out = torch.empty(N, K, device="cuda", dtype=torch.bfloat16)
            ref = torch.empty(N, K, device="cuda", dtype=torch.bfloat16)
            flops = 2.0 * M * N * K

            def kernel():
                ops.wgrad(G, X, out=out)

            def aten():
                torch.matmul(G.T, X, out=ref)

            row, med = [f"M {M:5d} {name:8s} N {N:5d} K {K:5d}:"], {}
            for tag, fn in (("lrp_wgrad", kernel), ("torch G.T @ X", aten)):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                med[tag], best = timed(fn, a.reps)
                row.append(f"{tag} {med[tag]:7.3f} ms ({best:7.3f}) {flops / med[tag] / 1e9:7.1f} TFLOP/s")
            row.append(f"ratio {med['lrp_wgrad'] / med['torch G.T @ X']:.2f}")
            say("  ".join(row))
            del G, X, out, ref
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
