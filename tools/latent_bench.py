#!/usr/bin/env python3
"""Latent feature attribution read-outs on the MI355X:
  (1) lrp_colsum_dot at the Llama-3-8B shapes, B S = 8192 rows (B = 4, S = 2048), N = 4096 (residual dims) and N = 14336 (MLP neurons), bf16:
      time per call from device events (median over --reps timed calls after warm-up) and the bytes the algorithm must read, 2 B S N 2,
      over it -- and that rate over the 8 TB/s HBM peak;
  (2) the per-step overhead of each LlamaLRP.explain(latent=...) option against a plain explain(), bf16, at the Llama-3-8B layer shape
      (H 4096, I 14336, 32 / 8 heads of 128) with --layers layers, B = 4, S = 2048; the requests alternate inside each round.
  --heads: the per-head attention read-outs instead (profiles/heads_bench.txt):
  (3) lrp_headdot at B S = 8192 rows, 32 query heads of 128, bf16: rep = 1 (q, o) and rep = 4 (k, v over 8 kv heads), with and without the
      rotated form, the bytes the algorithm must read (x, g and the fp32 output) over the median time, next to lrp_colsum_dot in the same run;
  (4) the per-step overhead of each LlamaLRP.explain(heads=...) name, and of all four, against a plain explain() of the same process.
  --attn-map: the token-to-token attention relevance maps instead (profiles/attn_map_bench.txt), B = 4, S = 2048,
  32 / 8 heads of 128, bf16:
  (5) lrp_attn_relmap alone (all 32 heads into one map, and one head), next to two yardsticks of the same process: lrp_attn_fwd at the same
      shape (the same number of contractions) and a torch restatement that materialises [B, nq, S, S];
  (6) the per-step overhead of explain(attn_map="sum") and of one (layer, head) pair against a plain explain() (--layers 32 for the figure
      the design document quotes).
usage: python tools/latent_bench.py [--heads | --attn-map] [--out FILE] [--layers 2] [--reps 20] [--rounds 5]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


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
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--heads", action="store_true", help="measure lrp_headdot and explain(heads=...) instead of the latent options")
    ap.add_argument("--attn-map", action="store_true", help="measure lrp_attn_relmap and explain(attn_map=...) instead of the latent options")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_bench needs a HIP device")
    from lxt_amd import ops
    import lxt_amd.engine as E
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- (1) the kernel
    B, S = 4, 2048
    g = torch.Generator(device="cuda").manual_seed(0)
    for N, pad in () if a.attn_map else ((4096, 0), (14336, 64)):
        x = torch.randn(B * S, N + pad, generator=g, device="cuda").bfloat16()[:, :N]
        y = torch.randn(B * S, N + pad, generator=g, device="cuda").bfloat16()[:, :N]
        out = torch.empty(B, N, device="cuda")
        for _ in range(5):
            ops.colsum_dot(x, y, B, S, out=out)
        med, best = timed(lambda: ops.colsum_dot(x, y, B, S, out=out), 50)
        nbytes = 2 * B * S * N * 2
        say(f"colsum_dot bf16 B={B} S={S} N={N} (row pitch {N + pad}): {med * 1e3:7.1f} us median, {best * 1e3:7.1f} us best over 50 calls; "
            f"{nbytes / 1e6:.0f} MB read -> {nbytes / med / 1e9:.2f} TB/s median = {nbytes / med / 1e9 / 8.0:.2f} of 8 TB/s "
            f"(best {nbytes / best / 1e9:.2f} TB/s); workspace {ops.lib.lrp_colsum_dot_ws(B, S, N) / 1e6:.1f} MB of fp32 partials")
        del x, y

    # ---- (3) the per-head kernel
    if a.heads:
        nq, d = 32, 128
        cos, sin = E.rope_tables(1.0 / (5e5 ** (torch.arange(0, d, 2, dtype=torch.float32) / d)), 1.0, S, torch.bfloat16, "cuda")
        for r in (1, 4):
            x = torch.randn(B * S, nq // r * d, generator=g, device="cuda").bfloat16()
            y = torch.randn(B * S, nq * d, generator=g, device="cuda").bfloat16()
            out = torch.empty(B, nq, S, device="cuda")
            for rope in (None, (cos, sin)):
                for _ in range(5):
                    ops.headdot(x, y, B, S, nq, r, d, rope=rope, out=out)
                med, best = timed(lambda: ops.headdot(x, y, B, S, nq, r, d, rope=rope, out=out), 50)
                nbytes = (x.numel() + y.numel()) * 2 + out.numel() * 4
                say(f"headdot bf16 B={B} S={S} nh={nq} rep={r} d={d} {'rotated' if rope else 'plain  '}: {med * 1e3:7.1f} us median, {best * 1e3:7.1f} us "
                    f"best over 50 calls; {nbytes / 1e6:.0f} MB -> {nbytes / med / 1e6:.0f} GB/s median = {nbytes / med / 1e9 / 8.0:.2f} of 8 TB/s "
                    f"(best {nbytes / best / 1e6:.0f} GB/s)")
            del x, y
    # ---- (5) the token-to-token kernel and its yardsticks
    if a.attn_map:
        nq, nk, d = 32, 8, 128
        scale = d ** -0.5
        q, gq = (torch.randn(B * S, nq * d, generator=g, device="cuda").bfloat16() for _ in range(2))
        k, v = (torch.randn(B * S, nk * d, generator=g, device="cuda").bfloat16() for _ in range(2))
        o, lse, out = torch.empty_like(q), torch.empty(B, nq, S, device="cuda"), torch.empty(B, S, S, device="cuda")
        up = torch.ones(S, S, dtype=torch.bool, device="cuda").triu(1)

        def restated():
            hd = lambda t, nh: t.view(B, S, nh, d).transpose(1, 2)                    # noqa: E731
            kh, vh = hd(k, nk).repeat_interleave(nq // nk, 1), hd(v, nk).repeat_interleave(nq // nk, 1)
            P = torch.exp((hd(q, nq) @ kh.transpose(2, 3)).float() * scale - lse[..., None])
            return (P * (hd(gq, nq) @ vh.transpose(2, 3)).float()).masked_fill_(up, 0.0).sum(1)

        runs = (("lrp_attn_fwd (yardstick: the same number of contractions)", lambda: ops.attn_fwd(q, k, v, None, o, lse, B, S, nq, nk, d, scale)),
                ("lrp_attn_relmap, 32 heads into one map", lambda: ops.attn_relmap(q, k, v, gq, lse, B, S, nq, nk, d, scale, out=out)),
                ("lrp_attn_relmap, one head", lambda: ops.attn_relmap(q, k, v, gq, lse, B, S, nq, nk, d, scale, heads=(5, 6), out=out)),
                ("torch restatement materialising [B, nq, S, S]", restated))
        med = {}
        for name, fn in runs:
            for _ in range(3):
                fn()
            med[name], best = timed(fn, 20)
            say(f"{name:62s}: {med[name] * 1e3:9.1f} us median, {best * 1e3:9.1f} us best over 20 calls  (bf16 B={B} S={S} nq={nq} nk={nk} d={d})")
        km = med[runs[1][0]]
        say(f"  lrp_attn_relmap / lrp_attn_fwd = {km / med[runs[0][0]]:.2f};  torch restatement / lrp_attn_relmap = {med[runs[3][0]] / km:.2f}; "
            f"causal flops 2 x 2 B nq d S^2 / 2 = {2 * B * nq * d * S * S / 1e9:.0f} GF -> {2 * B * nq * d * S * S / km / 1e9:.0f} TF/s")
        err = float((restated() - out.copy_(ops.attn_relmap(q, k, v, gq, lse, B, S, nq, nk, d, scale))).abs().max() / out.abs().max())
        say(f"  the two agree to {err:.1e} of the largest value (the restatement's products are bf16 GEMM outputs)")
        del q, gq, k, v, o, lse, out
    # ---- (2) the engine
    H, I, d, L = 4096, 14336, 128, a.layers
    cfg = dict(hidden=H, inter=I, n_layers=L, n_heads=32, n_kv=8, head_dim=d, vocab=4096, rope_theta=5e5, rms_eps=1e-5)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()      # noqa: E731
    ones = lambda: torch.ones(H, device="cuda").bfloat16()                                # noqa: E731
    W = dict(embed=rn(4096, H), norm=ones(), lm_head=rn(4096, H),
             layers=[dict(ln1=ones(), ln2=ones(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(L)])
    eng = E.LlamaLRP(cfg, W, dtype=torch.bfloat16, mode="efficient", max_seq=S)
    del W
    ids = torch.randint(0, 4096, (B, S), generator=torch.Generator().manual_seed(1)).cuda()
    reqs = dict(plain=None, trace=("trace",), resid=("resid",), mlp=("mlp",), all=("trace", "resid", "mlp"))
    kw = "latent"
    if a.heads:
        reqs, kw = dict(plain=None, out=("out",), q=("q",), k=("k",), v=("v",), all=E.HEADS), "heads"
    if a.attn_map:
        reqs, kw = dict(plain=None, sum="sum", pair=[(L // 2, 5)]), "attn_map"
    for lat in reqs.values():                                   # warm-up: every shape, every arena buffer
        for _ in range(2):
            eng.explain(ids, **{kw: lat})
    torch.cuda.synchronize()
    arena0 = eng._arena.nbytes()
    ts = {k: [] for k in reqs}
    for _ in range(a.rounds):
        for k, lat in reqs.items():
            ts[k].append(timed(lambda: eng.explain(ids, **{kw: lat}), max(1, a.reps // a.rounds))[0])
    base = statistics.median(ts["plain"])
    say(f"engine bf16, Llama-3-8B layer shape, {L} layers, B={B} S={S} (M = {B * S} rows), median of {a.rounds} rounds x "
        f"{max(1, a.reps // a.rounds)} steps, requests alternating:")
    for k in reqs:
        m = statistics.median(ts[k])
        say(f"  {kw}={k:6s}: {m:8.2f} ms per step   +{m - base:6.2f} ms  ({100 * (m - base) / base:+5.1f} %)  "
            f"= {(m - base) / L * 1e3:7.1f} us per layer   [spread {min(ts[k]):.2f} .. {max(ts[k]):.2f}]")
    say(f"  arena after every request: {arena0 / 2**30:.2f} GiB" + (f"; outputs {L} x {B} x 32 x {S} fp32 = {L * B * 32 * S * 4 / 2**20:.0f} MiB per name"
                                                                    if a.heads else
                                                                    f"; R_attn {L} x {B} x {S} x {S} fp32 = {L * B * S * S * 4 / 2**30:.2f} GiB" if a.attn_map else
                                                                    f" (kept m: {L} x {B * S} x {I} bf16 = {L * B * S * I * 2 / 2**30:.2f} GiB of it)"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
