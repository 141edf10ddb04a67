#!/usr/bin/env python3
"""The Gemma-3 read-outs on the MI355X, at the Gemma-3-4B layer shape: B = 4, S = 2048, 8 query / 4 kv heads of
d = 256, bf16; medians of device-event timings.
  (1) lrp_attn_relmap_d256 alone (all 8 heads into one map, and one head) next to two yardsticks of the same process: (a) a torch restatement
      that materialises [B, nq, S, S] -- the only alternative a user has --, (b) lrp_attn_fwd at the same shape (the same number of
      contractions); both ratios are printed; with a sliding window of 1024 folded into the row intervals as well (the local layers' call);
  (2) the per-step cost of Gemma3LRP.explain(attn_map="sum"), of one (layer, head) pair and of the other read-outs against a plain explain()
      of the same process, on the step tools/gemma3_engine_bench.py times (Gemma-3-4B shape: --layers 34, H 2560, I 10240, window 1024,
      5 local : 1 global, vocab 262208 tied; random weights on the device); the requests alternate inside each round.
usage: python tools/gemma3_readout_bench.py [--out profiles/gemma3_readout_bench.txt] [--layers 34] [--reps 10] [--rounds 5]"""
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
    ap.add_argument("--layers", type=int, default=34)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-engine", action="store_true", help="the kernel part only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemma3_readout_bench needs a HIP device")
    from lxt_amd import ops
    from lxt_amd.engine_gemma3 import Gemma3LRP
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- (1) the kernel and its yardsticks
    B, S, nq, nk, d, win = 4, 2048, 8, 4, 256, 1024
    scale = 256 ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    q, gq = (torch.randn(B * S, nq * d, generator=g, device="cuda").bfloat16() for _ in range(2))
    k, v = (torch.randn(B * S, nk * d, generator=g, device="cuda").bfloat16() for _ in range(2))
    o, lse, out = torch.empty_like(q), torch.empty(B, nq, S, device="cuda"), torch.empty(B, S, S, device="cuda")
    v_t = ops.transpose_heads(v, B, S, nk, d) if ops.attn_needs_transposed(q, d) else None
    up = torch.ones(S, S, dtype=torch.bool, device="cuda").triu(1)
    i = torch.arange(S, device="cuda", dtype=torch.int32)
    iv = ((i - (win - 1)).clamp_min(0)[None].expand(B, S).contiguous(), (i + 1)[None].expand(B, S).contiguous())

    def restated():
        hd = lambda t, nh: t.view(B, S, nh, d).transpose(1, 2)                    # noqa: E731
        kh, vh = hd(k, nk).repeat_interleave(nq // nk, 1), hd(v, nk).repeat_interleave(nq // nk, 1)
        P = torch.exp((hd(q, nq) @ kh.transpose(2, 3)).float() * scale - lse[..., None])
        return (P * (hd(gq, nq) @ vh.transpose(2, 3)).float()).masked_fill_(up, 0.0).sum(1)

    rm = lambda **kw: ops.attn_relmap(q, k, v, gq, lse, B, S, nq, nk, d, scale, out=out, **kw)      # noqa: E731
    runs = (("lrp_attn_fwd (yardstick b: the same number of contractions)", lambda: ops.attn_fwd(q, k, v, v_t, o, lse, B, S, nq, nk, d, scale)),
            ("lrp_attn_relmap_d256, 8 heads into one map", rm),
            ("lrp_attn_relmap_d256, one head", lambda: rm(heads=(5, 6))),
            ("lrp_attn_relmap_d256, 8 heads, window 1024 in the intervals", lambda: rm(row_iv=iv)),
            ("torch restatement materialising [B, nq, S, S] (yardstick a)", restated))
    med = {}
    for name, fn in runs:
        for _ in range(3):
            fn()
        med[name], best = timed(fn, 20)
        say(f"{name:62s}: {med[name] * 1e3:9.1f} us median, {best * 1e3:9.1f} us best over 20 calls  (bf16 B={B} S={S} nq={nq} nk={nk} d={d})")
    km = med[runs[1][0]]
    say(f"  lrp_attn_relmap_d256 / lrp_attn_fwd = {km / med[runs[0][0]]:.2f};  torch restatement / lrp_attn_relmap_d256 = {med[runs[4][0]] / km:.2f}; "
        f"causal flops 2 x 2 B nq d S^2 / 2 = {2 * B * nq * d * S * S / 1e9:.0f} GF -> {2 * B * nq * d * S * S / km / 1e9:.0f} TF/s; "
        f"the map itself, B S^2 fp32 = {B * S * S * 4 / 1e6:.0f} MB written")
    err = float((restated() - rm().clone()).abs().max() / out.abs().max())
    say(f"  the two agree to {err:.1e} of the largest value (the restatement's products are bf16 GEMM outputs)")
    del q, gq, k, v, o, lse, out, v_t
    if not a.no_engine:
        engine_part(a, say, Gemma3LRP, B, S)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def engine_part(a, say, Gemma3LRP, B, S):
    H, I, d, nq, nk, L, V = 2560, 10240, 256, 8, 4, a.layers, 262208
    g = torch.Generator(device="cuda").manual_seed(1)
    types = [("full_attention" if (i + 1) % 6 == 0 else "sliding_attention") for i in range(L)]
    inv = lambda theta: 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))      # noqa: E731
    cfg = dict(hidden=H, inter=I, n_layers=L, n_heads=nq, n_kv=nk, head_dim=d, vocab=V, rms_eps=1e-6, act="gelu_tanh", scale=256 ** -0.5,
               layer_types=types, window=1024, rope={"sliding_attention": (inv(1e4), 1.0), "full_attention": (inv(1e6), 1.0)}, embed_scale=H ** 0.5)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()      # noqa: E731
    nw = lambda n: (torch.randn(n, generator=g, device="cuda") * 0.1).bfloat16()         # noqa: E731
    emb = rn(V, H)
    W = dict(embed=emb, norm=nw(H), lm_head=emb,
             layers=[dict(ln_in=nw(H), ln_pa=nw(H), ln_pf=nw(H), ln_pff=nw(H), qn=nw(d), kn=nw(d), wq=rn(nq * d, H), wk=rn(nk * d, H),
                          wv=rn(nk * d, H), wo=rn(H, nq * d), wg=rn(I, H), wu=rn(I, H), wd=rn(H, I)) for _ in range(L)])
    eng = Gemma3LRP(cfg, W, dtype=torch.bfloat16, max_seq=S)
    del W, emb
    ids = torch.randint(0, 262000, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
    reqs = dict(plain={}, sum=dict(attn_map="sum"), pair=dict(attn_map=[(L // 2, 5)]), heads=dict(heads=("out", "q", "k", "v")),
                latent=dict(layer_relevance=True, latent=("trace", "resid", "mlp")))
    eng.explain(ids)
    torch.cuda.synchronize()
    arena_plain = eng._arena.nbytes()
    for kw in reqs.values():                                    # warm-up: every shape, every arena buffer
        for _ in range(2):
            eng.explain(ids, **kw)
    torch.cuda.synchronize()
    steps = max(1, a.reps // a.rounds)
    ts = {k: [] for k in reqs}
    for _ in range(a.rounds):
        for k, kw in reqs.items():
            ts[k].append(timed(lambda: eng.explain(ids, **kw), steps)[0])
    base = statistics.median(ts["plain"])
    say(f"engine bf16, Gemma-3-4B shape, {L} layers, B={B} S={S} (M = {B * S} rows), median of {a.rounds} rounds x {steps} steps, requests alternating:")
    for k in reqs:
        m = statistics.median(ts[k])
        say(f"  {k:6s}: {m:8.2f} ms per step   +{m - base:6.2f} ms  ({100 * (m - base) / base:+5.1f} %)  = {(m - base) / L * 1e3:7.1f} us per layer"
            f"   [spread {min(ts[k]):.2f} .. {max(ts[k]):.2f}]")
    say(f"  arena after a plain call {arena_plain / 2**30:.2f} GiB, after every request {eng._arena.nbytes() / 2**30:.2f} GiB (kept h: {L} x {B * S} x {H}, "
        f"kept m: {L} x {B * S} x {I} bf16); R_attn {L} x {B} x {S} x {S} fp32 = {L * B * S * S * 4 / 2**30:.2f} GiB, allocated per call")


if __name__ == "__main__":
    main()
