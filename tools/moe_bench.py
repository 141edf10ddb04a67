#!/usr/bin/env python3
"""Routed-expert LRP on the grouped HIP GEMMs (csrc/moe.hip) at the Qwen3-30B-A3B layer: H 2048, moe_intermediate_size 768, 128 experts,
top-8, bf16.   python tools/moe_bench.py [--out profiles/moe_bench.txt] [--no-e2e]

  1. per launch, T = 2048 and 8192 tokens: us, fraction of 2.5 PFLOP/s (a grouped GEMM's own FLOP; per direction 2 T k 3 H I) and fraction
     of 8 TB/s on weight bytes (each expert's 3 H I weights counted once per direction);
  2. the reference's per-expert loop (ref: lxt/efficient/models/qwen3_moe.py:14-44: a host-synced expert list, then per expert a gather,
     two Linears, the rule ops and index_add_) composed from existing lxt_amd ops (LinearFn, GatedActFn, divide_gradient), forward +
     backward, against MoEExpertsFn;
  3. end to end: a randomly initialised bf16 Qwen3MoeForCausalLM at the Qwen3-30B-A3B shape (48 layers, 32 q / 4 kv heads of 128) under
     lxt_amd.efficient.monkey_patch, the quickstart protocol at S = 2048 for 1 and 4 prompts: explanations per second."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import lxt_amd  # noqa: E402,F401
import lxt_amd.ops as ops  # noqa: E402

H, I, E, K = 2048, 768, 128, 8
PEAK_FLOPS, PEAK_BW = 2.5e15, 8e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us


def layer(T, Wgu, Wd, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T, H, device="cuda", generator=g, dtype=torch.bfloat16)
    idx = torch.rand(T, E, device="cuda", generator=g).argsort(1)[:, :K].contiguous()
    w = (torch.rand(T, K, device="cuda", generator=g) / K).to(torch.bfloat16)
    G = torch.randn(T, H, device="cuda", generator=g, dtype=torch.bfloat16)
    R = T * K
    plan = ops.MoePlan(idx, E)
    coef, m = ops.moe_gate_up_fwd(x, Wgu, plan)
    y = ops.moe_down_fwd(m, Wd, plan)
    Agu, _ = ops.moe_down_dgrad(G, Wd, coef, m, w, plan)
    gxr = ops.moe_gate_up_dgrad(Agu, Wgu, plan)
    f_gu, f_dn = 2.0 * R * 2 * I * H, 2.0 * R * H * I
    wb_gu, wb_dn = E * 2 * I * H * 2, E * H * I * 2
    rows = [("plan", lambda: ops.MoePlan(idx, E), 0, 0),
            ("gate_up_fwd (gather + coef epilogue)", lambda: ops.moe_gate_up_fwd(x, Wgu, plan), f_gu, wb_gu),
            ("down_fwd", lambda: ops.moe_down_fwd(m, Wd, plan), f_dn, wb_dn),
            ("combine_fwd", lambda: ops.moe_combine(y, plan, w), 0, 0),
            ("down_dgrad (gather + rule epilogue + G_w)", lambda: ops.moe_down_dgrad(G, Wd, coef, m, w, plan), f_dn, wb_dn),
            ("gate_up_dgrad", lambda: ops.moe_gate_up_dgrad(Agu, Wgu, plan), f_gu, wb_gu),
            ("combine_bwd", lambda: ops.moe_combine(gxr, plan), 0, 0)]
    say(f"\n== T = {T} tokens, {R} routed rows (~{R / E:.0f} per expert), bf16")
    say(f"{'launch':44s} {'us':>9s} {'PFLOP/s frac':>13s} {'8TB/s frac (weights)':>21s}")
    gemm_us, gemm_f, out = 0.0, 0.0, {}
    for name, fn, f, wb in rows:
        us = timed(fn)
        out[name.split(" ")[0]] = us
        fr = f / (us * 1e-6) / PEAK_FLOPS if f else 0.0
        br = wb / (us * 1e-6) / PEAK_BW if wb else 0.0
        say(f"{name:44s} {us:9.1f} {fr:13.3f} {br:21.3f}")
        if f:
            gemm_us += us
            gemm_f += f
    fwd = out["plan"] + out["gate_up_fwd"] + out["down_fwd"] + out["combine_fwd"]
    bwd = out["down_dgrad"] + out["gate_up_dgrad"] + out["combine_bwd"]
    say(f"four grouped GEMMs: {gemm_us:.1f} us = {gemm_f / (gemm_us * 1e-6) / PEAK_FLOPS:.3f} of 2.5 PFLOP/s, "
        f"{2 * (wb_gu + wb_dn) / (gemm_us * 1e-6) / PEAK_BW:.3f} of 8 TB/s on weight bytes")
    say(f"layer sum of launches: forward {fwd:.1f} us, backward {bwd:.1f} us")
    # whole Function, forward + backward (with allocations and Python)
    from lxt_amd.efficient.moe import MoEExpertsFn

    def fn_hip():
        xr = x.detach().requires_grad_()
        wr = w.detach().requires_grad_()
        MoEExpertsFn.apply(xr, idx, wr, Wgu, Wd, "silu").backward(G)
    t_hip = timed(fn_hip, reps=10)
    t_loop = timed(lambda: loop_baseline(x, idx, w, Wgu, Wd, G), reps=3, warm=1)
    say(f"MoEExpertsFn forward + backward: {t_hip:.1f} us | reference-style per-expert loop on lxt_amd ops: {t_loop:.1f} us "
        f"-> {t_loop / t_hip:.1f}x")
    return dict(T=T, launches_us=out, gemm_us=gemm_us, gemm_flop_frac=gemm_f / (gemm_us * 1e-6) / PEAK_FLOPS,
                gemm_weight_bw_frac=2 * (wb_gu + wb_dn) / (gemm_us * 1e-6) / PEAK_BW, fn_us=t_hip, loop_us=t_loop, speedup=t_loop / t_hip)


def loop_baseline(x, idx, w, Wgu, Wd, G):
    """the reference's experts_forward loop over lxt_amd's per-op Functions (what a user could compose from today's primitives)"""
    from lxt_amd.efficient.functions import GatedActFn, LinearFn
    from lxt_amd.efficient.rules import divide_gradient
    xr = x.detach().requires_grad_()
    wr = w.detach().requires_grad_()
    out = torch.zeros_like(xr)
    with torch.no_grad():
        mask = torch.nn.functional.one_hot(idx, num_classes=E).permute(2, 1, 0)
        hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
    for e in hit:
        e = int(e[0])
        pos, tok = torch.where(mask[e])
        gu = LinearFn.apply(xr[tok], Wgu[e], None)
        g, u = gu.chunk(2, dim=-1)
        m = divide_gradient(GatedActFn.apply(g.contiguous(), u.contiguous(), "silu"), 2)
        y = LinearFn.apply(m, Wd[e], None) * wr[tok, pos, None]
        out = out.index_add(0, tok, divide_gradient(y, 2))
    out.backward(G)


def e2e(prompts_list=(1, 4), S=2048):
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    from lxt_amd.efficient import monkey_patch
    monkey_patch(modeling_qwen3_moe)
    cfg = Qwen3MoeConfig(hidden_size=2048, moe_intermediate_size=768, num_experts=128, num_experts_per_tok=8, num_hidden_layers=48,
                         num_attention_heads=32, num_key_value_heads=4, head_dim=128, intermediate_size=6144, vocab_size=151936,
                         norm_topk_prob=True, attn_implementation="sdpa", max_position_embeddings=4096)
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)           # built in bf16 on the device (an fp32 build would need 120 GB first)
    with torch.device("cuda"):
        model = Qwen3MoeForCausalLM(cfg).eval()
    torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.requires_grad_(False)
            if "norm" in name:
                p.fill_(1.0)
            else:
                p.normal_(0.0, 0.02 if "experts" not in name else p.shape[-1] ** -0.5)
    say(f"\n== end to end: Qwen3MoeForCausalLM at the 30B-A3B shape, {sum(p.numel() for p in model.parameters()) / 1e9:.1f} B parameters, "
        f"bf16, S = {S}, quickstart protocol (inputs_embeds, arg-max logit of the last position, backward, (e * e.grad).sum(-1))")
    res = {}
    for B in prompts_list:
        ids = torch.randint(0, cfg.vocab_size, (B, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))

        def one():
            e = model.get_input_embeddings()(ids).detach().requires_grad_()
            logits = model(inputs_embeds=e, use_cache=False, logits_to_keep=1).logits[:, -1]
            idx = logits.argmax(-1)
            logits[torch.arange(B, device="cuda"), idx].sum().backward()
            return (e * e.grad).sum(-1)
        R = one()
        assert torch.isfinite(R.float()).all()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 3
        for _ in range(n):
            one()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        res[B] = B / dt
        say(f"{B} prompt(s): {dt * 1e3:.0f} ms per explain call -> {B / dt:.2f} expl/s  (peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}; layer H {H}, I {I}, {E} experts, top-{K}")
    g = torch.Generator(device="cuda").manual_seed(1)
    Wgu = (torch.randn(E, 2 * I, H, device="cuda", generator=g) * H ** -0.5).to(torch.bfloat16)
    Wd = (torch.randn(E, H, I, device="cuda", generator=g) * I ** -0.5).to(torch.bfloat16)
    result = dict(layers=[layer(T, Wgu, Wd) for T in (2048, 8192)])
    del Wgu, Wd
    torch.cuda.empty_cache()
    if not a.no_e2e:
        result["e2e_expl_per_s"] = e2e()
    say("JSON " + json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
