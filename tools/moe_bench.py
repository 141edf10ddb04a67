#!/usr/bin/env python3
"""Routed-expert LRP on the grouped HIP GEMMs (csrc/moe.hip) at the Qwen3-30B-A3B layer: H 2048, moe_intermediate_size 768, 128 experts,
top-8, bf16.   python tools/moe_bench.py [--out profiles/moe_bench.txt] [--no-e2e]
                python tools/moe_bench.py --engine [--out profiles/moe_engine_bench.txt]      (items 4 and 5 only)

  1. per launch, T = 2048 and 8192 tokens: us, fraction of 2.5 PFLOP/s (a grouped GEMM's own FLOP; per direction 2 T k 3 H I) and fraction
     of 8 TB/s on weight bytes (each expert's 3 H I weights counted once per direction);
  2. the reference's per-expert loop (ref: lxt/efficient/models/qwen3_moe.py:14-44: a host-synced expert list, then per expert a gather,
     two Linears, the rule ops and index_add_) composed from existing lxt_amd ops (LinearFn, GatedActFn, divide_gradient), forward +
     backward, against MoEExpertsFn;
  3. end to end: a randomly initialised bf16 Qwen3MoeForCausalLM at the Qwen3-30B-A3B shape (48 layers, 32 q / 4 kv heads of 128) under
     lxt_amd.efficient.monkey_patch, the quickstart protocol at S = 2048 for 1 and 4 prompts: explanations per second;
  4. --engine: the same model, in the same run, through the drop-in protocol of item 3 and through the fused driver
     lxt_amd.engine_qwen_moe.Qwen3MoeLRP.explain (with and without experts=True);
  5. --engine: the three router kernels of csrc/moe_router.hip alone at T = 8192, E = 128, k = 8, against the bytes they must move."""
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


def build_30b_a3b():
    """a randomly initialised bf16 Qwen3MoeForCausalLM at the Qwen3-30B-A3B shape, on the device, parameters frozen"""
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
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
    return model


def e2e(prompts_list=(1, 4), S=2048, model=None):
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    from lxt_amd.efficient import monkey_patch
    monkey_patch(modeling_qwen3_moe)
    model = build_30b_a3b() if model is None else model
    cfg = model.config
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


def router_kernels(T=8192):
    """the router forward, backward and the expert read-out alone, bf16: us and the fraction of 8 TB/s on the bytes each must move"""
    g = torch.Generator(device="cuda").manual_seed(2)
    logits = torch.randn(T, E, device="cuda", generator=g).to(torch.bfloat16)
    idx, w, lse = ops.moe_router_fwd(logits, K, True)
    gw = torch.randn(T, K, device="cuda", generator=g).to(torch.bfloat16)
    out, rel = torch.empty_like(logits), torch.empty(4, E, device="cuda", dtype=torch.float32)
    slots = T * K * (8 + 2)                                   # idx int64 + one bf16 value per slot
    rows = [("moe_router_fwd", lambda: ops.moe_router_fwd(logits, K, True), T * E * 2 + slots + T * 4),
            ("moe_router_bwd", lambda: ops.moe_router_bwd(logits, lse, idx, w, gw, True, out=out), 2 * T * E * 2 + slots + T * K * 2 + T * 4),
            ("moe_expert_relevance (4 prompts)", lambda: ops.moe_expert_relevance(idx, w, gw, 4, T // 4, E, out=rel), slots + T * K * 2 + 4 * E * 4)]
    say(f"\n== router kernels alone, T = {T}, E = {E}, k = {K}, bf16 (renorm)")
    say(f"{'launch':36s} {'us':>8s} {'bytes':>10s} {'8TB/s frac':>11s}")
    res = {}
    for name, fn, nbytes in rows:
        us = timed(fn, reps=50)
        res[name.split(" ")[0]] = us
        say(f"{name:36s} {us:8.1f} {nbytes:10d} {nbytes / (us * 1e-6) / PEAK_BW:11.4f}")
    return res


def engine_bench(prompts_list=(1, 4), S=2048):
    """items 4 and 5: the drop-in and the fused driver on ONE model in ONE run"""
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    model = build_30b_a3b()
    drop = e2e(prompts_list, S, model)
    eng = Qwen3MoeLRP.from_hf(model, max_seq=S)
    say(f"\n== the same model through Qwen3MoeLRP.explain (flat buffer {eng.flat.numel() * 2 / 2**30:.1f} GiB next to the expert weights, read as stored)")
    res = {}
    for B in prompts_list:
        ids = torch.randint(0, model.config.vocab_size, (B, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        for tag, kw in (("explain", {}), ("explain(experts=True)", dict(experts=True))):
            out = eng.explain(ids, **kw)
            assert torch.isfinite(out["R_tok"]).all()
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 3
            for _ in range(n):
                eng.explain(ids, **kw)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            res[f"{B}/{tag}"] = B / dt
            say(f"{B} prompt(s) {tag:22s}: {dt * 1e3:.0f} ms per call -> {B / dt:.2f} expl/s ({B / dt / drop[B]:.2f}x the drop-in; fused attention "
                f"half: {eng._attn_fused(B * S)}; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB)")
    return dict(dropin_expl_per_s=drop, engine_expl_per_s=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--engine", action="store_true", help="the fused driver against the drop-in on one model, and the router kernels alone")
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}; layer H {H}, I {I}, {E} experts, top-{K}")
    if a.engine:
        result = dict(router_us=router_kernels(), **engine_bench())
        say("JSON " + json.dumps(result))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")
        return
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
