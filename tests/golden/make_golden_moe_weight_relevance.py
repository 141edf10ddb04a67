#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): the per-weight relevance `weight * weight.grad` of a Qwen3-MoE
under `lxt.efficient.monkey_patch(modeling_qwen3_moe)` (ref lxt/efficient/models/qwen3_moe.py:14-44), run on the CPU in fp64 with the protocol
of make_golden_qwen3_moe_experts.py and the same inputs(case): eager attention, the arg-max logit of the last position seeded with 1.
    LXT_REFERENCE=<path of the reference> python tests/golden/make_golden_moe_weight_relevance.py
Asserts idx / logit equal those of the committed qwen3_moe_experts_{case}.npz.  Rows in HF order (qkv = q_proj | k_proj | v_proj rows,
gate_up = experts.gate_up_proj's [gate | up] rows).  Every file stays under 1 MiB (asserted), so the fixture is split:
  moe_weight_relevance_tiny.npz            layers (all), moe (the sparse ones), idx, logit, counts [L', E] (plan rows per expert),
                                           gate_up_total / down_total [L', E] fp64, router [L', E, H], qkv [L, ., H], o [L, H, .] fp32
  moe_weight_relevance_tiny_gate_up_l{l}_e{a}.npz   gate_up [4, 2 I, H] fp32 of experts a .. a + 3 of sparse layer l
  moe_weight_relevance_tiny_down_l{l}.npz           down [E, H, I] fp32 of sparse layer l
  moe_weight_relevance_fanout.npz          as tiny's first file without qkv / o / router, plus gate_up_rowsum [L', E, 2 I] and
                                           down_rowsum [L', E, H] fp32 (sums over the matrix's columns, formed in fp64), chosen [L', 3] (an expert
                                           with 0 rows, one with exactly 1 row, the most loaded) and chosen_rows [L', 3]
  moe_weight_relevance_fanout_dense.npz    router, qkv, o as above
  moe_weight_relevance_fanout_l{l}.npz     gate_up [3, 2 I, H] and down [3, H, I] fp32 of the chosen experts of sparse layer l
(fanout's full expert matrices are 24 MiB per layer.)"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
warnings.simplefilter("ignore")

from tests.golden.moe_models import build_qwen3_moe, inputs, model_case  # noqa: E402

MAX_BYTES = 1 << 20
PROTOCOL = ("lxt.efficient.monkey_patch(modeling_qwen3_moe), fp64, CPU, eager attention; arg-max logit of the last position seeded 1; "
            "p * p.grad of q/k/v/o_proj, mlp.gate, mlp.experts.gate_up_proj and mlp.experts.down_proj")


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  {name}: {size} bytes")
    assert size < MAX_BYTES, (name, size)


def f32(t):
    return t.to(torch.float32).numpy()


def explain(model, ids):
    """-> (idx, logit, per layer {name: p * p.grad fp64}, per sparse layer the selected experts [S, k])"""
    for p_ in model.parameters():
        p_.requires_grad_(True)
    model.zero_grad(set_to_none=True)
    sel, hooks = {}, []
    for li, L in enumerate(model.model.layers):
        if hasattr(L.mlp, "gate") and hasattr(L.mlp, "experts"):
            hooks.append(L.mlp.gate.register_forward_hook(lambda mod, inp, out, li=li: sel.__setitem__(li, out[2].detach())))
    e = model.get_input_embeddings()(ids).detach().requires_grad_()
    last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
    idx = int(last.argmax())
    last[idx].backward()
    for h in hooks:
        h.remove()
    rel = lambda p_: (p_ * p_.grad).detach()          # noqa: E731
    layers = []
    for li, L in enumerate(model.model.layers):
        a = L.self_attn
        d = dict(qkv=torch.cat([rel(a.q_proj.weight), rel(a.k_proj.weight), rel(a.v_proj.weight)]), o=rel(a.o_proj.weight))
        if li in sel:
            ex = L.mlp.experts
            assert ex.gate_up_proj.grad is not None and ex.down_proj.grad is not None and L.mlp.gate.weight.grad is not None
            d.update(router=rel(L.mlp.gate.weight), gate_up=rel(ex.gate_up_proj), down=rel(ex.down_proj))
        layers.append(d)
    return idx, float(last[idx]), layers, sel


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    monkey_patch(modeling_qwen3_moe)
    for case in ("tiny", "fanout"):
        ids, am, _ = inputs(case)
        assert am is None and ids.shape[0] == 1
        model = build_qwen3_moe(model_case(case)).double()
        E = model.config.num_experts
        idx, logit, layers, sel = explain(model, ids)
        old = np.load(os.path.join(HERE, f"qwen3_moe_experts_{case}.npz"))
        assert [idx] == old["idx"].tolist() and abs(logit - float(old["logit"][0])) <= 1e-12 * abs(logit), (idx, logit, old["idx"], old["logit"])
        moe = sorted(sel)
        for j, li in enumerate(moe):
            assert np.array_equal(sel[li].numpy(), old["expert_index"][li, 0])
        counts = torch.stack([torch.bincount(sel[li].flatten(), minlength=E) for li in moe])
        gu = torch.stack([layers[li]["gate_up"] for li in moe])              # [L', E, 2 I, H] fp64
        dn = torch.stack([layers[li]["down"] for li in moe])                 # [L', E, H, I]
        gu_tot, dn_tot = gu.sum((2, 3)), dn.sum((2, 3))
        R_expert = torch.from_numpy(old["R_expert"])[moe, 0]
        scale = float(R_expert.abs().max())
        dev = max(float((gu_tot - R_expert).abs().max()), float((dn_tot - R_expert).abs().max())) / scale
        print(f"[{case}] idx={idx} sparse layers {moe} rows per expert min {int(counts.min())} max {int(counts.max())}; per-expert totals vs "
              f"R_expert: gate_up {float((gu_tot - R_expert).abs().max()) / scale:.1e} down {float((dn_tot - R_expert).abs().max()) / scale:.1e}")
        assert dev <= 1e-9, dev
        assert bool((gu[counts == 0] == 0).all()) and bool((dn[counts == 0] == 0).all())
        head = dict(layers=np.arange(len(layers)), moe=np.asarray(moe), idx=np.asarray([idx]), logit=np.asarray([logit]), counts=counts.numpy(),
                    gate_up_total=gu_tot.numpy(), down_total=dn_tot.numpy(), protocol=np.array(PROTOCOL))
        dense = dict(router=f32(torch.stack([layers[li]["router"] for li in moe])), qkv=f32(torch.stack([d["qkv"] for d in layers])),
                     o=f32(torch.stack([d["o"] for d in layers])))
        if case == "tiny":
            save("moe_weight_relevance_tiny.npz", **head, **dense)
            for j, li in enumerate(moe):
                for a in range(0, E, 4):
                    save(f"moe_weight_relevance_tiny_gate_up_l{li}_e{a}.npz", gate_up=f32(gu[j, a:a + 4]))
                save(f"moe_weight_relevance_tiny_down_l{li}.npz", down=f32(dn[j]))
            continue
        chosen = []
        for j in range(len(moe)):
            c = counts[j]
            zero, one = torch.nonzero(c == 0).flatten(), torch.nonzero(c == 1).flatten()
            assert zero.numel() and one.numel(), "the case must leave an expert without a row and one with exactly one"
            chosen.append([int(zero[0]), int(one[0]), int(c.argmax())])
        chosen = torch.tensor(chosen)
        rows = torch.gather(counts, 1, chosen)
        print(f"  chosen experts {chosen.tolist()} with rows {rows.tolist()}")
        save("moe_weight_relevance_fanout.npz", **head, gate_up_rowsum=f32(gu.sum(3)), down_rowsum=f32(dn.sum(3)), chosen=chosen.numpy(),
             chosen_rows=rows.numpy())
        save("moe_weight_relevance_fanout_dense.npz", **dense)
        for j, li in enumerate(moe):
            save(f"moe_weight_relevance_fanout_l{li}.npz", gate_up=f32(gu[j, chosen[j]]), down=f32(dn[j, chosen[j]]))


if __name__ == "__main__":
    main(*sys.argv[1:2])
