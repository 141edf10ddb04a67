"""Seeded Qwen3-MoE model of the bf16 engine test (tests/test_qwen_moe_engine_gpu.py): H 256, 4 / 2 heads of d = 64, moe_intermediate_size 128,
8 experts, top-2 with renorm, layers sparse / dense / sparse.  Routing has to survive bf16: with i.i.d. weights the smallest 2nd-to-3rd
probability gap over 2 x 128 tokens and two routers is ~1e-6 while bf16 moves probabilities by ~0.1, so no seed can separate rounding from a
flipped expert.  The routing is therefore PLANTED: token v carries A at hidden dim a(v) and 0.6 A at dim b(v) (a, b < 8, seeded, distinct),
router e reads hidden dim e alone and the norms leave those eight dims unweighted -- every token's two experts stand clear of each other and
of the other six in every layer, by margins the test asserts against the measured bf16 probability error (seed 3: 0.085 and 0.098
against 0.0026).  Everything else is seeded noise, initialised explicitly as in moe_models.py."""
import torch

SEED, S, B = 3, 128, 2
PLANT, SECOND, ROUTER_GAIN, NOISE = 30.0, 0.6, 0.12, 0.5


def build(attn="eager", seed=SEED):
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(hidden_size=256, intermediate_size=512, moe_intermediate_size=128, num_attention_heads=4, num_key_value_heads=2,
                         head_dim=64, vocab_size=256, max_position_embeddings=512, attn_implementation=attn, tie_word_embeddings=False,
                         use_sliding_window=False, decoder_sparse_step=1, num_experts=8, num_experts_per_tok=2, norm_topk_prob=True,
                         num_hidden_layers=3, mlp_only_layers=[1])
    torch.manual_seed(seed)
    model = Qwen3MoeForCausalLM(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1000)
    E = cfg.num_experts
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("mlp.gate.weight"):
                p.zero_()
                p[:, :E] = ROUTER_GAIN * torch.eye(E)
            elif "experts." in name:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
            elif "norm" in name:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
                if p.shape[0] == cfg.hidden_size:
                    p[:E] = 1.0          # (the routers read the planted dims as planted: a norm weight of 1.19 against 0.74 undoes a 0.6 ratio)
            elif name.endswith("embed_tokens.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * NOISE)
                pick = torch.rand(p.shape[0], E, generator=g).argsort(1)[:, :2]
                p[:, :E] = 0.0
                p.scatter_(1, pick, torch.tensor([PLANT, SECOND * PLANT]).expand(p.shape[0], 2))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return model


def inputs(seed=SEED):
    return torch.randint(0, 256, (B, S), generator=torch.Generator().manual_seed(seed + 7))


def wsum(model):
    return float(sum(p.detach().double().abs().sum() for p in model.parameters()))


def router_probs(model, ids):
    """fp64 softmax of every router's logits in one plain HF forward -> [n_sparse_layers, B S, E]"""
    out = []
    hooks = [m.register_forward_hook(lambda mod, i, o: out.append(torch.softmax(o[0].detach().double(), -1)))
             for m in model.modules() if type(m).__name__ == "Qwen3MoeTopKRouter"]
    with torch.no_grad():
        model(input_ids=ids, use_cache=False)
    for h in hooks:
        h.remove()
    return torch.stack(out)


def margin_and_bf16_shift(seed=SEED):
    """-> (the smallest 2nd-to-3rd and 1st-to-2nd probability gaps of the fp32 model over every token and router -- the second keeps the
    slot ORDER --, the largest |p_bf16 - p_fp32|), on the CPU"""
    ids, model = inputs(seed), build(seed=seed)
    p32 = router_probs(model, ids)
    srt = p32.sort(-1, descending=True).values
    pb = router_probs(model.to(torch.bfloat16), ids)
    return float((srt[..., 1] - srt[..., 2]).min()), float((srt[..., 0] - srt[..., 1]).min()), float((pb - p32).abs().max())
