"""Seeded Qwen3-MoE builders for the MoE fixtures (tests/golden/make_golden_qwen3_moe.py) and tests/moe_worker.py.  Every parameter is
initialised explicitly from the seed: the router's __init__ leaves zeros (all-tie routing) and the experts' tensors are torch.empty."""
import torch

CASES = {
    # tiny: 8 experts, top-2, renormalised top-k, one dense layer (mlp_only_layers)
    "tiny": dict(num_experts=8, num_experts_per_tok=2, norm_topk_prob=True, num_hidden_layers=3, mlp_only_layers=[1], seed=85, router_std=0.3),
    # real fan-out: 128 experts, top-8, no renorm; 48 tokens x 8 slots leave most experts with 0-3 rows
    "fanout": dict(num_experts=128, num_experts_per_tok=8, norm_topk_prob=False, num_hidden_layers=2, mlp_only_layers=[], seed=51,
                   router_std=0.3),
}
SEQ = {"tiny": 64, "fanout": 48}


def build_qwen3_moe(case="tiny", attn="eager"):
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    c = dict(CASES[case])
    seed, router_std = c.pop("seed"), c.pop("router_std")
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_attention_heads=4, num_key_value_heads=2,
                         head_dim=32, vocab_size=256, max_position_embeddings=512, attn_implementation=attn, tie_word_embeddings=False,
                         use_sliding_window=False, decoder_sparse_step=1, **c)
    torch.manual_seed(seed)
    model = Qwen3MoeForCausalLM(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("mlp.gate.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * router_std)
            elif "experts." in name:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
            elif "norm" in name:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return model


def wsum(model):
    return float(sum(p.detach().double().abs().sum() for p in model.parameters()))


def inputs(case):
    """-> (ids [B, S], attention_mask [B, S] or None, last position per row)"""
    g = torch.Generator().manual_seed(4321)
    if case == "padded":
        S, lens = 64, [64, 41]
        ids = torch.randint(1, 256, (2, S), generator=g)
        am = torch.zeros(2, S, dtype=torch.long)
        for b, n in enumerate(lens):
            am[b, S - n:] = 1
        return ids, am, torch.full((2,), S - 1)
    S = SEQ[case]
    return torch.randint(0, 256, (1, S), generator=g), None, torch.tensor([S - 1])


def model_case(case):
    return "tiny" if case == "padded" else case
