"""Seeded Gemma-3 text model at head dim 256 for the read-out fixtures (make_golden_gemma3_readouts.py) and their tests: the smallest decoder
that reaches the d = 256 attention kernels and the bf16 map kernel lrp_attn_relmap_d256."""
import torch

D256_S, D256_ISEED = 136, 41           # tiles of 64 / 64 / 8 keys: a ragged last tile and, with window 48, a tile wholly outside the window


def build_gemma3_d256(seed=23, attn="eager"):
    """H 256, I 512, layers sliding / sliding / full with window 48, 4 query + 2 kv heads of d = 256, query_pre_attn_scalar 256, vocab 256;
    non-trivial norm weights as hf_models.build_gemma3_4bdims sets them (HF initialises Gemma's (1 + w) norm weights to zero)"""
    from transformers import Gemma3TextConfig, Gemma3ForCausalLM
    torch.manual_seed(seed)
    cfg = Gemma3TextConfig(vocab_size=256, hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=256, sliding_window=48, max_position_embeddings=512,
                           layer_types=["sliding_attention", "sliding_attention", "full_attention"], query_pre_attn_scalar=256,
                           attn_implementation=attn, tie_word_embeddings=False)
    m = Gemma3ForCausalLM(cfg).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for n_, p_ in m.named_parameters():
            if "norm" in n_:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.1)
    return m


def d256_ids():
    return torch.randint(0, 256, (D256_S,), generator=torch.Generator().manual_seed(D256_ISEED))


def to_bf16_rotary_fp32(model):
    """the model in bf16 with the rotary frequencies kept fp32, as a checkpoint loaded in bf16 has them (`.to(bfloat16)` rounds the inv_freq
    buffers: README)"""
    rot = model.model.rotary_emb
    keep = {n: b.detach().clone() for n, b in rot.named_buffers()}
    model = model.to(torch.bfloat16)
    for n, b in keep.items():
        setattr(rot, n, b)
    return model
