"""Seeded dense Qwen2 / Qwen3 models at shapes the fused decoder layer accepts (bf16, head_dim 64 / 128, H % 256 == 0), shared by the fixture
generator make_golden_qwen_fused.py and the tests.  Weights come from the seed (a checksum in the fixture pins them); biases and q / k norm
weights are randomised: HF initialises them to 0 and 1, which would hide a dropped bias or norm weight."""
import torch

# B x S = 24576 rows: the smallest row count at which every GEMM of these layers (the narrowest: nq d = H = 512 columns) fills the 190 output
# tiles lxt_amd.engine.fused_layer_ok asks for
B, S, VOCAB = 24, 1024, 512

CASES = dict(
    qwen2_d64=dict(family="qwen2", nq=8, nk=2, d=64, tie=False, seed=21),
    qwen2_d128=dict(family="qwen2", nq=4, nk=2, d=128, tie=True, seed=22),        # rope_cols = 768: a multiple of 256
    qwen3_d128=dict(family="qwen3", nq=4, nk=2, d=128, tie=False, seed=23),
)


def wsum(model):
    return float(sum(p.detach().double().abs().sum() for p in model.parameters()))


def build(case, attn="eager"):
    c = CASES[case]
    torch.manual_seed(c["seed"])
    kw = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=c["nq"], num_key_value_heads=c["nk"],
              vocab_size=VOCAB, max_position_embeddings=2048, attn_implementation=attn, tie_word_embeddings=c["tie"], use_sliding_window=False)
    if c["family"] == "qwen2":
        from transformers import Qwen2Config, Qwen2ForCausalLM
        model = Qwen2ForCausalLM(Qwen2Config(head_dim=c["d"], **kw))
    else:
        from transformers import Qwen3Config, Qwen3ForCausalLM
        model = Qwen3ForCausalLM(Qwen3Config(head_dim=c["d"], **kw))
    g = torch.Generator().manual_seed(c["seed"] + 100)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("proj.bias"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif name.endswith("norm.weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
    return model.eval()


def prompts(case):
    return torch.randint(0, VOCAB, (B, S), generator=torch.Generator().manual_seed(CASES[case]["seed"] + 200))


def to_bf16_rotary_fp32(model):
    """the model in bf16 with the rotary frequencies kept fp32 (as a checkpoint loaded in bf16 has them)"""
    for p in model.parameters():
        p.requires_grad_(False)
    inv = model.model.rotary_emb.inv_freq.detach().clone()
    model = model.to(torch.bfloat16)
    model.model.rotary_emb.inv_freq = inv.to(model.model.rotary_emb.inv_freq.device)
    return model
