"""CPU: the dense Qwen surface that needs no device -- the new C entry points are declared and exported, their host-side predicates answer,
QwenLRP.config_from_hf accepts the fixture models and refuses what the driver does not implement, the Llama driver keeps refusing Qwen."""
import ctypes
import re

import pytest
import torch

import lxt_amd._lib as L
from tests.golden import qwen_models as qm

BF16 = 1
NEW = ("lrp_gemm_nt_rs_bias", "lrp_gemm_nt_rs_bias_rope_ok", "lrp_gemm_nt_rs_bias_rope")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)
    return {m.group(2): m.group(3) for m in re.finditer(r"\b(int64_t|int|const char\*)\s+(lrp_\w+)\s*\(([^)]*)\)\s*;", src)}


def test_new_entry_points_declared_exported_and_counted():
    decl = _declared()
    assert len(decl) == 89 and L.lib.lrp_version() == 8
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in decl and hasattr(raw, name)
    # same argument lists as the un-biased neighbours plus `const void* bias`
    n = lambda s: len([a for a in s.split(",") if a.strip()])      # noqa: E731
    assert n(decl["lrp_gemm_nt_rs_bias"]) == n(decl["lrp_gemm_nt_rs"]) + 1 and "bias" in decl["lrp_gemm_nt_rs_bias"]
    assert n(decl["lrp_gemm_nt_rs_bias_rope"]) == n(decl["lrp_gemm_nt_rs_rope"]) + 1 and "bias" in decl["lrp_gemm_nt_rs_bias_rope"]
    assert n(decl["lrp_gemm_nt_rs_bias_rope_ok"]) == n(decl["lrp_gemm_nt_rs_rope_ok"])
    readme = open(L.HEADER_PATH.replace("include/lrp_hip.h", "README.md")).read()
    assert "89 entry points" in readme


def test_bias_rope_predicate_and_argument_checks():
    lib = L.lib
    assert lib.lrp_gemm_nt_rs_bias_rope_ok(8192, 6144, 4096, 4096, 4224, 6144, 2048, 5120, 128, BF16) == 1
    assert lib.lrp_gemm_nt_rs_bias_rope_ok(24576, 1024, 512, 512, 512, 1024, 1024, 768, 128, BF16) == 1          # the d = 128 fixture layers
    assert lib.lrp_gemm_nt_rs_bias_rope_ok(8192, 6144, 4096, 4096, 4224, 6144, 2048, 5120, 64, BF16) == 0
    # odd nq + nk at d = 128 (rope_cols % 256 == 128): the tile that holds the last k head holds the first v head -- refused here; the
    # un-biased predicate takes the shape, and rightly: the kernel decides "rotate" per wave = per head (test_gemm_nt_rs_rope_odd_head_count)
    assert lib.lrp_gemm_nt_rs_bias_rope_ok(8192, 4352, 4096, 4096, 4224, 4352, 2048, 4224, 128, BF16) == 0
    assert lib.lrp_gemm_nt_rs_rope_ok(8192, 4352, 4096, 4096, 4224, 4352, 2048, 4224, 128, BF16) == 1
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    assert lib.lrp_gemm_nt_rs_bias(None, None, None, None, None, 256, 256, 128, 128, 128, 256, BF16, None) == -1          # LRP_EINVAL
    assert lib.lrp_gemm_nt_rs_bias_rope(None, None, None, None, None, None, None, 256, 256, 128, 128, 128, 256, 256, 256, 128, BF16, None) == -1
    # shape refused before anything is touched (a 4-tile problem is not the ping-pong kernel's)
    eshape = lib.lrp_gemm_nt_rs(a, a, a, a, 512, 512, 128, 128, 128, 512, BF16, None)
    assert eshape < 0 and lib.lrp_gemm_nt_rs_bias(a, a, a, a, a, 512, 512, 128, 128, 128, 512, BF16, None) == eshape
    assert lib.lrp_gemm_nt_rs_bias_rope(a, a, a, a, a, a, a, 8192, 4352, 4096, 4096, 4224, 4352, 2048, 4224, 128, BF16, None) == eshape


@pytest.mark.parametrize("case", list(qm.CASES))
def test_qwen_config_accepts_the_fixture_models(case):
    import lxt_amd.engine as E
    import lxt_amd.engine_qwen as Q
    c = qm.CASES[case]
    model = qm.build(case)
    cfg, W = Q.weights_from_hf(model)
    assert (cfg["n_heads"], cfg["n_kv"], cfg["head_dim"], cfg["hidden"], cfg["inter"]) == (c["nq"], c["nk"], c["d"], 512, 1024)
    assert cfg["qkv_bias"] == (c["family"] == "qwen2") and cfg["qk_norm"] == (c["family"] == "qwen3") and cfg["tied"] == c["tie"]
    assert ("lm_head" in W) != c["tie"] and len(W["layers"]) == 3
    assert all(("bq" in Lw) == cfg["qkv_bias"] and ("qn" in Lw) == cfg["qk_norm"] for Lw in W["layers"])
    top, layer = Q.QwenLRP.flat_layout(cfg, torch.bfloat16)
    assert ("lm_head" in top) != c["tie"] and ("bqkv" in layer) == cfg["qkv_bias"] and ("qn" in layer) == cfg["qk_norm"]
    flat, _, layers = E.pack_flat(top, layer, 3, torch.bfloat16, "meta")
    if cfg["qkv_bias"]:
        assert layers[0]["bqkv"].shape == ((c["nq"] + 2 * c["nk"]) * c["d"],) and layers[0]["bqkv"].storage_offset() % 8 == 0      # 16-byte aligned
    with pytest.raises(NotImplementedError):
        E.config_from_hf(model.config)                     # the Llama driver keeps refusing the family
    # the fused layer applies at the fixture's row count
    pt = E.fused_layout(512, 1024, c["nq"], c["nk"], c["d"], torch.bfloat16)
    Wm = {k: v for k, v in layers[0].items()}
    assert pt["Wqkv"] == Wm["wqkv"].stride(0)
    assert E.fused_layer_ok(qm.B * qm.S, Wm, (c["nq"], c["nk"], c["d"], 1e-6, "silu", c["d"] ** -0.5), torch.bfloat16, {}).full


def test_qwen_config_refuses_what_the_driver_does_not_implement():
    from transformers import LlamaConfig, Qwen2Config, Qwen3Config
    import lxt_amd.engine as E
    import lxt_amd.engine_qwen as Q
    kw = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, vocab_size=512)
    assert Q.config_from_hf(Qwen2Config(**kw))["qkv_bias"] and Q.config_from_hf(Qwen3Config(head_dim=64, **kw))["qk_norm"]
    bad = [Qwen2Config(use_sliding_window=True, sliding_window=128, max_window_layers=1, **kw),
           Qwen3Config(layer_types=["full_attention", "sliding_attention"], **kw),
           Qwen2Config(mlp_bias=True, **kw),
           Qwen3Config(attention_bias=True, **kw),
           Qwen2Config(rope_parameters=dict(rope_type="dynamic", factor=2.0, rope_theta=10000.0), **kw),
           LlamaConfig(**kw)]
    for c in bad:
        with pytest.raises(NotImplementedError):
            Q.config_from_hf(c)
    with pytest.raises(NotImplementedError, match="z = x W\\^T \\+ b"):
        Q.QwenLRP.set_mode(object.__new__(Q.QwenLRP), "explicit")
    with pytest.raises(NotImplementedError):
        E.config_from_hf(Qwen2Config(**kw))


def test_fixtures_pin_the_models():
    from tests.util import load
    for case in qm.CASES:
        fx = load(f"qwen_fused_{case}.npz")
        assert abs(qm.wsum(qm.build(case)) - float(fx["wsum"])) < 1e-6 * float(fx["wsum"]), "weights did not reproduce"
        assert fx["ids"].shape == (qm.B, qm.S) and fx["R_tok_fp64"].dtype.name == "float64" and float(fx["gap"].max()) < 1e-4
        assert (fx["ids"] == qm.prompts(case).numpy()).all()
        assert fx["margin"].shape == (qm.B,) and (fx["margin"] >= 0).all()
