"""CPU: the router surface that needs no device -- the three entry points of csrc/moe_router.hip are declared in the header lrp_hip.h includes,
exported and bound; they refuse bad shapes and pitches before any launch; ops.* check their arguments; Qwen3MoeLRP's config_from_hf accepts
the fixture models and refuses what the driver does not implement; the expert-relevance fixtures satisfy their identities."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lxt_amd._lib as L
from tests.golden.moe_models import CASES
from tests.util import load

F32, BF16 = 0, 1
EINVAL, EALIGN, ESHAPE = -1, -2, -3
NEW = ("lrp_moe_router_fwd", "lrp_moe_router_bwd", "lrp_moe_expert_relevance")


def test_entry_points_declared_exported_and_bound():
    inc = os.path.join(os.path.dirname(L.HEADER_PATH), "lrp_hip_moe_router.h")
    assert '#include "lrp_hip_moe_router.h"' in open(L.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", open(inc).read(), flags=re.S)
    declared = re.findall(r"\bint\s+(lrp_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and name in L.DECLS and getattr(L.lib, name).argtypes is not None
    assert L.lib.lrp_version() == 8
    import lxt_amd.ops as ops
    assert all(callable(getattr(ops, n)) for n in ("moe_router_fwd", "moe_router_bwd", "moe_expert_relevance"))


def test_shape_and_alignment_are_refused_before_any_launch():
    """host memory only: every call below must return before it launches (a launch on it would be an error of its own)"""
    lib = L.lib
    buf = (ctypes.c_char * 256)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    for dt in (F32, BF16):
        # k > 16, k > E, E > 1024
        for E, k in ((64, 17), (8, 9), (1025, 8)):
            assert lib.lrp_moe_router_fwd(a, a, a, a, 4, E, k, E, 1, dt, None) == ESHAPE
            assert lib.lrp_moe_router_bwd(a, a, a, a, a, a, 4, E, k, E, E, 1, dt, None) == ESHAPE
            assert lib.lrp_moe_expert_relevance(a, a, a, a, 2, 2, k, E, dt, None) == ESHAPE
        assert lib.lrp_moe_router_fwd(a, a, a, a, 4, 8, 2, 6, 1, dt, None) == ESHAPE                   # pitch < E
        assert lib.lrp_moe_router_fwd(None, a, a, a, 4, 8, 2, 8, 1, dt, None) == EINVAL
        assert lib.lrp_moe_router_bwd(a, a, a, a, None, a, 4, 8, 2, 8, 8, 1, dt, None) == EINVAL
        assert lib.lrp_moe_expert_relevance(a, a, a, None, 2, 2, 2, 8, dt, None) == EINVAL
        assert lib.lrp_moe_router_fwd(a, a, a, a, 4, 8, 2, 8, 1, 7, None) == EINVAL                     # unknown dtype
    # an odd pitch (bf16: rows off the 4-byte grid), for the logits and for the gradient; a base off the grid
    assert lib.lrp_moe_router_fwd(a, a, a, a, 4, 8, 2, 9, 1, BF16, None) == EALIGN
    assert lib.lrp_moe_router_bwd(a, a, a, a, a, a, 4, 8, 2, 9, 8, 1, BF16, None) == EALIGN
    assert lib.lrp_moe_router_bwd(a, a, a, a, a, a, 4, 8, 2, 8, 9, 1, BF16, None) == EALIGN
    assert lib.lrp_moe_router_fwd(a + 2, a, a, a, 4, 8, 2, 8, 1, F32, None) == EALIGN
    assert lib.lrp_moe_router_fwd(a, a + 4, a, a, 4, 8, 2, 8, 1, F32, None) == EALIGN                   # int64 idx off 8 bytes
    assert lib.lrp_moe_expert_relevance(a + 4, a, a, a, 2, 2, 2, 8, F32, None) == EALIGN


def test_ops_argument_checks_raise_value_error():
    import lxt_amd.ops as ops
    x = torch.zeros(4, 8)
    idx, w, lse = torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 2), torch.zeros(4)
    with pytest.raises(ValueError):
        ops.moe_router_fwd(torch.zeros(4, 8, 2), 2, True)                       # not [T, E]
    with pytest.raises(ValueError):
        ops.moe_router_fwd(torch.zeros(8, 4).t(), 2, True)                      # column stride
    with pytest.raises(ValueError):
        ops.moe_router_fwd(x.half(), 2, True)                                   # dtype
    with pytest.raises(ValueError):
        ops.moe_router_fwd(x, 9, True)                                          # k > E
    with pytest.raises(ValueError):
        ops.moe_router_fwd(torch.zeros(2, 64), 17, True)                        # k > 16
    with pytest.raises(ValueError):
        ops.moe_router_fwd(torch.zeros(2, 1026), 2, True)                       # E > 1024
    with pytest.raises(ValueError):
        ops.moe_router_bwd(x, lse, idx.int(), w, w, True)                       # idx dtype
    with pytest.raises(ValueError):
        ops.moe_router_bwd(x, lse, idx, w.bfloat16(), w, True)                  # w dtype
    with pytest.raises(ValueError):
        ops.moe_router_bwd(x, lse, idx, w, torch.zeros(4, 3), True)             # G_w shape
    with pytest.raises(ValueError):
        ops.moe_router_bwd(x, lse.double(), idx, w, w, True)                    # lse dtype
    with pytest.raises(ValueError):
        ops.moe_router_bwd(x, lse, idx, w, w, True, out=torch.zeros(4, 9))      # out shape
    with pytest.raises(ValueError):
        ops.moe_expert_relevance(idx, w, w, 3, 2, 8)                            # B S != T
    with pytest.raises(ValueError):
        ops.moe_expert_relevance(idx, w, w[:, :1], 2, 2, 8)
    with pytest.raises(ValueError):
        ops.moe_expert_relevance(idx, w, w, 2, 2, 8, out=torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.moe_router_fwd(x, 2, True)                                          # well-formed, but on the host: no CPU fallback


def _hf_config(**kw):
    from transformers import Qwen3MoeConfig
    base = dict(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_attention_heads=4, num_key_value_heads=2, head_dim=32,
                vocab_size=256, num_hidden_layers=3, num_experts=8, num_experts_per_tok=2, use_sliding_window=False, decoder_sparse_step=1,
                mlp_only_layers=[1], norm_topk_prob=True)
    base.update(kw)
    return Qwen3MoeConfig(**base)


def test_config_from_hf_accepts_the_fixture_models():
    import lxt_amd.engine_qwen_moe as QM
    for case, c in CASES.items():
        c = {k: v for k, v in c.items() if k not in ("seed", "router_std")}
        cfg = QM.config_from_hf(_hf_config(**c))
        assert cfg["qk_norm"] and not cfg["qkv_bias"] and cfg["n_experts"] == c["num_experts"] and cfg["top_k"] == c["num_experts_per_tok"]
        assert cfg["norm_topk"] == c["norm_topk_prob"] and cfg["moe_inter"] == 128 and cfg["inter"] == 256
        assert list(cfg["moe_layers"]) == [li not in c["mlp_only_layers"] for li in range(c["num_hidden_layers"])]
    assert list(QM.config_from_hf(_hf_config(mlp_only_layers=[], decoder_sparse_step=2, num_hidden_layers=4))["moe_layers"]) == \
        [False, True, False, True]


@pytest.mark.parametrize("kw,word", [
    (dict(use_sliding_window=True), "sliding-window"),
    (dict(attention_bias=True), "bias"),
    (dict(hidden_act="relu"), "activation"),
    (dict(hidden_size=192, head_dim=48), "multiples of 128"),
    (dict(moe_intermediate_size=96), "multiples of 128"),
    (dict(num_experts=1025), "experts"),
    (dict(num_experts=64, num_experts_per_tok=17), "experts"),
])
def test_config_from_hf_refusals(kw, word):
    import lxt_amd.engine_qwen_moe as QM
    with pytest.raises(NotImplementedError, match=word):
        QM.config_from_hf(_hf_config(**kw))


def test_other_families_are_refused_both_ways():
    import lxt_amd.engine_qwen as Q
    import lxt_amd.engine_qwen_moe as QM
    from transformers import Qwen3Config
    with pytest.raises(NotImplementedError, match="Qwen3-MoE"):
        QM.config_from_hf(Qwen3Config(hidden_size=128, intermediate_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=1))
    with pytest.raises(NotImplementedError):
        Q.config_from_hf(_hf_config())


@pytest.mark.parametrize("case", ["tiny", "fanout", "padded"])
def test_expert_fixtures_satisfy_their_identities(case):
    fx, old = load(f"qwen3_moe_experts_{case}.npz"), load(f"hf_qwen3_moe_{case}.npz")
    R, index, blk = fx["R_expert"], fx["expert_index"], fx["R_block"]
    L_, B, E = R.shape
    c = CASES["tiny" if case == "padded" else case]
    assert index.shape == (L_, B, old["ids"].shape[1], c["num_experts_per_tok"]) and E == c["num_experts"]
    assert float(np.abs(R.sum(-1) - 0.5 * blk).max()) <= 1e-12 * float(np.abs(R).max())
    assert float(fx["margin"]) >= 1e-4
    valid = old["mask"].astype(bool)
    for li in range(L_):
        if li in c["mlp_only_layers"]:
            assert not R[li].any() and (index[li] == -1).all() and not blk[li].any()
        else:
            assert R[li].any()
            for b in range(B):
                assert (index[li, b][valid[b]] >= 0).all() and (index[li, b][~valid[b]] == -1).all()
                # an expert no token of the prompt was routed to carries exactly nothing
                hit = np.zeros(E, dtype=bool)
                hit[index[li, b][valid[b]].ravel()] = True
                assert not R[li, b][~hit].any()
    # the same run as the drop-in's fixture: same explained token, same token relevance
    assert fx["idx"].tolist() == old["idx"].tolist()
    assert float(np.abs(fx["R_tok"] - old["R_tok_fp64"]).max()) <= 1e-5 * float(np.abs(old["R_tok_fp64"]).max())
