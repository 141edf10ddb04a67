"""CPU: the per-head attention relevance read-out (lrp_headdot, LlamaLRP.explain(heads=...)) -- its C ABI is declared and exported, rejects
bad calls before any launch, the engine's request check refuses unknown names before a kernel of the model runs, and the two fixtures of
the real reference (tests/golden/make_golden_heads.py) satisfy the identities their generator asserted."""
import ctypes

import numpy as np
import pytest
import torch

from tests.util import load


def test_headdot_symbol_declared_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    # (x, g, cos, sin, out, M, B, S, nh, rep, d, ldx, ldg, scale, dtype, stream)
    assert decls["lrp_headdot"] == ("int", ["void*", "void*", "float*", "float*", "float*", "int", "int", "int", "int", "int", "int",
                                            "int64_t", "int64_t", "float", "int", "void*"])
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "lrp_headdot")
    from lxt_amd import ops
    assert callable(ops.headdot)


def test_headdot_argument_validation_without_gpu():
    import lxt_amd._lib as L
    lib, BF16, F32 = L.lib, L.BF16, L.F32
    A = 1 << 12                                   # an aligned fake device address: every call below is rejected before a launch
    # 2 prompts x 128 rows, 8 query heads over 2 kv heads of d = 32: x [256, 64] (rep = 4), g [256, 256]
    ok = dict(x=A, g=A, cos=None, sin=None, out=A, M=256, B=2, S=128, nh=8, rep=4, d=32, ldx=64, ldg=256, scale=1.0, dtype=BF16, stream=None)
    call = lambda **kw: lib.lrp_headdot(*{**ok, **kw}.values())      # noqa: E731
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    for kw in (dict(x=None), dict(g=None), dict(out=None), dict(dtype=7), dict(cos=A), dict(sin=A)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(M=255), dict(B=0, M=0), dict(S=0, M=0), dict(nh=0), dict(rep=0), dict(d=0), dict(nh=8, rep=3), dict(d=264, ldx=528, ldg=2112),
               dict(cos=A, sin=A, d=33, ldx=72, ldg=264), dict(ldx=56), dict(ldg=248)):
        assert call(**kw) == ESHAPE, kw
    for kw in (dict(x=A + 2), dict(g=A + 8), dict(cos=A + 4, sin=A), dict(cos=A, sin=A + 8), dict(ldx=68), dict(ldg=260),
               dict(d=36, ldx=72, ldg=288), dict(dtype=F32, d=6, ldx=12, ldg=48), dict(out=A + 2), dict(dtype=F32, ldx=66)):
        assert call(**kw) == EALIGN, kw
    # d = 36 is a whole number of 16-byte vectors in fp32, not in bf16
    assert call(d=36, ldx=72, ldg=288) == EALIGN and call(d=260, ldx=520, ldg=2080, dtype=F32) == ESHAPE


def test_headdot_binding_rejects_cpu_tensors():
    from lxt_amd import ops
    x, g = torch.randn(8, 16), torch.randn(8, 32)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.headdot(x, g, 2, 4, 4, 2, 8)
    with pytest.raises(ValueError):
        ops.headdot(x, torch.randn(8, 16), 2, 4, 4, 2, 8)              # g is not [B S, nh d]


def test_head_request_names():
    from lxt_amd.engine import head_request, latent_request, HEADS, LATENT
    bf, f4 = torch.bfloat16, torch.float32
    assert HEADS == ("out", "q", "k", "v") and frozenset(LATENT) == {"trace", "resid", "mlp"}
    assert head_request(None, 128, bf) == frozenset() and head_request([], 128, bf) == frozenset()
    assert head_request("out", 128, bf) == frozenset({"out"})                  # one name as a string, not its letters
    assert head_request(["q", "q", "k"], 128, bf) == frozenset({"q", "k"})
    assert head_request(HEADS, 32, f4) == frozenset(HEADS)
    for bad in (["heads"], ("out", "R_head"), "o", 3, ["trace"]):
        with pytest.raises(ValueError):
            head_request(bad, 128, bf)
    # a head dim the kernel cannot read: rows of 16-byte vectors, d <= 256
    for d, dt in ((36, bf), (6, f4), (512, bf), (0, bf), (None, bf)):
        with pytest.raises(ValueError):
            head_request(["out"], d, dt)
    assert head_request(None, 36, bf) == frozenset() and head_request(["v"], 36, f4) == frozenset({"v"})
    # the read-outs are a keyword of their own, not latent names
    for bad in ("heads", ["attention_heads"], ["out"]):
        with pytest.raises(ValueError):
            latent_request(bad, 4096, 14336, bf)


def test_explain_rejects_heads_before_anything_runs():
    """LlamaLRP.explain checks heads first: a stub without weights or a device raises the ValueError, not an error of a missing kernel input"""
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_qwen import QwenLRP
    for cls in (LlamaLRP, QwenLRP):
        stub = cls.__new__(cls)
        stub.cfg, stub.dtype = dict(hidden=64, inter=128, vocab=32, head_dim=16), torch.bfloat16
        with pytest.raises(ValueError, match="unknown read-out"):
            stub.explain(torch.zeros(1, 4, dtype=torch.long), heads=["nope"])
        with pytest.raises(ValueError, match="iterable"):
            stub.explain(torch.zeros(1, 4, dtype=torch.long), heads=3)


@pytest.mark.parametrize("name,L,nq,nk,S", [("heads_llama.npz", 4, 8, 2, 128), ("heads_qwen3.npz", 3, 4, 2, 80)])
def test_fixture_identities(name, L, nq, nk, S):
    fx = load(name)
    for k in ("out", "q", "k", "v"):
        assert fx[k].shape == (L, nq, S) and fx[k].dtype == np.float64 and np.isfinite(fx[k]).all() and np.abs(fx[k]).max() > 0
    assert fx["k_kv"].shape == (L, nk, S) and fx["v_kv"].shape == (L, nk, S) and fx["ids"].shape == (S,)
    scale = np.abs(fx["out"]).max()
    # the group sums of the per-query-head maps are the kv-head-level relevance
    for a, b in (("k", "k_kv"), ("v", "v_kv")):
        assert np.abs(fx[a].reshape(L, nk, nq // nk, S).sum(2) - fx[b]).max() <= 1e-12 * scale
    # the uniform rule of the P V product: a head's value relevance is half of what it writes
    assert np.abs(fx["v"].sum(-1) - 0.5 * fx["out"].sum(-1)).max() <= 1e-12 * scale
    # above the top layer only the last position is live: its queries elsewhere carry nothing
    assert not fx["q"][-1, :, :-1].any() and np.abs(fx["q"][-1, :, -1]).max() > 0
