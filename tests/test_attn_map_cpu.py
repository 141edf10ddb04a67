"""CPU: the token-to-token attention relevance maps (lrp_attn_relmap, LlamaLRP.explain(attn_map=...)) -- the C ABI is declared and exported,
rejects bad calls before any launch, the engine's request check refuses bad requests before a kernel of the model runs, and the two
fixtures of the real reference (tests/golden/make_golden_attn_map.py) satisfy the identities their generator asserted."""
import ctypes

import numpy as np
import pytest
import torch

from tests.util import load


def test_attn_relmap_symbol_declared_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    # (q, k, v, g, lse, out, M, B, S, Hq, Hkv, d, h_lo, h_hi, ldq, ldk, ldv, ldg, scale, gscale, causal, row_lo, row_hi, dtype, stream)
    assert decls["lrp_attn_relmap"] == ("int", ["void*", "void*", "void*", "void*", "float*", "float*", "int", "int", "int", "int", "int", "int",
                                                "int", "int", "int64_t", "int64_t", "int64_t", "int64_t", "float", "float", "int", "int*", "int*",
                                                "int", "void*"])
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "lrp_attn_relmap")
    from lxt_amd import ops
    assert callable(ops.attn_relmap)


def test_attn_relmap_argument_validation_without_gpu():
    import lxt_amd._lib as L
    lib, BF16, F32 = L.lib, L.BF16, L.F32
    A = 1 << 12                                   # an aligned fake device address: every call below is rejected before a launch
    # 2 prompts x 128 rows, 8 query heads over 2 kv heads of d = 64: q, g [256, 512], k, v [256, 128]
    ok = dict(q=A, k=A, v=A, g=A, lse=A, out=A, M=256, B=2, S=128, Hq=8, Hkv=2, d=64, h_lo=0, h_hi=8, ldq=512, ldk=128, ldv=128, ldg=512,
              scale=0.125, gscale=1.0, causal=1, row_lo=None, row_hi=None, dtype=BF16, stream=None)
    call = lambda **kw: lib.lrp_attn_relmap(*{**ok, **kw}.values())      # noqa: E731
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(g=None), dict(lse=None), dict(out=None), dict(dtype=7)):
        assert call(**kw) == EINVAL, kw
    f32_32 = dict(dtype=F32, d=32, ldq=256, ldk=64, ldv=64, ldg=256)
    for kw in (dict(M=255), dict(B=0, M=0), dict(S=0, M=0), dict(Hq=0), dict(Hkv=0), dict(Hkv=3), dict(h_lo=-1), dict(h_hi=9), dict(h_lo=3, h_hi=3),
               dict(h_lo=5, h_hi=4), dict(d=32), dict(d=96, ldq=768, ldk=192, ldv=192, ldg=768), dict(d=256, ldq=2048, ldk=512, ldv=512, ldg=2048),
               dict(dtype=F32, d=6, ldq=48, ldk=12, ldv=12, ldg=48), dict(dtype=F32, d=260, ldq=2080, ldk=520, ldv=520, ldg=2080), dict(d=0),
               dict(ldq=504), dict(ldk=120), dict(ldv=120), dict(ldg=504), dict(row_lo=A), dict(row_hi=A)):
        assert call(**kw) == ESHAPE, kw
    for kw in (dict(q=A + 2), dict(k=A + 8), dict(v=A + 4), dict(g=A + 8), dict(ldq=516), dict(ldk=132), dict(ldv=130), dict(ldg=514),
               dict(out=A + 2), {**f32_32, "ldq": 258}, {**f32_32, "g": A + 4}):
        assert call(**kw) == EALIGN, kw
    # what bf16 refuses, fp32 serves (checked up to the alignment stage: an unaligned out is the last thing looked at)
    assert call(**f32_32, out=A + 1) == EALIGN and call(dtype=F32, d=8, ldq=64, ldk=16, ldv=16, ldg=64, out=A + 1) == EALIGN
    assert call(row_lo=A, row_hi=A, out=A + 1) == EALIGN


def test_attn_relmap_binding_rejects_cpu_tensors():
    from lxt_amd import ops
    q, kv, lse = torch.randn(8, 64), torch.randn(8, 32), torch.zeros(2, 2, 4)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.attn_relmap(q, kv, kv, q, lse, 2, 4, 2, 1, 32, 1.0)
    with pytest.raises(ValueError):
        ops.attn_relmap(q, kv, q, q, lse, 2, 4, 2, 1, 32, 1.0)              # v is not [B S, Hkv d]
    with pytest.raises(ValueError):
        ops.attn_relmap(q, kv, kv, q, torch.zeros(2, 4, 2), 2, 4, 2, 1, 32, 1.0)      # lse is not [B, Hq, S]


def test_attn_map_request_forms():
    from lxt_amd.engine import attn_map_request
    bf, f4 = torch.bfloat16, torch.float32
    req = lambda a, nL=4, nq=8, d=128, dt=bf, mode="efficient": attn_map_request(a, nL, nq, d, dt, mode)      # noqa: E731
    assert req(None) == (False, ()) and req([]) == (False, ()) and req(None, d=36, mode="explicit") == (False, ())
    assert req("sum") == (True, ()) and req(["sum"]) == (True, ())               # the name as a string, not as its letters
    assert req([(0, 1), (3, 7)]) == (False, ((0, 1), (3, 7)))
    assert req([(3, 7), (0, 1), (3, 7), [0, 1]]) == (False, ((3, 7), (0, 1)))     # repeated pairs count once, first mention keeps its place
    assert req(((1, 2), "sum", (0, 0), "sum")) == (True, ((1, 2), (0, 0)))       # mixed forms
    assert req(iter([(2, 3)]), d=32, dt=f4) == (False, ((2, 3),)) and req("sum", d=64) == (True, ())
    hash(req(["sum", (1, 2)]))                                                  # (part of the graph cache's key)
    for bad in ("su", "s", ["nope"], ["sum", "out"], 3, 2.5, [3], [(0,)], [(0, 1, 2)], [(0.5, 1)], [("0", 1)], [(4, 0)], [(0, 8)], [(-1, 0)],
                [(0, -1)], [None], [(0, 1), "total"]):
        with pytest.raises(ValueError):
            req(bad)
    # a head dim or dtype the kernel does not serve, and the explicit placement
    for d, dt in ((32, bf), (96, bf), (256, bf), (6, f4), (260, f4), (None, bf), (128, torch.float16)):
        with pytest.raises(ValueError, match="no kernel"):
            req("sum", d=d, dt=dt)
    for a in ("sum", [(0, 0)]):
        with pytest.raises(ValueError, match="efficient placement"):
            req(a, mode="explicit")


def test_explain_rejects_attn_map_before_anything_runs():
    """LlamaLRP.explain checks attn_map first: a stub without weights or a device raises the ValueError, not an error of a missing kernel input"""
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_qwen import QwenLRP
    ids = torch.zeros(1, 4, dtype=torch.long)
    for cls in (LlamaLRP, QwenLRP):
        stub = cls.__new__(cls)
        stub.cfg, stub.dtype = dict(hidden=64, inter=128, vocab=32, head_dim=64, n_heads=2), torch.bfloat16
        with pytest.raises(ValueError, match="unknown request"):
            stub.explain(ids, attn_map=["nope"])
        with pytest.raises(ValueError, match="iterable"):
            stub.explain(ids, attn_map=3)
        with pytest.raises(ValueError, match="outside the model"):
            stub.explain(ids, attn_map=[(0, 0)])                     # (a stub has no layers)
        stub.mode = "explicit"
        with pytest.raises(ValueError, match="efficient placement"):
            stub.explain(ids, attn_map="sum")


@pytest.mark.parametrize("name,heads,L,nq,S", [("attn_map_llama.npz", "heads_llama.npz", 4, 8, 128), ("attn_map_qwen3.npz", "heads_qwen3.npz", 3, 4, 80)])
def test_fixture_identities(name, heads, L, nq, S):
    fx, hx = load(name), load(heads)
    layers = fx["head_layers"].tolist()
    tot, per = fx["total"], fx["per_head"]
    assert tot.shape == (L, S, S) and tot.dtype == np.float64 and np.isfinite(tot).all() and np.abs(tot).max() > 0
    assert per.shape == (len(layers), nq, S, S) and np.isfinite(per).all() and layers[0] == 0 and layers[-1] == L - 1
    assert fx["ids"].shape == (S,) and int(fx["idx"]) == int(hx["idx"]) and "retain_grad" in str(fx["protocol"])
    scale = np.abs(hx["out"]).max()
    # invisible (i, j) carry nothing; above the top layer only the last query row is live
    up = np.triu(np.ones((S, S), dtype=bool), 1)
    assert not tot[:, up].any() and not per[:, :, up].any()
    assert not tot[-1, :-1].any() and np.abs(tot[-1, -1]).max() > 0
    # a row of the map splits what the head writes at that position (heads_*.npz's `out`) over the source positions
    assert np.abs(tot.sum(-1) - hx["out"].sum(1)).max() <= 1e-12 * scale
    assert np.abs(per.astype(np.float64).sum(-1) - hx["out"][layers]).max() <= 1e-6 * scale        # (stored as float32)
    # the head sum is the sum of the per-head maps where those are stored
    assert np.abs(per.astype(np.float64).sum(1) - tot[layers]).max() <= 1e-6 * scale
