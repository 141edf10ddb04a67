"""CPU: the read-outs of the Gemma-3 drivers (Gemma3LRP / Gemma3MMLRP .explain(layer_relevance, latent, heads, attn_map), DESIGN.md section
19) -- lrp_attn_relmap_d256 is declared, exported, bound and rejects bad calls before any launch; the Gemma-side map request accepts
bf16 / 256 and refuses what the shared parser refuses; explain() checks its requests before anything else; the three fixtures of the real
reference (tests/golden/make_golden_gemma3_readouts.py) reload and satisfy the identities their generator asserted."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests.util import load


def test_relmap_d256_symbol_declared_exported_and_bound():
    import lxt_amd._lib as L
    decls = L.parse_header()
    assert decls["lrp_attn_relmap_d256"] == decls["lrp_attn_relmap"]          # the sibling's argument list, in its order
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "lrp_attn_relmap_d256") and L.lib.lrp_attn_relmap_d256 is not None
    from lxt_amd import ops
    assert "lrp_attn_relmap_d256" in inspect.getsource(ops.attn_relmap)


def test_relmap_d256_argument_validation_without_gpu():
    import lxt_amd._lib as L
    lib, BF16, F32 = L.lib, L.BF16, L.F32
    A = 1 << 12                                   # an aligned fake device address: every call below is rejected before a launch
    # 2 prompts x 128 rows, 8 query heads over 2 kv heads of d = 256: q, g [256, 2048], k, v [256, 512]
    ok = dict(q=A, k=A, v=A, g=A, lse=A, out=A, M=256, B=2, S=128, Hq=8, Hkv=2, d=256, h_lo=0, h_hi=8, ldq=2048, ldk=512, ldv=512, ldg=2048,
              scale=0.0625, gscale=1.0, causal=1, row_lo=None, row_hi=None, dtype=BF16, stream=None)
    call = lambda **kw: lib.lrp_attn_relmap_d256(*{**ok, **kw}.values())      # noqa: E731
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(g=None), dict(lse=None), dict(out=None), dict(dtype=7)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(M=255), dict(B=0, M=0), dict(S=0, M=0), dict(Hq=0), dict(Hkv=0), dict(Hkv=3), dict(h_lo=-1), dict(h_hi=9), dict(h_lo=3, h_hi=3),
               dict(h_lo=5, h_hi=4), dict(d=0), dict(d=32), dict(d=64, ldq=512, ldk=128, ldv=128, ldg=512),
               dict(d=128, ldq=1024, ldk=256, ldv=256, ldg=1024), dict(d=512, ldq=4096, ldk=1024, ldv=1024, ldg=4096), dict(dtype=F32),
               dict(dtype=F32, d=128, ldq=1024, ldk=256, ldv=256, ldg=1024), dict(dtype=F32, d=32, ldq=256, ldk=64, ldv=64, ldg=256),
               dict(ldq=2040), dict(ldk=504), dict(ldv=504), dict(ldg=2040), dict(row_lo=A), dict(row_hi=A), dict(B=65536, S=1, M=65536)):
        assert call(**kw) == ESHAPE, kw
    for kw in (dict(q=A + 2), dict(k=A + 8), dict(v=A + 4), dict(g=A + 8), dict(ldq=2052), dict(ldk=516), dict(ldv=514), dict(ldg=2050),
               dict(out=A + 2), dict(lse=A + 2), dict(row_lo=A + 2, row_hi=A), dict(row_lo=A, row_hi=A + 1)):
        assert call(**kw) == EALIGN, kw
    # served up to the alignment stage (an unaligned out is the last thing looked at): padded pitches, intervals, a head range, rep 4
    assert call(out=A + 1) == EALIGN and call(ldq=2056, ldk=520, ldv=528, ldg=2064, out=A + 1) == EALIGN
    assert call(row_lo=A, row_hi=A, out=A + 1) == EALIGN and call(Hq=4, Hkv=1, h_lo=1, h_hi=3, out=A + 1) == EALIGN
    # the sibling still refuses bf16 / 256: the new entry is the only way in
    assert lib.lrp_attn_relmap(*ok.values()) == ESHAPE


def test_gemma_attn_map_request_forms():
    from lxt_amd.engine import attn_map_request
    from lxt_amd.engine_gemma3 import gemma_attn_map_request
    bf, f4 = torch.bfloat16, torch.float32
    req = lambda a, nL=3, nq=4, d=256, dt=bf, mode="efficient": gemma_attn_map_request(a, nL, nq, d, dt, mode)      # noqa: E731
    assert req(None) == (False, ()) and req("sum") == (True, ()) and req(["sum", (2, 3), (0, 0), (2, 3)]) == (True, ((2, 3), (0, 0)))
    assert req("sum", d=256, dt=f4) == (True, ()) and req("sum", d=32, dt=f4) == (True, ()) and req([(1, 1)], d=128) == (False, ((1, 1),))
    for d, dt in ((32, bf), (96, bf), (512, bf), (260, f4), (None, bf), (256, torch.float16)):
        with pytest.raises(ValueError, match="no kernel"):
            req("sum", d=d, dt=dt)
    for a in ("sum", [(0, 0)]):
        with pytest.raises(ValueError, match="efficient placement"):
            req(a, mode="explicit")
    for bad in ("su", ["nope"], 3, [(0,)], [(3, 0)], [(0, 4)], [(-1, 0)], [(0.5, 1)], [None]):
        with pytest.raises(ValueError):
            req(bad)
    with pytest.raises(ValueError, match="no kernel"):          # the shared parser keeps its behaviour
        attn_map_request("sum", 3, 4, 256, bf, "efficient")


def test_explain_rejects_requests_before_anything_runs():
    """a stub without weights, layers or a device raises the request's ValueError, not an error of a missing attribute or input"""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_gemma3_mm import Gemma3MMLRP
    stub = Gemma3LRP.__new__(Gemma3LRP)
    stub.cfg, stub.dtype = dict(hidden=64, inter=128, vocab=32, head_dim=256, n_heads=2), torch.bfloat16
    ids = torch.zeros(1, 4, dtype=torch.long)
    mm = Gemma3MMLRP.__new__(Gemma3MMLRP)
    mm.text, mm.vision = stub, None
    for call in (lambda **kw: stub.explain(ids, **kw), lambda **kw: mm.explain(ids, None, **kw)):
        with pytest.raises(ValueError, match="unknown request"):
            call(attn_map=["nope"])
        with pytest.raises(ValueError, match="outside the model"):
            call(attn_map=[(0, 0)])                     # (a stub has no layers)
        with pytest.raises(ValueError, match="unknown read-out"):
            call(heads=["out", "nope"])
    with pytest.raises(ValueError, match="unknown read-out"):
        stub.explain(ids, latent="neurons")
    with pytest.raises(TypeError):
        mm.explain(ids, None, latent="mlp")             # the image + text driver takes no latent read-outs
    stub.dtype = torch.float16
    with pytest.raises(ValueError, match="no kernel"):
        stub.explain(ids, attn_map="sum")


@pytest.mark.parametrize("name,L,nq,S,H,I,stored", [("gemma3_readouts_tiny.npz", 4, 4, 80, 128, 256, 4), ("gemma3_readouts_d256.npz", 3, 4, 136, 256, 512, 3)])
def test_text_fixture_identities(name, L, nq, S, H, I, stored):
    fx = load(name)
    tot, per, out = fx["total"], fx["per_head"], fx["out"]
    layers, w, sliding = fx["head_layers"].tolist(), int(fx["window"]), fx["layer_sliding"].tolist()
    assert fx["ids"].shape == (S,) and "retain_grad" in str(fx["protocol"]) and len(layers) == stored and sliding == [True] * (L - 1) + [False]
    assert fx["trace"].shape == (L + 1, S) and fx["resid"].shape == (L + 1, H) and fx["mlp"].shape == (L, I)
    assert all(fx[k].shape == (L, nq, S) and fx[k].dtype == np.float64 for k in ("out", "q", "k", "v"))
    assert tot.shape == (L, S, S) and tot.dtype == np.float64 and per.shape == (stored, nq, S, S) and np.abs(tot).max() > 0
    scale = np.abs(out).max()
    i = np.arange(S)
    up, outside = i[None, :] > i[:, None], i[None, :] <= i[:, None] - w
    assert outside.any() and not tot[:, up].any() and not per[:, :, up].any()
    for l in range(L):
        assert not tot[l][outside].any() if sliding[l] else np.abs(tot[l][outside]).max() > 0
    assert not tot[-1, :-1].any() and np.abs(tot[-1, -1]).max() > 0 and not fx["q"][-1, :, :-1].any()
    assert np.abs(tot.sum(-1) - out.sum(1)).max() <= 1e-12 * scale
    assert np.abs(per.astype(np.float64).sum(-1) - out[layers]).max() <= 1e-6 * scale
    assert np.abs(fx["v"].sum(-1) - 0.5 * out.sum(-1)).max() <= 1e-12 * scale
    assert np.abs(fx["resid"].sum(-1) - fx["trace"].sum(-1)).max() <= 1e-12 * np.abs(fx["trace"]).max()
    if "d256" in name:
        gaps = {k.split("/")[1]: v for k, v in fx.items() if k.startswith("gap_bf16/")}
        assert set(gaps) == {"trace", "resid", "mlp", "out", "q", "k", "v", "total", "per_head", "layer_R"}
        assert gaps["per_head"].shape == (L, nq) and all(v.shape == () for k, v in gaps.items() if k != "per_head")
        assert all(1e-4 < float(g.min()) and float(g.max()) < 1e-1 for g in gaps.values()), gaps


def test_mm_fixture_identities():
    fx = load("gemma3_mm_readouts.npz")
    S, tt = int(fx["S"]), fx["token_type_ids"][0].astype(bool)
    tot, out = fx["total"], fx["out"]
    assert tot.shape == (3, S, S) and out.shape == (3, 4, S) and fx["layer_R"].shape == (4,) and tt.sum() == 4
    assert np.abs(tot.sum(-1) - out.sum(1)).max() <= 1e-12 * np.abs(out).max()
    up = np.triu(np.ones((S, S), dtype=bool), 1)
    blk = tt[:, None] & tt[None, :]
    assert not tot[:, up & ~blk].any() and np.abs(tot[:2][:, up & blk]).max() > 0          # only an image block looks ahead
    assert not tot[-1, :-1].any()
