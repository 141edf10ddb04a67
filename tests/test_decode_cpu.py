"""CPU: the decode entry points of include/lrp_hip_decode.h are declared, exported and validate their arguments before any launch (host
pointers only); the workspace and slab queries agree; the generate_*.npz fixtures hold what their generator asserts."""
import ctypes

import numpy as np
import pytest
import torch

from tests.util import load

NAMES = ("lrp_decode_rope_append", "lrp_attn_decode", "lrp_attn_decode_slab", "lrp_attn_decode_ws")
EINVAL, EALIGN, ESHAPE = -1, -2, -3


def test_decode_symbols_declared_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert name in decls, f"{name} is not declared in a header lrp_hip.h includes"
        assert hasattr(raw, name), f"{name} declared but not exported"
    assert decls["lrp_attn_decode_ws"][0] == "int64_t" and decls["lrp_attn_decode_slab"] == ("int", [])
    assert len(decls["lrp_decode_rope_append"][1]) == 20 and len(decls["lrp_attn_decode"][1]) == 19
    assert L.lib.lrp_version() == 8


def test_slab_and_workspace_are_consistent():
    import lxt_amd._lib as L
    lib = L.lib
    slab = lib.lrp_attn_decode_slab()
    assert slab >= 16 and slab & (slab - 1) == 0
    for B, Hq, d, cap in ((1, 4, 32, 1), (3, 8, 128, slab), (3, 8, 128, slab + 1), (2, 32, 128, 2112), (1, 1, 8, 5 * slab - 1), (4, 8, 256, 4096)):
        ns = -(-cap // slab)
        need = B * Hq * ns * (d + 2) * 4            # (m, l, acc [d]) fp32 per (prompt, head, slab)
        got = lib.lrp_attn_decode_ws(B, Hq, d, cap)
        assert got % 16 == 0 and need <= got < need + 16, (B, Hq, d, cap, got)
    # one more key past a slab boundary is one more slab; nothing else changes the size
    assert lib.lrp_attn_decode_ws(2, 8, 64, slab + 1) == 2 * lib.lrp_attn_decode_ws(2, 8, 64, slab)
    for bad in ((0, 4, 32, 8), (1, 0, 32, 8), (1, 4, 4, 8), (1, 4, 36, 8), (1, 4, 264, 8), (1, 4, 32, 0)):
        assert lib.lrp_attn_decode_ws(*bad) == -1, bad


def test_rope_append_argument_ladder_without_gpu():
    """NULL -> EINVAL, shapes -> ESHAPE, the 16-byte grid -> EALIGN, in that order and all of it before a launch: the pointers are host
    integers that no kernel may ever see"""
    import lxt_amd._lib as L
    lib, F32, BF16 = L.lib, L.F32, L.BF16
    P = 4096          # "pointers" on the 16-byte grid

    def call(qk=P, ldqk=6 * 64, v=P, ldv=2 * 64, cos=P, sin=P, rows=64, pos=P, q_rot=P, ldq=4 * 64, kc=P, vc=P, ldc=2 * 64, B=2, cap=16, nq=4,
             nk=2, d=64, dtype=BF16):
        return lib.lrp_decode_rope_append(qk, ldqk, v, ldv, cos, sin, rows, pos, q_rot, ldq, kc, vc, ldc, B, cap, nq, nk, d, dtype, None)

    for name in ("qk", "v", "cos", "sin", "pos", "q_rot", "kc", "vc"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(B=-1), dict(nq=0), dict(nk=0), dict(cap=0), dict(rows=0), dict(dtype=7)):
        assert call(**kw) == EINVAL, kw
    # (NULL wins over a bad shape, a bad shape over a bad alignment)
    assert call(qk=None, d=3) == EINVAL and call(d=3, kc=P + 2) == ESHAPE
    for kw in (dict(d=0), dict(d=63), dict(d=260), dict(d=4), dict(d=12), dict(ldqk=6 * 64 - 8), dict(ldv=2 * 64 - 8), dict(ldq=4 * 64 - 8),
               dict(ldc=2 * 64 - 8)):
        assert call(**kw) == ESHAPE, kw
    # d * sizeof(T) on the 16-byte grid: fp32 takes d = 4, not d = 2 (every accepted call here has B = 0: nothing may launch on these pointers)
    assert call(d=4, dtype=F32, ldqk=24, ldv=8, ldq=16, ldc=8, B=0) == 0 and call(d=2, dtype=F32) == ESHAPE
    for name in ("qk", "v", "q_rot", "kc", "vc", "cos", "sin"):
        assert call(**{name: P + 8}) == EALIGN, name
    assert call(pos=P + 2) == EALIGN and call(pos=P + 4, B=0) == 0
    for kw in (dict(ldqk=6 * 64 + 4), dict(ldv=2 * 64 + 4), dict(ldq=4 * 64 + 4), dict(ldc=2 * 64 + 4)):
        assert call(**kw) == EALIGN, kw
    assert call(ldc=2 * 64 + 2, dtype=F32) == EALIGN and call(ldc=2 * 64 + 4, dtype=F32, B=0) == 0
    assert call(B=0) == 0                                    # nothing to do, nothing launched


def test_attn_decode_argument_ladder_without_gpu():
    import lxt_amd._lib as L
    lib, F32, BF16 = L.lib, L.F32, L.BF16
    P = 4096

    def call(q=P, ldq=8 * 64, kc=P, vc=P, ldc=2 * 64, lo=P, pos=P, o=P, ldo=8 * 64, ws=P, ws_bytes=None, B=2, cap=100, Hq=8, Hkv=2, d=64,
             dtype=BF16):
        if ws_bytes is None:
            ws_bytes = max(lib.lrp_attn_decode_ws(max(B, 1), max(Hq, 1), d, max(cap, 1)), 16)
        return lib.lrp_attn_decode(q, ldq, kc, vc, ldc, lo, pos, o, ldo, ws, ws_bytes, B, cap, Hq, Hkv, d, 0.125, dtype, None)

    for name in ("q", "kc", "vc", "lo", "pos", "o", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(B=-1), dict(Hq=0, ws_bytes=16), dict(Hkv=0), dict(cap=0, ws_bytes=16), dict(dtype=2)):
        assert call(**kw) == EINVAL, kw
    assert call(q=None, Hkv=3) == EINVAL and call(Hkv=3, q=P + 4) == ESHAPE
    for kw in (dict(Hkv=3), dict(d=4, ws_bytes=1 << 20), dict(d=36, ws_bytes=1 << 20), dict(d=264, ws_bytes=1 << 20), dict(ldq=8 * 64 - 8),
               dict(ldo=8 * 64 - 8), dict(ldc=2 * 64 - 8), dict(B=65536, ws_bytes=1 << 40)):
        assert call(**kw) == ESHAPE, kw
    need = lib.lrp_attn_decode_ws(2, 8, 64, 100)
    assert call(ws_bytes=need - 1) == ESHAPE and call(ws_bytes=need - 1, o=P + 2) == ESHAPE
    for name in ("q", "kc", "vc", "o", "ws"):
        assert call(**{name: P + 8}) == EALIGN, name
    assert call(lo=P + 2) == EALIGN and call(pos=P + 1) == EALIGN
    for kw in (dict(ldq=8 * 64 + 4), dict(ldo=8 * 64 + 4), dict(ldc=2 * 64 + 4), dict(ldc=2 * 64 + 2, dtype=F32)):
        assert call(**kw) == EALIGN, kw
    assert call(B=0) == 0 and call(B=0, ws_bytes=0) == 0


def test_ops_wrappers_refuse_host_tensors():
    """the wrappers check shapes, dtypes and strides first and hand only device tensors on: a CPU tensor raises, nothing falls back"""
    import lxt_amd.ops as ops
    assert ops.ATTN_DECODE_SLAB == ops.lib.lrp_attn_decode_slab()
    q, kc = torch.zeros(2, 4 * 32), torch.zeros(2, 8, 2 * 32)
    pos, lo = torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.attn_decode(q, kc, kc.clone(), lo, pos, 4, 2, 32, 1.0)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.decode_rope_append(torch.zeros(2, 6 * 32), torch.zeros(2, 2 * 32), torch.zeros(8, 32), torch.zeros(8, 32), pos, q, kc, kc.clone(), 4, 2, 32)
    with pytest.raises(ValueError):
        ops.attn_decode_ws(1, 4, 36, 8)


CASES = (("llama", 12), ("qwen2", 9), ("qwen3", 27))


@pytest.mark.parametrize("name,distinct", CASES)
def test_generate_fixture_holds_what_the_generator_asserts(name, distinct):
    from tests.golden import make_golden_generate as gg
    from tests.golden.hf_models import wsum
    fx = load(f"generate_{name}.npz")
    B, S, T = gg.B, gg.S, gg.NEW
    V = fx["logits"].shape[-1]
    assert fx["ids"].shape == (B, S) and fx["tokens"].shape == (B, T) and fx["logits"].shape == (B, T, V) and fx["logits"].dtype == np.float64
    assert tuple(fx["lengths"]) == gg.LENGTHS == (24, 15, 7)
    assert np.array_equal(fx["ids"], gg.prompts(name, V).numpy()), "the seeded prompts did not reproduce"
    assert np.array_equal(fx["logits"].argmax(-1), fx["tokens"])
    top2 = np.sort(fx["logits"], -1)[..., -2:]
    margin = float((top2[..., 1] - top2[..., 0]).min())
    assert margin == float(fx["margin"]) and margin >= 2e-4
    assert len(set(fx["tokens"].ravel().tolist())) == distinct          # (a continuation that collapsed to one repeated token would test little)
    got = wsum(gg.build(name))
    assert abs(got - float(fx["wsum"])) <= 1e-9 * got, "the seeded weights did not reproduce"


def test_hf_fp32_reproduces_the_llama_fixture_tokens():
    from tests.golden import make_golden_generate as gg
    fx = load("generate_llama.npz")
    model, ids = gg.build("llama"), torch.from_numpy(fx["ids"])
    for b, n in enumerate(gg.LENGTHS):
        toks, logits = gg.greedy(model, ids[b, gg.S - n:], gg.NEW)
        assert np.array_equal(toks, fx["tokens"][b]), b
        assert np.abs(logits - fx["logits"][b]).max() <= 1e-5 * np.abs(fx["logits"][b]).max()
