"""GPU: the two decode kernels alone (csrc/decode.hip).  attn_decode against an fp64 restatement in torch on caches poisoned with NaN outside
the live interval, with its bitwise properties (repeatable, batch invariant, independent of cap); decode_rope_append bitwise against
ops.rope_fwd on the same rows, with the cache untouched everywhere else and for every column outside it."""
import pytest
import torch

from tests.decode_ref import BAR, DEV, DTYPES, make_case, reference

pytestmark = pytest.mark.gpu


def slab():
    import lxt_amd.ops as ops
    return ops.ATTN_DECODE_SLAB


def lives():
    s = slab()
    return (1, 2, s - 1, s, s + 1, 3 * s + 5)


@pytest.mark.parametrize("heads", [(4, 4), (8, 2), (8, 1)], ids=lambda h: f"h{h[0]}kv{h[1]}")
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_attn_decode_against_fp64_and_bitwise_invariants(dname, B, d, heads):
    import lxt_amd.ops as ops
    dtype, (Hq, Hkv), s = DTYPES[dname], heads, slab()
    scale = d ** -0.5
    worst = 0.0
    for n in lives():
        for lo_kind in ("zeros", "mixed"):
            lo_l = [0] * B if lo_kind == "zeros" else [(0, n - 1, n // 2)[b % 3] for b in range(B)]
            lo = torch.tensor(lo_l, dtype=torch.int32, device=DEV)
            pos = torch.tensor([n - 1], dtype=torch.int32, device=DEV)
            outs = {}
            for cap in (n, n + s + 3):
                q, kc, vc = make_case(dtype, B, n, cap, Hq, Hkv, d, lo_l, seed=1000 * n + d + Hq)
                o = ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale)
                assert bool(torch.isfinite(o).all()), f"a poisoned cache row reached the result (n={n}, cap={cap}, lo={lo_l})"
                assert torch.equal(o, ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale)), "a repeated call differs"
                outs[cap] = o
                if cap == n:
                    ref = reference(q, kc, vc, lo_l, n, Hq, Hkv, d, scale)
                    err = float((o.double().cpu() - ref).abs().max() / ref.abs().max())
                    worst = max(worst, err)
                    assert err <= BAR[dname], f"n={n} lo={lo_l}: {err:.3e} > {BAR[dname]:.3e}"
                    for b in range(B if B > 1 else 0):          # prompt b alone == its row of the batch
                        ob = ops.attn_decode(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], lo[b:b + 1].clone(), pos, Hq, Hkv, d, scale)
                        assert torch.equal(ob[0], o[b]), f"prompt {b} alone differs from its row in the batch (n={n})"
            assert torch.equal(outs[n], outs[n + s + 3]), f"the result depends on cap (n={n})"
    print(f"attn_decode {dname} B={B} d={d} Hq/Hkv={Hq}/{Hkv}: worst max-normalised error vs fp64 {worst:.3e} (bar {BAR[dname]:.3e})")


def test_attn_decode_lo_is_clamped_and_bad_pos_writes_nothing():
    """lo below 0 reads from key 0, lo above *pos reads key *pos alone; *pos outside [0, cap) leaves the output as it was (the guard is
    evaluated on the device on a valid allocation: nothing out of bounds is attempted)"""
    import lxt_amd.ops as ops
    B, Hq, Hkv, d, n = 2, 4, 2, 64, 70
    q, kc, vc = make_case(torch.float32, B, n, n + 5, Hq, Hkv, d, [0, 0], seed=3)
    pos = torch.tensor([n - 1], dtype=torch.int32, device=DEV)
    o = ops.attn_decode(q, kc, vc, torch.tensor([-7, n + 100], dtype=torch.int32, device=DEV), pos, Hq, Hkv, d, 0.125)
    want = ops.attn_decode(q, kc, vc, torch.tensor([0, n - 1], dtype=torch.int32, device=DEV), pos, Hq, Hkv, d, 0.125)
    assert torch.equal(o, want)
    assert torch.equal(o[1].view(Hq, d), vc[1, n - 1].view(Hkv, 1, d).expand(Hkv, Hq // Hkv, d).reshape(Hq, d))      # one key: softmax = 1
    for bad in (-1, n + 5):
        out = torch.full((B, Hq * d), 7.0, device=DEV)
        ops.attn_decode(q, kc, vc, torch.zeros(B, dtype=torch.int32, device=DEV), torch.tensor([bad], dtype=torch.int32, device=DEV), Hq, Hkv, d,
                        0.125, out=out)
        assert bool((out == 7.0).all()), bad


@pytest.mark.parametrize("dname,d", [("fp32", 32), ("fp32", 64), ("fp32", 128), ("fp32", 12), ("bf16", 32), ("bf16", 64), ("bf16", 128), ("bf16", 24)])
def test_decode_rope_append_bitwise(dname, d):
    """q_rot and the appended k row are ops.rope_fwd(seq=1) of the same rows with the tables' row p, bit for bit; v is a copy; every other
    cache row keeps its sentinel; a column outside the cache (or past the tables) writes nothing.  d = 12 in fp32 and d = 24 in bf16
    (d * sizeof(T) on the 16-byte grid, d / 2 not a whole number of vectors) take the element-wise partner loads"""
    import lxt_amd.ops as ops
    dtype = DTYPES[dname]
    B, nq, nk, cap, rows = 3, 4, 2, 9, 16
    g = torch.Generator().manual_seed(d)
    qkv = torch.randn(B, (nq + 2 * nk) * d, generator=g).to(dtype).to(DEV)          # q | k | v: the two views of one buffer
    nqk = (nq + nk) * d
    ang = torch.rand(rows, d, generator=g) * 6.0
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    for p_ in (0, cap - 1):
        kc = torch.full((B, cap, nk * d), 3.0, dtype=dtype, device=DEV)
        vc = torch.full((B, cap, nk * d), 5.0, dtype=dtype, device=DEV)
        q_rot = torch.zeros(B, nq * d, dtype=dtype, device=DEV)
        pos = torch.tensor([p_], dtype=torch.int32, device=DEV)
        ops.decode_rope_append(qkv[:, :nqk], qkv[:, nqk:], cos, sin, pos, q_rot, kc, vc, nq, nk, d)
        want = ops.rope_fwd(qkv[:, :nqk], torch.empty(B, nqk, dtype=dtype, device=DEV), cos[p_:p_ + 1].contiguous(), sin[p_:p_ + 1].contiguous(),
                            1, nq + nk, d)
        assert torch.equal(q_rot, want[:, : nq * d]) and torch.equal(kc[:, p_], want[:, nq * d:])
        assert torch.equal(vc[:, p_], qkv[:, nqk:])
        keep = torch.ones(cap, dtype=torch.bool, device=DEV)
        keep[p_] = False
        assert bool((kc[:, keep] == 3.0).all()) and bool((vc[:, keep] == 5.0).all())
    for bad in (cap, -1, rows + 1):
        big = cap if bad < rows else rows + 4          # (past the TABLES inside a larger cache: nothing is written either)
        kc = torch.full((B, big, nk * d), 3.0, dtype=dtype, device=DEV)
        vc = torch.full((B, big, nk * d), 5.0, dtype=dtype, device=DEV)
        q_rot = torch.full((B, nq * d), 9.0, dtype=dtype, device=DEV)
        ops.decode_rope_append(qkv[:, :nqk], qkv[:, nqk:], cos, sin, torch.tensor([bad], dtype=torch.int32, device=DEV), q_rot, kc, vc, nq, nk, d)
        assert bool((kc == 3.0).all()) and bool((vc == 5.0).all()) and bool((q_rot == 9.0).all()), bad
