"""GPU: lrp_decode_qknorm_rope_append (csrc/decode_site.hip) bit for bit against the three launches it replaces (head_rmsnorm_fwd on q,
head_rmsnorm_fwd on k, decode_rope_append), and the two kernels of csrc/decode.hip at head dim 256, which no other test runs above 128:
attn_decode against fp64 with its bitwise invariants, decode_rope_append against rope_fwd(seq = 1)."""
import pytest
import torch

from tests.decode_ref import BAR, DEV, DTYPES, bits
from tests.decode_ref import make_case as attn_case
from tests.decode_ref import reference as attn_reference

pytestmark = pytest.mark.gpu

# d == one 16-byte vector (fp32 4, bf16 8): both composed kernels accept it, and d / 2 is then NOT a whole number of vectors (the rotate-half
# partner sits inside the lane's own vector)
ONE_VECTOR = {"fp32": 4, "bf16": 8}
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    import lxt_amd.ops as ops
    return ops


def site_case(dtype, B, nq, nk, d, cap, rows, seed):
    """q | k | v as column ranges of one PADDED projection buffer (pitch > (nq + 2 nk) d), norm weights, tables"""
    g = torch.Generator().manual_seed(seed)
    epc = 16 // torch.empty(0, dtype=dtype).element_size()
    width = (nq + 2 * nk) * d
    buf = torch.randn(B, width + 3 * epc, generator=g).to(dtype).to(DEV)
    qkv = buf[:, epc: epc + width]                    # a pitched view that does not start at the buffer's first column
    wq = (torch.randn(d, generator=g) * 0.3).to(dtype).to(DEV)
    wk = (torch.randn(d, generator=g) * 0.3).to(dtype).to(DEV)
    ang = torch.rand(rows, d, generator=g) * 6.0
    return qkv, wq, wk, ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()


def caches(dtype, B, cap, nkd):
    nan = torch.full((B, cap, nkd), float("nan"), dtype=dtype, device=DEV)
    return nan, nan.clone()


def three_launches(ops, qkv, wq, wk, cos, sin, pos, kc, vc, q_rot, nq, nk, d, w_off):
    B, nqk = qkv.shape[0], (nq + nk) * d
    qn = torch.empty(B, nqk, dtype=qkv.dtype, device=DEV)
    ops.head_rmsnorm_fwd(qkv[:, : nq * d], wq, qn[:, : nq * d], torch.empty(B * nq, device=DEV), nq, d, EPS, w_off)
    ops.head_rmsnorm_fwd(qkv[:, nq * d: nqk], wk, qn[:, nq * d:], torch.empty(B * nk, device=DEV), nk, d, EPS, w_off)
    return ops.decode_rope_append(qn, qkv[:, nqk:], cos, sin, pos, q_rot, kc, vc, nq, nk, d)


@pytest.mark.parametrize("w_off", [0.0, 1.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [(4, 2), (8, 4), (3, 1)], ids=lambda h: f"q{h[0]}k{h[1]}")
@pytest.mark.parametrize("dkind", ["d32", "d256", "one_vector"])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_site_kernel_is_bitwise_the_three_launches(ops, dname, dkind, heads, B, w_off):
    """q_rot, cache row p of kc / vc and every other cache row (NaN sentinels, untouched) against the composition, for p at the first row,
    inside and at the last row of a cache of cap = 7; p = -1, cap and table_rows write nothing"""
    dtype, (nq, nk) = DTYPES[dname], heads
    d = dict(d32=32, d256=256, one_vector=ONE_VECTOR[dname])[dkind]
    cap, rows, nqk = 7, 9, (nq + nk) * d
    qkv, wq, wk, cos, sin = site_case(dtype, B, nq, nk, d, cap, rows, seed=7 * d + nq + B)
    for p_ in (0, 5, 6):
        pos = torch.tensor([p_], dtype=torch.int32, device=DEV)
        kc_r, vc_r = caches(dtype, B, cap, nk * d)
        q_r = three_launches(ops, qkv, wq, wk, cos, sin, pos, kc_r, vc_r, torch.zeros(B, nq * d, dtype=dtype, device=DEV), nq, nk, d, w_off)
        kc, vc = caches(dtype, B, cap, nk * d)
        q = ops.decode_qknorm_rope_append(qkv[:, :nqk], qkv[:, nqk:], wq, wk, EPS, cos, sin, pos, torch.zeros(B, nq * d, dtype=dtype, device=DEV),
                                          kc, vc, nq, nk, d, w_off)
        assert bool(torch.isfinite(q_r).all()) and bool(torch.isfinite(kc_r[:, p_]).all())
        assert torch.equal(bits(q), bits(q_r)), f"q_rot differs at p={p_}"
        assert torch.equal(bits(kc[:, p_]), bits(kc_r[:, p_])), f"the appended k row differs at p={p_}"
        assert torch.equal(bits(vc[:, p_]), bits(qkv[:, nqk:])) and torch.equal(bits(vc), bits(vc_r)), f"the appended v row differs at p={p_}"
        assert torch.equal(bits(kc), bits(kc_r)), f"a cache row other than p={p_} was written"
        again_k, again_v = caches(dtype, B, cap, nk * d)
        q2 = ops.decode_qknorm_rope_append(qkv[:, :nqk], qkv[:, nqk:], wq, wk, EPS, cos, sin, pos, torch.zeros_like(q), again_k, again_v, nq, nk,
                                           d, w_off)
        assert torch.equal(bits(q2), bits(q)) and torch.equal(bits(again_k), bits(kc)), "a repeated call differs"
    for bad, big in ((-1, cap), (cap, cap), (rows, rows + 4)):          # (past the TABLES inside a larger cache: nothing is written either)
        kc, vc = caches(dtype, B, big, nk * d)
        fresh_k, fresh_v = caches(dtype, B, big, nk * d)
        q = torch.full((B, nq * d), 9.0, dtype=dtype, device=DEV)
        ops.decode_qknorm_rope_append(qkv[:, :nqk], qkv[:, nqk:], wq, wk, EPS, cos, sin, torch.tensor([bad], dtype=torch.int32, device=DEV), q, kc,
                                      vc, nq, nk, d, w_off)
        assert bool((q == 9.0).all()) and torch.equal(bits(kc), bits(fresh_k)) and torch.equal(bits(vc), bits(fresh_v)), bad


def test_site_kernel_refuses_what_a_composed_kernel_refuses(ops):
    """d = 24 in bf16 and d = 12 in fp32 are head dims decode_rope_append takes and head_rmsnorm_fwd does not (3 vectors: no power of two)"""
    for dtype, d in ((torch.bfloat16, 24), (torch.float32, 12), (torch.bfloat16, 512)):
        qkv = torch.zeros(2, 4 * d, dtype=dtype, device=DEV)
        w = torch.zeros(d, dtype=dtype, device=DEV)
        tab = torch.zeros(4, d, device=DEV)
        kc = torch.zeros(2, 4, d, dtype=dtype, device=DEV)
        with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
            ops.decode_qknorm_rope_append(qkv[:, : 3 * d], qkv[:, 3 * d:], w, w, EPS, tab, tab, torch.zeros(1, dtype=torch.int32, device=DEV),
                                          torch.zeros(2, 2 * d, dtype=dtype, device=DEV), kc, kc.clone(), 2, 1, d, 1.0)


# ---- the two kernels of csrc/decode.hip at d = 256 -------------------------------------------------------------------------------------
# the bars: tests/decode_ref.py
LIVES = (1, 63, 64, 65, 197)


@pytest.mark.parametrize("heads", [(8, 4), (4, 1)], ids=lambda h: f"h{h[0]}kv{h[1]}")
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_attn_decode_d256_against_fp64_and_bitwise_invariants(ops, dname, B, heads):
    dtype, (Hq, Hkv), d, s = DTYPES[dname], heads, 256, ops.ATTN_DECODE_SLAB
    scale = d ** -0.5
    worst = 0.0
    for n in LIVES:
        for lo_kind in ("zeros", "mixed"):
            lo_l = [0] * B if lo_kind == "zeros" else [(0, n - 1, n // 2)[b % 3] for b in range(B)]
            lo = torch.tensor(lo_l, dtype=torch.int32, device=DEV)
            pos = torch.tensor([n - 1], dtype=torch.int32, device=DEV)
            outs = {}
            for cap in (n, n + s + 3):
                q, kc, vc = attn_case(dtype, B, n, cap, Hq, Hkv, d, lo_l, seed=1000 * n + Hq)
                o = ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale)
                assert bool(torch.isfinite(o).all()), f"a poisoned cache row reached the result (n={n}, cap={cap}, lo={lo_l})"
                outs[cap] = o
                if cap == n:
                    ref = attn_reference(q, kc, vc, lo_l, n, Hq, Hkv, d, scale)
                    err = float((o.double().cpu() - ref).abs().max() / ref.abs().max())
                    worst = max(worst, err)
                    assert err <= BAR[dname], f"n={n} lo={lo_l}: {err:.3e} > {BAR[dname]:.3e}"
                    for b in range(B if B > 1 else 0):          # prompt b alone == its row of the batch
                        ob = ops.attn_decode(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], lo[b:b + 1].clone(), pos, Hq, Hkv, d, scale)
                        assert torch.equal(ob[0], o[b]), f"prompt {b} alone differs from its row in the batch (n={n})"
            assert torch.equal(outs[n], outs[n + s + 3]), f"the result depends on cap (n={n})"
    print(f"attn_decode {dname} d=256 B={B} Hq/Hkv={Hq}/{Hkv}: worst max-normalised error vs fp64 {worst:.3e} (bar {BAR[dname]:.3e})")


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_decode_rope_append_d256_bitwise(ops, dname):
    dtype, d = DTYPES[dname], 256
    B, nq, nk, cap, rows = 3, 8, 4, 9, 16
    g = torch.Generator().manual_seed(d)
    qkv = torch.randn(B, (nq + 2 * nk) * d, generator=g).to(dtype).to(DEV)
    nqk = (nq + nk) * d
    ang = torch.rand(rows, d, generator=g) * 6.0
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    for p_ in (0, 4, cap - 1):
        kc, vc = caches(dtype, B, cap, nk * d)
        fresh, _ = caches(dtype, B, cap, nk * d)
        pos = torch.tensor([p_], dtype=torch.int32, device=DEV)
        q_rot = ops.decode_rope_append(qkv[:, :nqk], qkv[:, nqk:], cos, sin, pos, torch.zeros(B, nq * d, dtype=dtype, device=DEV), kc, vc, nq, nk, d)
        want = ops.rope_fwd(qkv[:, :nqk], torch.empty(B, nqk, dtype=dtype, device=DEV), cos[p_:p_ + 1].contiguous(), sin[p_:p_ + 1].contiguous(),
                            1, nq + nk, d)
        assert torch.equal(q_rot, want[:, : nq * d]) and torch.equal(kc[:, p_], want[:, nq * d:]) and torch.equal(vc[:, p_], qkv[:, nqk:])
        keep = torch.ones(cap, dtype=torch.bool, device=DEV)
        keep[p_] = False
        assert torch.equal(bits(kc[:, keep]), bits(fresh[:, keep])) and torch.equal(bits(vc[:, keep]), bits(fresh[:, keep]))
