"""GPU parity of the two CP-LRP kernels (include/lrp_hip_attn_cp.h): lrp_attn_bwd_dv against an fp64 restatement of

    dv[b, j, hk] = sum_{h in group hk} sum_{i >= max(j, q_begin), j in [lo_i, hi_i)} exp(scale q_h[i].k_hk[j] - lse[b, h, i]) G[b, i, h]

and against gqa_reduce(dv_h) of lrp_attn_bwd_dkv fed the same operands; lrp_gated_cp_bwd_il against act(g) * Gm in fp64.
The bound on dv is the one tests/test_kernels_gpu.py::test_attention holds lrp_attn_bwd_dkv's dv_h to (3 x 3e-5 fp32, 3 x 3e-2 bf16,
normalised max error); the gated kernel's is that file's element-wise bound (2e-5 / 2e-2)."""
import pytest
import torch
import torch.nn.functional as F

from tests.util import nmax

pytestmark = pytest.mark.gpu

DV_TOL = {torch.float32: 3 * 3e-5, torch.bfloat16: 3 * 3e-2}          # test_kernels_gpu.py::test_attention: nmax(dv, dV) < tol * 3
EW_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}                  # test_kernels_gpu.py: TOL
B, HKV = 2, 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.ops as o
    return o


def rnd(*shape, dtype=torch.float32, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _operands(ops, dtype, S, rep, d, row_iv, nb=B):
    """token-major q [nb S, Hq d], k, v, G and the forward's own lse (the formula's operand), prompt b drawn from seed 10 b + ..: a B = 1 call
    on prompt 0 sees the same values"""
    Hq = HKV * rep
    mk = lambda H, s: torch.cat([rnd(S, H * d, dtype=dtype, seed=10 * b + s) for b in range(nb)])      # noqa: E731
    q, k, v, G = mk(Hq, 1), mk(HKV, 2), mk(HKV, 3), mk(Hq, 4)
    v_t = ops.transpose_heads(v, nb, S, HKV, d) if ops.attn_needs_transposed(q, d) else None
    o, lse = torch.empty_like(q), torch.empty(nb, Hq, S, device="cuda")
    ops.attn_fwd(q, k, v, v_t, o, lse, nb, S, Hq, HKV, d, d ** -0.5, True, 0, row_iv=row_iv)
    return q, k, v, G, lse


def _dv_ref(q, k, G, lse, S, rep, d, q_begin, row_iv, nb=B):
    Hq = HKV * rep
    hm = lambda x, H: x.double().view(nb, S, H, d).permute(0, 2, 1, 3)      # noqa: E731
    qd, kx, Gd = hm(q, Hq), hm(k, HKV).repeat_interleave(rep, 1), hm(G, Hq)
    i = torch.arange(S, device="cuda")
    vis = (i[None, :] <= i[:, None]) & (i[:, None] >= q_begin)                      # [query, key]
    vis = vis[None].expand(nb, S, S)
    if row_iv is not None:
        lo, hi = (t.view(nb, S, 1) for t in row_iv)
        vis = vis & (i[None, None, :] >= lo) & (i[None, None, :] < hi)
    P = torch.exp(qd @ kx.transpose(-1, -2) * d ** -0.5 - lse.double()[..., None])
    P = torch.where(vis[:, None], P, torch.zeros_like(P))
    dV = (P.transpose(-1, -2) @ Gd).view(nb, HKV, rep, S, d).sum(2)
    return dV.permute(0, 2, 1, 3).reshape(nb * S, HKV * d)


def _dv(ops, q, k, G, lse, S, rep, d, q_begin=0, row_iv=None, nb=B):
    Hq = HKV * rep
    G_t = ops.transpose_heads(G, nb, S, Hq, d) if ops.attn_needs_transposed(q, d) else None
    dv = torch.full((nb * S, HKV * d), float("nan"), dtype=q.dtype, device="cuda")
    return ops.attn_bwd_dv(q, k, G, lse, dv, nb, S, Hq, HKV, d, d ** -0.5, q_begin=q_begin, row_iv=row_iv, G_t=G_t)


def _intervals(S):
    """prompt 0: left-padded by min(5, S - 1) columns (rows from the pad on have lo = 5; the pad rows see nothing); prompt 1: causal, but its
    last two rows see nothing -- so no query sees keys S - 2, S - 1 of prompt 1, nor the pad keys of prompt 0"""
    i = torch.arange(S, dtype=torch.int32)
    n_pad = min(5, S - 1)
    lo, hi = torch.zeros(B, S, dtype=torch.int32), (i + 1).repeat(B, 1)
    lo[0, n_pad:] = n_pad
    hi[0, :n_pad] = 0
    hi[1, max(S - 2, 0):] = 0
    unseen = torch.zeros(B, S, dtype=torch.bool)
    unseen[0, :n_pad] = True
    unseen[1, max(S - 2, 0):] = True
    return (lo.cuda().contiguous(), hi.cuda().contiguous()), unseen.cuda()


@pytest.mark.parametrize("rep", [1, 4, 8])
@pytest.mark.parametrize("S", [1, 31, 33, 64, 97, 160])
@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 64), (torch.bfloat16, 96), (torch.bfloat16, 128),
                                     (torch.float32, 16), (torch.float32, 64), (torch.float32, 128)])
def test_attn_bwd_dv(ops, dtype, d, S, rep):
    assert ops.attn_bwd_dv_ok(dtype, d)
    Hq, tol = HKV * rep, DV_TOL[dtype]
    q, k, v, G, lse = _operands(ops, dtype, S, rep, d, None)
    for q_begin in (0, S - 1):
        dv = _dv(ops, q, k, G, lse, S, rep, d, q_begin)
        ref = _dv_ref(q, k, G, lse, S, rep, d, q_begin, None)
        err = nmax(dv, ref)
        print(f"dv {dtype} d={d} S={S} rep={rep} q_begin={q_begin}: {err:.3e}")
        assert torch.isfinite(dv.float()).all() and err < tol
    # repeatability and batch invariance: bitwise
    dv0 = _dv(ops, q, k, G, lse, S, rep, d)
    assert torch.equal(dv0, _dv(ops, q, k, G, lse, S, rep, d))
    q1, k1, _, G1, lse1 = _operands(ops, dtype, S, rep, d, None, nb=1)
    assert torch.equal(q1, q[:S]) and torch.equal(lse1[0], lse[0])
    assert torch.equal(_dv(ops, q1, k1, G1, lse1, S, rep, d, nb=1), dv0[:S])
    # the pair it replaces, on the same operands: lrp_attn_bwd_dkv fed Gho = G, then the GQA group sum
    need_t = ops.attn_needs_transposed(q, d)
    q_t, G_t = (ops.transpose_heads(x, B, S, Hq, d) if need_t else None for x in (q, G))
    dk_h, dv_h, red = torch.empty_like(q), torch.empty_like(q), torch.empty_like(dv0)
    ops.attn_bwd_dkv(q, k, v, q_t, G, G_t, lse, torch.zeros(B, Hq, S, device="cuda"), dk_h, dv_h, B, S, Hq, HKV, d, d ** -0.5, 0.0, 0.0)
    ops.gqa_reduce(dv_h, red, B * S, HKV, rep, d)
    err = nmax(dv0, red.double())
    print(f"dv {dtype} d={d} S={S} rep={rep} vs gqa_reduce(dkv dv_h): {err:.3e}")
    assert err < 2 * tol
    # row intervals: left padding and rows that see nothing; keys no query sees get exact zeros
    row_iv, unseen = _intervals(S)
    q, k, v, G, lse = _operands(ops, dtype, S, rep, d, row_iv)
    for q_begin in (0, S - 1):
        dv = _dv(ops, q, k, G, lse, S, rep, d, q_begin, row_iv)
        ref = _dv_ref(q, k, G, lse, S, rep, d, q_begin, row_iv)
        assert torch.isfinite(dv.float()).all()
        assert (dv.view(B, S, -1)[unseen] == 0).all()
        if float(ref.abs().max()) > 0:
            err = nmax(dv, ref)
            print(f"dv {dtype} d={d} S={S} rep={rep} q_begin={q_begin} intervals: {err:.3e}")
            assert err < tol
        else:
            assert (dv == 0).all()


@pytest.mark.parametrize("d", [64, 128])
def test_attn_bwd_dv_both_workgroup_sizes(ops, d):
    """bf16: the host cuts the keys into 128-key (4-wave) workgroups while B Hkv ceil(S / 256) < 4 x the CU count and into 256-key (8-wave)
    ones from there on.  B = 4 x 128 kv heads x 2 key blocks = 1024 workgroups is past that on a 256-CU device, one prompt of it (256) is
    not: the two must agree bitwise (a key's sum does not see the split), and prompt 0 is held to the fp64 formula"""
    import lxt_amd._lib as L
    nb, Hkv, rep, S, dt = 4, 128, 1, 257, torch.bfloat16
    assert nb * Hkv * 2 >= 1024 > Hkv * 2
    q, k, G = (torch.cat([rnd(S, Hkv * d, dtype=dt, seed=10 * b + s) for b in range(nb)]) for s in (1, 2, 4))
    v, o, lse = torch.zeros_like(k), torch.empty_like(q), torch.empty(nb, Hkv, S, device="cuda")
    ops.attn_fwd(q, k, v, None, o, lse, nb, S, Hkv, Hkv, d, d ** -0.5, True, 0)
    run = lambda n: ops.attn_bwd_dv(q[: n * S], k[: n * S], G[: n * S], lse[:n].contiguous(),          # noqa: E731
                                    torch.full((n * S, Hkv * d), float("nan"), dtype=dt, device="cuda"), n, S, Hkv, Hkv, d, d ** -0.5)
    big, one = run(nb), run(1)
    assert torch.isfinite(big.float()).all() and torch.equal(big[:S], one)
    hm = lambda x: x[:S].double().view(S, Hkv, d).permute(1, 0, 2)          # noqa: E731
    i = torch.arange(S, device="cuda")
    P = torch.exp(hm(q) @ hm(k).transpose(-1, -2) * d ** -0.5 - lse[0].double()[..., None])
    P = torch.where(i[None, :] <= i[:, None], P, torch.zeros_like(P))
    ref = (P.transpose(-1, -2) @ hm(G)).permute(1, 0, 2).reshape(S, Hkv * d)
    err = nmax(one, ref)
    print(f"dv bf16 d={d} S={S} Hkv={Hkv}: 8-wave grid bitwise the 4-wave grid; vs fp64 {err:.3e} (CUs: {torch.cuda.get_device_properties(0).multi_processor_count})")
    assert err < DV_TOL[dt] and L.lib.lrp_attn_bwd_dv_ok(1, d)


def _act64(g, act):
    return {"silu": F.silu(g), "gelu_tanh": F.gelu(g, approximate="tanh"), "gelu": F.gelu(g), "tanh": torch.tanh(g)}[act]


@pytest.mark.parametrize("I", [64, 224])          # 2 x GATED_IL; 7 blocks: off every larger grid
@pytest.mark.parametrize("M", [1, 3, 130])
@pytest.mark.parametrize("act", ["silu", "gelu_tanh", "gelu", "tanh"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gated_cp_bwd_il(ops, dtype, act, M, I):
    IL = ops.GATED_IL
    assert I % IL == 0
    g, u, Gm = rnd(M, I, dtype=dtype, seed=1), rnd(M, I, dtype=dtype, seed=2), rnd(M, I, dtype=dtype, seed=3)
    gu = torch.stack((g.view(M, I // IL, IL), u.view(M, I // IL, IL)), 2).reshape(M, 2 * I).contiguous()
    Agu = torch.full_like(gu, float("nan"))
    ops.gated_cp_bwd_il(Gm, gu, Agu, act)
    A = Agu.view(M, I // IL, 2, IL)
    assert (A[:, :, 0] == 0).all() and not torch.signbit(A[:, :, 0]).any()                 # gate slots: +0 bitwise
    ref = _act64(g.double(), act) * Gm.double()
    err = nmax(A[:, :, 1].reshape(M, I), ref)
    print(f"gated_cp {dtype} {act} M={M} I={I}: {err:.3e}")
    assert err < EW_TOL[dtype]
