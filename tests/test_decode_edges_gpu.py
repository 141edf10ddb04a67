"""GPU: lrp_attn_decode (csrc/decode.hip) at the edges of its dispatch, which the other decode tests do not reach: every <T, NC, RT>
instantiation, partial head tiles, partial vectors, more than 64 live slabs, pitched operands, a caller-owned workspace full of stale NaN, and
the engine's decode path at GQA ratios 3, 7 and 2.  Method of test_decode_kernels_gpu.py: operands rounded to the storage type, every cache row
outside [lo[b], n - 1] NaN, fp64 softmax attention on the CPU as the reference, max |o - ref| / max |ref| against the project's bars
(tests/decode_ref.py), and the bitwise properties with torch.equal.

Host dispatch: rep = Hq / Hkv, RT = 8 if rep >= 5, 4 if rep >= 3, else rep; ntile = ceil(rep / RT); the last tile serves nlive = rep - (ntile
- 1) RT heads.  NC = vectors of 16 bytes per lane of a key row: nch = d / (16 / sizeof(T)) vectors on 16 lanes, NC = 1 (nch <= 16), 2 (<= 32),
4 (fp32 only).  Which case of test_every_instantiation_partial_tiles_and_partial_vectors reaches which of the 20 instantiations:

    fp32  <1,1> d40 h3kv3     <1,2> d8 h4kv2      <1,4> d24 h6kv2      <1,8> d64 h18kv2, d32 h18kv3
          <2,1> d80 h2kv2     <2,2> d72 h4kv2     <2,4> d104 h8kv2     <2,8> d96 h14kv2, d128 h24kv2
          <4,1> d136 h2kv2    <4,2> d200 h4kv2    <4,4> d160 h8kv2     <4,8> d192 h10kv2, d256 h16kv2
    bf16  <1,1> d40 h3kv3     <1,2> d8 h4kv2, d64 h4kv2                <1,4> d80 h6kv2
          <1,8> d96 h14kv2, d128 h32kv2           <2,1> d136 h2kv2     <2,2> d200 h4kv2
          <2,4> d160 h6kv2    <2,8> d192 h10kv2, d256 h16kv2, d256 h12kv1
"""
import pytest
import torch

from tests.decode_ref import BAR, DEV, DTYPES, bits, live_rows, poisoned_cache, reference
from tests.util import nmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import lxt_amd.ops as ops
    return ops


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def check_case(ops, dname, Hq, Hkv, d, n, lo_l, seed):
    """one (shape, live length, lo) at cap = n and cap = n + SLAB + 3: the result is finite (no poisoned row reached it), a repeated call is
    bit-equal, it is under the bar against fp64 at cap = n, each prompt alone equals its row of the batch, and it does not depend on cap
    -> the error against fp64"""
    dtype, s, B, scale = DTYPES[dname], ops.ATTN_DECODE_SLAB, len(lo_l), d ** -0.5
    q, k, v = live_rows(dtype, B, n, Hq, Hkv, d, seed)
    q, lo, pos = q.to(DEV), i32(lo_l), i32([n - 1])
    what = f"{dname} d={d} Hq/Hkv={Hq}/{Hkv} n={n} lo={lo_l}"
    outs, err = {}, None
    for cap in (n, n + s + 3):
        kc, vc = poisoned_cache(k, cap, lo_l), poisoned_cache(v, cap, lo_l)
        o = ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale)
        assert bool(torch.isfinite(o).all()), f"{what} cap={cap}: a poisoned cache row reached the result"
        assert torch.equal(o, ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale)), f"{what} cap={cap}: a repeated call differs"
        outs[cap] = o
        if cap == n:
            ref = reference(q, kc, vc, lo_l, n, Hq, Hkv, d, scale)
            err = float((o.double().cpu() - ref).abs().max() / ref.abs().max())
            assert err <= BAR[dname], f"{what}: {err:.3e} > {BAR[dname]:.3e}"
            for b in range(B if B > 1 else 0):          # prompt b alone == its row of the batch
                ob = ops.attn_decode(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], lo[b:b + 1].clone(), pos, Hq, Hkv, d, scale)
                assert torch.equal(ob[0], o[b]), f"{what}: prompt {b} alone differs from its row in the batch"
    assert torch.equal(outs[n], outs[n + s + 3]), f"{what}: the result depends on cap"
    return err


# ---- 1. every instantiation, partial head tiles, partial vectors ------------------------------------------------------------------------
EVERY = [
    # dtype, d, Hq, Hkv        ratio, what the case is there to reach
    ("fp32", 8, 4, 2),       # 2: <1,2>, two live lanes per key
    ("fp32", 24, 6, 2),      # 3: <1,4>, nlive 3
    ("fp32", 72, 4, 2),      # 2: <2,2>, second vector on 2 of 16 lanes
    ("fp32", 96, 14, 2),     # 7: <2,8>, nlive 7
    ("fp32", 128, 24, 2),    # 12: <2,8>, two tiles, 8 + 4
    ("fp32", 136, 2, 2),     # 1: <4,1>, third vector on 2 lanes, fourth empty
    ("fp32", 192, 10, 2),    # 5: <4,8>, nlive 5
    ("fp32", 256, 16, 2),    # 8: <4,8>, full
    ("fp32", 64, 18, 2),     # 9: <1,8>, two tiles, 8 + 1
    ("fp32", 32, 18, 3),     # 6: <1,8>, nlive 6, odd Hkv
    ("fp32", 40, 3, 3),      # 1: <1,1>, 10 live lanes, odd Hkv
    ("fp32", 80, 2, 2),      # 1: <2,1>, second vector on 4 lanes
    ("fp32", 104, 8, 2),     # 4: <2,4>, full tile, second vector on 10 lanes
    ("fp32", 200, 4, 2),     # 2: <4,2>, fourth vector on 2 lanes
    ("fp32", 160, 8, 2),     # 4: <4,4>, third vector on 8 lanes, fourth empty
    ("bf16", 8, 4, 2),       # 2: <1,2>, one live lane
    ("bf16", 64, 4, 2),      # 2: <1,2>
    ("bf16", 80, 6, 2),      # 3: <1,4>, nlive 3
    ("bf16", 96, 14, 2),     # 7: <1,8>, nlive 7
    ("bf16", 128, 32, 2),    # 16: <1,8>, two full tiles
    ("bf16", 136, 2, 2),     # 1: <2,1>, second vector on one lane
    ("bf16", 192, 10, 2),    # 5: <2,8>, nlive 5
    ("bf16", 256, 16, 2),    # 8: <2,8>, full
    ("bf16", 256, 12, 1),    # 12: <2,8>, two tiles, 8 + 4, one kv head
    ("bf16", 40, 3, 3),      # 1: <1,1>, 5 live lanes, odd Hkv
    ("bf16", 200, 4, 2),     # 2: <2,2>, second vector on 9 lanes
    ("bf16", 160, 6, 2),     # 3: <2,4>, nlive 3, second vector on 4 lanes
]


@pytest.mark.parametrize("case", EVERY, ids=lambda c: f"{c[0]}-d{c[1]}-h{c[2]}kv{c[3]}")
def test_every_instantiation_partial_tiles_and_partial_vectors(ops, case):
    """B = 2, live lengths 1, SLAB + 1 and 3 SLAB + 5, lo all-zero and mixed, two capacities.  The table in the module docstring names the
    instantiation each case launches; between them: all 20, nlive < RT for RT = 4 (ratio 3) and RT = 8 (ratios 5, 6, 7), ntile = 2 with a full
    (ratio 16) and a partial (ratios 9, 12) last tile, a partly filled second, third and fourth vector (d / E off a multiple of 16), and
    Hkv >= 2 in all but one case, so that a wrong kvh * rep term cannot hide"""
    dname, d, Hq, Hkv = case
    s, B = ops.ATTN_DECODE_SLAB, 2
    worst = 0.0
    for n in (1, s + 1, 3 * s + 5):
        for lo_kind in ("zeros", "mixed"):
            lo_l = [0] * B if lo_kind == "zeros" else [(0, n - 1, n // 2)[b % 3] for b in range(B)]
            worst = max(worst, check_case(ops, dname, Hq, Hkv, d, n, lo_l, seed=1000 * n + d + Hq))
    print(f"attn_decode {dname} d={d} Hq/Hkv={Hq}/{Hkv}: worst max-normalised error vs fp64 {worst:.3e} (bar {BAR[dname]:.3e})")


# ---- 2. more than 64 live slabs: the combine launch's chunk loop ------------------------------------------------------------------------
def long_lives(s):
    """(lo, n) of two prompts, live slabs = (n - 1) / SLAB - lo / SLAB + 1; prompt 0 has the count the case is named after"""
    return {
        "64": ([0, s + 3], 64 * s),                                # one full chunk (prompt 1: 63)
        "65-from-slab-0": ([0, 32 * s + 1], 64 * s + 1),            # a second chunk of one slab (prompt 1: 33)
        "65-from-slab-3": ([3 * s + 7, 0], 68 * s - 2),             # the walk starts at a slab other than 0 (prompt 1: 68, second chunk of 4)
        "78": ([0, 2 * s + 1], 77 * s + 9),                         # second chunk of 14: more than 8, no multiple of 8 (prompt 1: 76, 12)
        "130": ([0, 64 * s + 63], 129 * s + 17),                    # three chunks, the last of 2 (prompt 1: 66, second chunk of 2)
    }


@pytest.mark.parametrize("slabs", ["64", "65-from-slab-0", "65-from-slab-3", "78", "130"])
@pytest.mark.parametrize("shape", [("fp32", 32, 4, 2), ("bf16", 32, 4, 2), ("bf16", 256, 10, 2)], ids=lambda c: f"{c[0]}-d{c[1]}-h{c[2]}kv{c[3]}")
def test_more_than_64_live_slabs(ops, shape, slabs):
    """the combine kernel fetches the live slabs' (m, l) 64 at a time and re-uses its LDS weights behind a barrier: 64 slabs are one chunk,
    65 a second chunk of one, 78 a second chunk that is neither <= 8 nor a multiple of 8, 130 three chunks; the same bars as at 197 keys"""
    dname, d, Hq, Hkv = shape
    s = ops.ATTN_DECODE_SLAB
    lo_l, n = long_lives(s)[slabs]
    count = (n - 1) // s - lo_l[0] // s + 1
    assert str(count) == slabs.split("-")[0]
    err = check_case(ops, dname, Hq, Hkv, d, n, lo_l, seed=n + d)
    print(f"attn_decode {dname} d={d} Hq/Hkv={Hq}/{Hkv} n={n} lo={lo_l} ({count} live slabs): max-normalised error vs fp64 {err:.3e} "
          f"(bar {BAR[dname]:.3e})")


# ---- 3. pitched operands and untouched memory -------------------------------------------------------------------------------------------
def nan_like(t):
    return torch.full_like(t, float("nan"))


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_attn_decode_pitched_operands_and_untouched_memory(ops, dname, d, B):
    """q and out: column ranges, one 16-byte vector in, of wider buffers; kc / vc: the first Hkv d columns of rows that are one vector longer;
    every byte outside the views NaN.  Bit-equal to the call on contiguous copies (ldq, ldo, ldc reach every address), and out's surrounding
    columns and both cache buffers keep their bits"""
    dtype, (Hq, Hkv), cap, n = DTYPES[dname], (6, 2), 70, 69
    epc = 16 // torch.empty(0, dtype=dtype).element_size()
    lo_l = [5, n - 1, 0][:B]
    q, k, v = live_rows(dtype, B, n, Hq, Hkv, d, seed=d + B)
    qbuf = torch.full((B, Hq * d + 3 * epc), float("nan"), dtype=dtype)
    qbuf[:, epc: epc + Hq * d] = q
    qbuf = qbuf.to(DEV)
    obuf = nan_like(qbuf)
    kbuf, vbuf = poisoned_cache(k, cap, lo_l, pad=epc), poisoned_cache(v, cap, lo_l, pad=epc)
    kbuf0, vbuf0 = kbuf.clone(), vbuf.clone()
    qv, out, kc, vc = qbuf[:, epc: epc + Hq * d], obuf[:, epc: epc + Hq * d], kbuf[:, :, : Hkv * d], vbuf[:, :, : Hkv * d]
    assert kc.stride(1) == Hkv * d + epc and not kc.is_contiguous() and qv.stride(0) == Hq * d + 3 * epc
    lo, pos, scale = i32(lo_l), i32([n - 1]), d ** -0.5
    ops.attn_decode(qv, kc, vc, lo, pos, Hq, Hkv, d, scale, out=out)
    want = ops.attn_decode(qv.contiguous(), kc.contiguous(), vc.contiguous(), lo, pos, Hq, Hkv, d, scale)
    assert bool(torch.isfinite(out).all()), "a NaN outside the views or the live rows reached the result"
    assert torch.equal(bits(out), bits(want)), "pitched operands give other bits than contiguous copies"
    err = nmax(out, reference(qv, kc, vc, lo_l, n, Hq, Hkv, d, scale))
    assert err <= BAR[dname], f"{err:.3e} > {BAR[dname]:.3e}"
    fresh = nan_like(obuf)
    assert torch.equal(bits(obuf[:, :epc]), bits(fresh[:, :epc])) and torch.equal(bits(obuf[:, epc + Hq * d:]), bits(fresh[:, epc + Hq * d:])), \
        "a column of out's buffer outside the view was written"
    assert torch.equal(bits(kbuf), bits(kbuf0)) and torch.equal(bits(vbuf), bits(vbuf0)), "a cache was written"
    print(f"attn_decode {dname} d={d} B={B} pitched: max-normalised error vs fp64 {err:.3e} (bar {BAR[dname]:.3e})")


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("kernel", ["rope", "qknorm_rope"])
def test_appends_into_pitched_caches_write_one_row(ops, kernel, dname, d, B):
    """decode_rope_append and decode_qknorm_rope_append on caches whose rows are one 16-byte vector longer than nk d, all NaN: q_rot and the
    appended row are the contiguous call's bits, every pad column and every other row keeps its sentinel"""
    dtype, (nq, nk), cap = DTYPES[dname], (6, 2), 70
    epc = 16 // torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator().manual_seed(3 * d + B)
    nqk, cols = (nq + nk) * d, nk * d
    buf = torch.randn(B, (nq + 2 * nk) * d + 3 * epc, generator=g).to(dtype).to(DEV)
    qkv = buf[:, epc: epc + (nq + 2 * nk) * d]
    wq, wk = ((torch.randn(d, generator=g) * 0.3).to(dtype).to(DEV) for _ in range(2))
    ang = torch.rand(cap, d, generator=g) * 6.0
    cos, sin = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()

    def append(pos, q_rot, kc, vc):
        if kernel == "rope":
            return ops.decode_rope_append(qkv[:, :nqk], qkv[:, nqk:], cos, sin, pos, q_rot, kc, vc, nq, nk, d)
        return ops.decode_qknorm_rope_append(qkv[:, :nqk], qkv[:, nqk:], wq, wk, 1e-6, cos, sin, pos, q_rot, kc, vc, nq, nk, d, 1.0)

    for p_ in (0, 37, cap - 1):
        pos = i32([p_])
        kbuf = torch.full((B, cap, cols + epc), float("nan"), dtype=dtype, device=DEV)
        vbuf = kbuf.clone()
        kc_c, vc_c = (torch.full((B, cap, cols), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
        q_c = append(pos, torch.zeros(B, nq * d, dtype=dtype, device=DEV), kc_c, vc_c)
        q_p = append(pos, torch.zeros(B, nq * d, dtype=dtype, device=DEV), kbuf[:, :, :cols], vbuf[:, :, :cols])
        assert bool(torch.isfinite(q_c).all()) and bool(torch.isfinite(kc_c[:, p_]).all()) and bool(torch.isfinite(vc_c[:, p_]).all())
        assert torch.equal(bits(q_p), bits(q_c)), f"q_rot differs at p={p_}"
        for name, got, cont in (("kc", kbuf, kc_c), ("vc", vbuf, vc_c)):
            want = nan_like(got)
            want[:, p_, :cols] = cont[:, p_]
            assert torch.equal(bits(got[:, p_, :cols]), bits(cont[:, p_])), f"the row appended to {name} differs at p={p_}"
            assert torch.equal(bits(got), bits(want)), f"{name}: a pad column or a row other than p={p_} was written"


# ---- 4. a workspace the caller owns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [("fp32", 64, 4, 2), ("bf16", 64, 4, 2), ("fp32", 200, 6, 2), ("bf16", 192, 10, 2)],
                         ids=lambda c: f"{c[0]}-d{c[1]}-h{c[2]}kv{c[3]}")
def test_stale_workspace_is_never_read(ops, shape):
    """the engine allocates its workspace once and never clears it: slabs below lo / SLAB and above pos / SLAB hold what earlier steps and
    layers left.  A workspace of 0xFF bytes (every float a NaN) with dead slabs on both sides of the live ones gives the bits of the call
    on the shared workspace; the 256 bytes behind attn_decode_ws stay 0xFF; and calls with other (lo, n) on the same, now partly written,
    workspace -- the slabs written before are dead now -- give the bits of a fresh one"""
    dname, d, Hq, Hkv = shape
    dtype, s, B, scale = DTYPES[dname], ops.ATTN_DECODE_SLAB, 2, d ** -0.5
    cap = 6 * s
    need = ops.attn_decode_ws(B, Hq, d, cap)
    guard = torch.full((256,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    assert bool(torch.isnan(ws[:need].view(torch.float32)).all())
    # live slabs 1..3 and 2..3 of 6; then 4..5 (the slabs written before lie below lo); then 0 alone (they lie above pos)
    for step, (lo_l, n) in enumerate((([s + 3, 2 * s], 3 * s + 5), ([4 * s + 1, 4 * s + 9], 5 * s + 2), ([0, 7], s))):
        q, k, v = live_rows(dtype, B, n, Hq, Hkv, d, seed=n + d)
        q, kc, vc, lo, pos = q.to(DEV), poisoned_cache(k, cap, lo_l), poisoned_cache(v, cap, lo_l), i32(lo_l), i32([n - 1])
        o = ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale, ws=ws)
        assert bool(torch.isfinite(o).all()), f"step {step}: a stale workspace slab or a poisoned cache row reached the result"
        assert torch.equal(o, ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale)), f"step {step}: differs from the call without ws"
        fresh = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        assert torch.equal(o, ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale, ws=fresh)), f"step {step}: differs from a fresh workspace"
        assert torch.equal(ws[need:], guard), f"step {step}: bytes behind attn_decode_ws were written"
        err = nmax(o, reference(q, kc, vc, lo_l, n, Hq, Hkv, d, scale))
        assert err <= BAR[dname], f"step {step}: {err:.3e} > {BAR[dname]:.3e}"


def test_workspace_and_shape_refusals(ops):
    """host checks, nothing is launched: a workspace one byte short, head dims off the grid of 8 or above 256, Hq no multiple of Hkv"""
    B, Hq, Hkv, d, cap = 2, 4, 2, 64, 70
    q = torch.zeros(B, Hq * d, device=DEV)
    kc = torch.zeros(B, cap, Hkv * d, device=DEV)
    lo, pos = i32([0, 0]), i32([cap - 1])
    need = ops.attn_decode_ws(B, Hq, d, cap)
    ops.attn_decode(q, kc, kc.clone(), lo, pos, Hq, Hkv, d, 0.125, ws=torch.zeros(need, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.attn_decode(q, kc, kc.clone(), lo, pos, Hq, Hkv, d, 0.125, ws=torch.zeros(need - 1, dtype=torch.uint8, device=DEV))
    for bad in (12, 264):
        with pytest.raises(ValueError):
            ops.attn_decode_ws(B, Hq, bad, cap)
    kc3 = torch.zeros(B, cap, 4 * d, device=DEV)
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
        ops.attn_decode(torch.zeros(B, 6 * d, device=DEV), kc3, kc3.clone(), lo, pos, 6, 4, d, 0.125)


# ---- 5. the engine at GQA ratios its fixtures lack ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [(12, 4, 64), (14, 2, 128), (4, 2, 128)], ids=lambda h: f"h{h[0]}kv{h[1]}d{h[2]}")
def test_engine_decode_path_equals_prefill_path_at_other_gqa_ratios(heads):
    """fp32 LlamaLRP engines of 2 layers on random weights at 12 / 4 heads of 64 (ratio 3: RT = 4 with nlive 3), 14 / 2 of 128 (ratio 7: RT = 8
    with nlive 7) and 4 / 2 of 128 (ratio 2), hidden 128, inter 256, vocabulary 512.  One left-padded generate() of 6 tokens, lengths (24, 15,
    7); the logits row of step t = 1..5 came through the cache and lrp_attn_decode, and is compared with the only logits row of a 1-token
    generate() on the first S + t columns, which comes from the prefill forward alone: whole rows within 1e-4 max-normalised, the project's
    fp32 bar for decode path against prefill path (test_generate_gpu.py, part iii).  The third engine stands for 4 / 2 heads of 96: the
    prefill's fp32 attention kernels exist for head dims 16, 32, 64, 128 and 256 only (ATT_DISPATCH_D in csrc/attention.hip returns
    LRP_ESHAPE for any other), so the forward refuses 96; 128 is the nearest it takes and launches the instantiation <float, 2, 2> that 96
    would have (the partly filled second vector at ratio 2 is the kernel test's d = 72 case above)"""
    import lxt_amd.engine as E
    nq, nk, d = heads
    H, I, V, S, T, lens = 128, 256, 512, 24, 6, (24, 15, 7)
    cfg = dict(hidden=H, inter=I, n_layers=2, n_heads=nq, n_kv=nk, head_dim=d, vocab=V, rope_theta=10000.0, rms_eps=1e-5)
    g = torch.Generator(device=DEV).manual_seed(nq + d)
    rn = lambda std, *s: torch.randn(*s, generator=g, device=DEV) * std              # noqa: E731
    nw = lambda: 1.0 + 0.1 * torch.randn(H, generator=g, device=DEV)                 # noqa: E731
    # (q and k five times wider than the rest: scores of a few units, a softmax that is far from uniform over the keys)
    W = dict(embed=rn(0.02, V, H), norm=nw(), lm_head=rn(0.02, V, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(0.1, nq * d, H), wk=rn(0.1, nk * d, H), wv=rn(0.02, nk * d, H), wo=rn(0.02, H, nq * d),
                          wg=rn(0.02, I, H), wu=rn(0.02, I, H), wd=rn(0.02, H, I)) for _ in range(2)])
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, max_seq=64, device=DEV)
    ids = torch.randint(0, V, (3, S), generator=torch.Generator().manual_seed(5))
    out = eng.generate(ids, T, lengths=lens, return_logits=True)
    assert out["logits"].shape == (3, T, V) and bool(torch.isfinite(out["logits"]).all())
    worst = 0.0
    for t in range(1, T):
        pre = eng.generate(out["sequences"][:, : S + t], 1, lengths=[n + t for n in lens], return_logits=True)
        assert pre["logits"].shape == (3, 1, V)
        err = nmax(out["logits"][:, t], pre["logits"][:, 0])
        worst = max(worst, err)
        assert err <= 1e-4, f"step {t}: decode path vs prefill path {err:.3e} > 1e-4"
    print(f"[generate fp32 {nq}/{nk} heads of {d}] decode path vs prefill path, whole logits rows: {worst:.2e} (bar 1e-4)")
