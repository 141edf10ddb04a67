"""The element-wise bounds of tests/rowsite_bound.py, checked without a GPU:

  (a) the header's formula and the trace's fp64 value agree, and the torch model of each kernel's arithmetic (fp32, storage round trips exactly
      where the kernel stores) stays within every bound on every element of every case of the GPU test that is not past a grid cap;
  (b) each planted structural fault leaves the bound on every output it touches -- next to whether the bars tests/test_kernels_gpu.py holds
      today (one nmax per output, x 1 / 5 / 20 / 50) would have passed it;
  (c) the signed-bias statistic separates truncating bf16 stores from round-to-nearest;
  (d) the shapes of tests/test_rowsite_bound_gpu.py reach the paths and trip counts they claim: the host rules mirrored in rowsite_bound, held
      against the library's own lrp_sandwich_norm_ok where it exports the rule.  No device is touched.
"""
import math

import pytest
import torch

from tests import rowsite_bound as rb

BF16, F32 = rb.BF16, rb.F32
DT = {"bf16": BF16, "fp32": F32}


def _small_cases(dtype, family):
    return [c for c in rb.cases(dtype, family) if not c[3]["big"]]


@pytest.mark.parametrize("family", rb.FAMILIES)
@pytest.mark.parametrize("dt", list(DT))
def test_model_is_within_every_bound(dt, family):
    dtype, worst = DT[dt], {}
    for tag, op, kw, place in _small_cases(dtype, family):
        d = rb.operands(op, dtype, **kw)
        tr, hd = rb.TRACES[op](rb.Ctx(dtype), d), rb.header(op, d)
        for n, t in tr.items():          # the trace's value IS the header's formula
            ref = hd[n]
            fin = torch.isfinite(ref) & torch.isfinite(t.v)
            assert bool((fin | (torch.isnan(ref) == torch.isnan(t.v))).all()), (tag, n)
            dev = float(((t.v - ref).abs()[fin] / (ref.abs()[fin] + 1e-300)).max()) if bool(fin.any()) else 0.0
            assert dev < 1e-9 or float((t.v - ref).abs()[fin].max()) <= 1e-13 * float(ref.abs()[fin].max()), (tag, n, dev)
        out = rb.model(op, d)
        log = rb.evaluate(op, d, out, strict=True, tag=f"{tag} ")
        assert len(log) == len(out)
        for n, share in rb.excluded(op, d).items():
            assert share <= rb.EXCLUDED_CAP, (tag, n, share)
        for n, r in log.items():
            key = f"{op} {n.split()[-1]}"
            worst[key] = max(worst.get(key, 0.0), r)
        # the truncating model differs only where something is rounded to bf16
        if dtype == F32:
            bad = rb.model(op, d, rnd=rb.trunc)
            assert all(torch.equal(torch.nan_to_num(out[n]), torch.nan_to_num(bad[n])) for n in out)
    print(f"model {family} {dt}: worst err / bound per output: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_planted_zeros_are_asserted():
    """the zeros the module's docstring promises sit inside the `zero` masks the GPU test asserts: zero rows, g = 0, g = -eps_g (fp32), z = 0 under a
    stabiliser, the gate slots of the CP form"""
    for dtype in (BF16, F32):
        d = rb.operands("add_rmsnorm_fwd", dtype, M=5, H=96, w_off=1.0)
        R = rb.references("add_rmsnorm_fwd", d)
        assert bool(R["y"][2][d["zero_row"]].all()) and bool(R["hsum"][2][d["zero_row"]].all()) and not bool(R["y"][2][0].any())
        d = rb.operands("rmsnorm_bwd_add2", dtype, M=5, H=96, w_off=0.0, subset="rxhbl", eps_add=1e-8, eps_lin=1e-8)
        R = rb.references("rmsnorm_bwd_add2", d)
        assert bool(R["Gs"][2][d["zero_row"]].all()) and bool(R["rel"][2][d["zero_row"]].all())
        assert bool(R["Gs"][2][0, 48]) and bool(R["A"][2][0, 48])          # hsum = 0 under eps_add: 0 / eps
        d = rb.operands("gated_bwd", dtype, M=5, I=96, act="silu", eps_g=1e-8, eps_lin=1e-8)
        R = rb.references("gated_bwd", d)
        assert bool(R["Ag"][2][0, 0]) and bool(R["Au"][2][0, 0]) and bool(R["Ag"][2][d["g"].shape[0] // 2].all())
        assert bool(R["Ag"][2][0, 1]) == (dtype == F32)                      # g = -eps_g: representable in fp32 storage only
        R = rb.references("gated_cp", rb.operands("gated_cp", dtype, M=5, I=96, act="silu"))
        assert bool(R["Ag"][2].all())
        d = rb.operands("rope_bwd", dtype, rows=79, nh=3, d=16, seq=37, eps_rope=1e-8, eps_lin=1e-8)
        assert bool(rb.references("rope_bwd", d)["A"][2][0, 0, 1])          # x = 0 under eps_lin
        d = rb.operands("qkv_bwd_pack", dtype, rows=79, nq=4, nk=1, d=64, seq=37, w_off=1.0)
        assert all(bool(v[2][78].all()) for v in rb.references("qkv_bwd_pack", d).values())


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------
def _fault_case(op, dtype):
    W = rb.epc(dtype)
    kw = {"add_rmsnorm_fwd": dict(M=5, H=257 * W, w_off=1.0), "rmsnorm_bwd_add2": dict(M=5, H=65 * W, w_off=1.0, subset="rx", eps_add=0.0, eps_lin=0.0),
          "head_rmsnorm_fwd": dict(rows=7, heads=3, d=16 * W, w_off=1.0), "head_rmsnorm_bwd": dict(rows=7, heads=3, d=16 * W, w_off=1.0),
          "rope_fwd": dict(rows=79, nh=3, d=64, seq=37), "rope_bwd": dict(rows=79, nh=3, d=64, seq=37, eps_rope=0.0, eps_lin=0.0),
          "gated_fwd": dict(M=5, I=96, act="silu"), "gated_bwd": dict(M=5, I=96, act="silu", eps_g=1e-10, eps_lin=0.0),
          "sandwich_fwd": dict(M=5, H=672 * W, w_off=1.0), "sandwich_bwd": dict(M=5, H=300 * W, w_off=1.0),
          "qk_norm_rope": dict(rows=79, nq=4, nk=2, d=64, seq=37, w_off=1.0), "qkv_bwd_pack": dict(rows=79, nq=4, nk=2, d=64, seq=37, w_off=1.0),
          "gqa_reduce_rope": dict(rows=79, nh=2, rep=4, d=64, seq=37)}[op]
    return rb.operands(op, dtype, **kw)


ON_SMALL = ("rstd_neighbour", "rope_pos")          # planted on the rows / heads that carry the scale 2^-6


def test_planted_faults_leave_the_bound():
    passed_today = []
    print("fault @ op dtype: err / bound per touched output | today's nmax against its bar")
    for fault, ops in rb.FAULTS.items():
        for op, touched in ops.items():
            for dt, dtype in DT.items():
                d = _fault_case(op, dtype)
                out, clean, R = rb.model(op, d, fault=fault), rb.model(op, d), rb.references(op, d)
                ratios = {n: rb.evaluate(op, d, out, strict=False, only=(n,))[n] for n in touched}
                bars = {n: rb.todays_bars(out[n], R[n][0], rb.TODAY[op], dtype) for n in touched}
                through = all(b[0] for b in bars.values())
                print(f"  {fault:15s} @ {op:17s} {dt}: " + " ".join(f"{n} {r:.3g}" for n, r in ratios.items()) + " | "
                      + " ".join(f"{n} {b[1]:.2e}" for n, b in bars.items()) + f" (x{rb.TODAY[op]}) | today's bars: {'PASS (missed)' if through else 'caught'}")
                for n, r in ratios.items():
                    assert r > 1.0, (fault, op, dt, n, r)
                    assert rb.todays_bars(clean[n], R[n][0], rb.TODAY[op], dtype)[0], (op, n)
                if through and fault in ON_SMALL:
                    passed_today.append((fault, op, dt))
    assert passed_today, "no structural fault on 2^-6-scaled values passes today's bars: the premise of these tests is gone"
    print("missed by today's bars on small values:", passed_today)


def test_planted_values_are_small():
    """the rows the faults of ON_SMALL sit on carry about 2^-6 of the output's maximum"""
    for op, n, pick in (("add_rmsnorm_fwd", "hsum", lambda t, d: t[d["small"]]), ("rope_fwd", "xr", lambda t, d: t[37:39])):
        d = _fault_case(op, BF16)
        ref = rb.references(op, d)[n][0]
        share = float(pick(ref, d).abs().max() / ref.abs().max())
        assert 2.0 ** -9 < share < 2.0 ** -4, (op, share)


@pytest.mark.parametrize("dt", list(DT))
def test_a_skipped_second_trip_and_a_truncating_store_leave_the_bound(dt):
    """a grid-stride kernel that stops after its first trip leaves the tail of its output as the buffer held it (NaN in the GPU test's guards):
    planted on a small case by shrinking the grid to 2 blocks; and one truncated store of a value that is not representable is outside u"""
    dtype = DT[dt]
    for op, kw, n in (("gated_fwd", dict(M=130, I=96, act="silu"), "m"), ("rope_fwd", dict(rows=79, nh=3, d=64, seq=37), "xr"),
                      ("head_rmsnorm_bwd", dict(rows=77, heads=3, d=16 * rb.epc(dtype), w_off=1.0), "out"),
                      ("sandwich_bwd", dict(M=130, H=8 * rb.epc(dtype), w_off=1.0), "Gs")):
        d = rb.operands(op, dtype, **kw)
        out = rb.model(op, d)
        flat = out[n].reshape(-1).clone()
        first_trip = 2 * 256 * rb.epc(dtype)
        assert flat.numel() > first_trip
        flat[first_trip:] = math.nan
        r = rb.evaluate(op, d, {n: flat.reshape(out[n].shape)}, strict=False, only=(n,))[n]
        print(f"  second trip skipped @ {op} {dt}: {n} {r:.3g}")
        assert r > 1.0
        if dtype == BF16:
            bad = rb.model(op, d, rnd=rb.trunc)
            r = rb.evaluate(op, d, bad, strict=False, only=(n,))[n]
            print(f"  truncating store @ {op} {dt}: {n} {r:.3g}")
            assert r > 1.0


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------
BIAS_CASES = [("add_rmsnorm_fwd", dict(M=130, H=520, w_off=1.0), ("y", "hsum")), ("rmsnorm_bwd_add2", dict(M=130, H=520, w_off=0.0, subset="rx", eps_add=0.0, eps_lin=0.0), ("Gs",)),
              ("head_rmsnorm_fwd", dict(rows=77, heads=3, d=128, w_off=1.0), ("y",)), ("rope_fwd", dict(rows=79, nh=3, d=128, seq=37), ("xr",)),
              ("rope_bwd", dict(rows=79, nh=3, d=128, seq=37, eps_rope=0.0, eps_lin=0.0), ("A",)), ("gated_fwd", dict(M=130, I=96, act="silu"), ("m",)),
              ("gated_bwd", dict(M=130, I=96, act="silu", eps_g=1e-10, eps_lin=0.0), ("Ag", "Au")), ("add2", dict(n=4099, eps=1e-8), ("Ra", "Rb")),
              ("sandwich_fwd", dict(M=30, H=2400, w_off=1.0), ("y", "hsum")), ("sandwich_bwd", dict(M=30, H=2400, w_off=1.0), ("Gs", "Ga")),
              ("qk_norm_rope", dict(rows=79, nq=4, nk=1, d=64, seq=37, w_off=1.0), ("qr", "kr")),
              ("qkv_bwd_pack", dict(rows=79, nq=4, nk=1, d=64, seq=37, w_off=1.0), ("Aq", "Ak", "Av")),
              ("gqa_reduce_rope", dict(rows=79, nh=2, rep=4, d=64, seq=37), ("out",))]


@pytest.mark.parametrize("op,kw,names", BIAS_CASES, ids=[c[0] for c in BIAS_CASES])
def test_bias_tells_truncation(op, kw, names):
    d = rb.operands(op, BF16, **kw)
    assert rb.bias_case(op, d)
    good, bad, R = rb.model(op, d), rb.model(op, d, rnd=rb.trunc), rb.references(op, d)
    for n in names:
        b_rne, b_trunc = (rb.signed_bias(rb.bias_view(op, t[n]), rb.bias_view(op, R[n][0])) for t in (good, bad))
        print(f"  {op} {n}: bias rne {b_rne:+.3f} u, trunc {b_trunc:+.3f} u")
        assert b_trunc < -0.25 and abs(b_rne) <= 0.5 * abs(b_trunc), (op, n, b_rne, b_trunc)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------
def test_shapes_reach_what_they_claim():
    import lxt_amd._lib as L
    lib = L.lib
    code = {BF16: L.BF16, F32: L.F32}
    for dtype in (BF16, F32):
        W = rb.epc(dtype)
        # row norms: vector / scalar kernel, 64 / 256 threads on both sides of H / EPC = 64 | 65, passes and the uneven last pass
        seen = set()
        for k, M, off in rb.ROW_WIDTHS:
            H = -k if k < 0 else k * W
            w, nt, passes, uneven = rb.row_plan(H, dtype, aligned=not off)
            if off:
                assert (w, nt) == (1, 256) and H % W == 0          # an aligned width: only the base address sends it to the scalar kernel
            else:
                assert (w == W, nt, passes, uneven) == rb.ROW_REACH[k], (k, w, nt, passes, uneven)
            seen.add(M)
        assert seen == {1, 3, 130}
        assert rb.row_threads(64 * W, W) == 64 and rb.row_threads(65 * W, W) == 256
        # per-head norms: every lane-group size, one block / several blocks, the capped grid's second trip for exactly one group
        assert sorted({k for _, _, k in rb.HEAD_CASES}) == [1, 2, 16, 64] and {h for _, h, _ in rb.HEAD_CASES} == {1, 3}
        for rows, heads, k in rb.HEAD_CASES:
            assert rb.head_shape_ok(k * W, dtype)
            lpg, nb, trips = rb.group_plan(rows * heads, k * W, dtype, 8192)
            assert lpg == k and trips == 1
        rows, heads, k = rb.HEAD_BIG
        lpg, nb, trips = rb.group_plan(rows * heads, k * W, dtype, 8192)
        assert (lpg, nb, trips) == (64, 8192, 2) and rows * heads == 8192 * (256 // 64) + 1
        assert not rb.head_shape_ok(3 * W, dtype) and not rb.head_shape_ok(128 * W, dtype)
        # RoPE and the gated kernels: vector / scalar, one trip / two
        for tag, op, kw, place in rb.cases(dtype, "rope") + rb.cases(dtype, "gated") + rb.cases(dtype, "add2"):
            if op in ("rope_fwd", "rope_bwd", "gqa_reduce_rope"):
                vec = (kw["d"] // 2) % W == 0 and not place["off"] and place["pad"] % W == 0
                work = kw["rows"] * kw["nh"] * (kw["d"] // 2)
            elif op == "add2":
                vec, work = not place["off"], kw["n"] // W * W if not place["off"] else kw["n"]
            else:
                vec = kw["I"] % W == 0 and not place["off"] and place["pad"] % W == 0
                work = kw["M"] * kw["I"]
            w, g, trips = rb.elt_plan(work, dtype, vec)
            if place["big"]:
                assert vec and g == 2048 and trips == 2 and work // W - 2048 * 256 <= 1024, (tag, g, trips, work)
            else:
                assert trips == 1 or (op == "add2" and kw["n"] < W and trips == 0), (tag, trips)          # (n < EPC: the tail launch alone)
            if "pad3" in tag or tag.endswith("-pad") or "-pad-" in tag or "-off" in tag or "I25" in tag:
                assert not vec, tag
        assert [(dd // 2) % W == 0 for dd in (8, 24)] == ([False, False] if dtype == BF16 else [True, True])
        assert rb.grid_for(2048 * 256) == 2048 and rb.grid_for(2048 * 256 + 1) == 2048 and rb.grid_for(1) == 1
        # sandwich: the chunks-per-thread choice, the gate's edge, the backward's cap
        for k in rb.SANDWICH_K:
            H = k * W
            nt, need, ch, idle = rb.sandwich_chunks(H, dtype)
            assert (nt, need, ch) == rb.SANDWICH_REACH[k], (k, nt, need, ch)
            assert rb.sandwich_ok(H, dtype) and lib.lrp_sandwich_norm_ok(H, code[dtype]) == 1
            assert idle == (k in (8, 200, 300, 672, 1000))
        H = rb.SANDWICH_NO * W
        assert not rb.sandwich_ok(H, dtype) and lib.lrp_sandwich_norm_ok(H, code[dtype]) == 0
        for H in range(1, 1100 * W, 7):
            assert rb.sandwich_ok(H, dtype) == bool(lib.lrp_sandwich_norm_ok(H, code[dtype])), H
        if dtype == BF16:
            assert 5376 == 672 * W and 8192 == 1024 * W
        big = rb.past_cap("sandwich_bwd", dtype)
        assert rb.sandwich_bwd_plan(big["M"], big["H"], dtype) == (16384, 2) and rb.sandwich_bwd_plan(big["M"] - 1, big["H"], dtype) == (16384, 1)
        # q / k site kernels
        for dd, nq, nk in rb.QK_CASES:
            assert rb.head_shape_ok(dd, dtype, least=2) and nq % nk == 0
            for heads in (nq + nk, nq + 2 * nk):
                assert rb.group_plan(rb.QK_ROWS * heads, dd, dtype, 16384)[2] == 1
        assert sorted({nq // nk for _, nq, nk in rb.QK_CASES}) == [1, 4, 8]
        big = rb.past_cap("qk", dtype)
        for heads in (5, 6):
            lpg, nb, trips = rb.group_plan(big["rows"] * heads, big["d"], dtype, 16384)
            assert (nb, trips) == (16384, 2), (heads, nb, trips)
        assert rb.group_plan((big["rows"] - 1) * 5, big["d"], dtype, 16384)[2] == 1
    assert rb.QK_ROWS % rb.QK_SEQ and rb.ROPE_ROWS % rb.ROPE_SEQ          # rows are no multiple of seq
    assert set(rb.GATED_I) == {32, 96, 1024}
    # the interleaved gated entries refuse a row of gu / Agu shorter than 2 I before any launch (no pointer is read on the host)
    ptr, M, I = 4096, 4, 64
    for c in code.values():
        assert lib.lrp_gated_act_fwd_il(ptr, ptr, M, I, 2 * I - 8, I, 0, c, None) == -3 and lib.lrp_gated_act_fwd_il(ptr, ptr, M, I, 2 * I, I - 8, 0, c, None) == -3
        assert lib.lrp_gated_act_bwd_il(ptr, ptr, ptr, M, I, I, 2 * I - 8, 2 * I, 1e-10, 0.0, 0, c, None) == -3
        assert lib.lrp_gated_act_bwd_il(ptr, ptr, ptr, M, I, I, 2 * I, 2 * I - 8, 1e-10, 0.0, 0, c, None) == -3
        assert lib.lrp_gated_act_bwd_il(ptr, ptr, ptr, M, I, I - 8, 2 * I, 2 * I, 1e-10, 0.0, 0, c, None) == -3
        assert lib.lrp_gated_cp_bwd_il(ptr, ptr, ptr, M, I, I, 2 * I - 8, 2 * I, 0, c, None) == -3
    # the LEAN switch of csrc/eltwise.hip:219 sits between the stabiliser settings
    assert [eg >= 1e-30 and el == 0.0 for eg, el in rb.STABS] == [True, False, False]
