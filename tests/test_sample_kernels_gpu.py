"""GPU: lrp_sample_rows / ops.sample_rows (csrc/sample.hip) against the fp64 restatement of its definition
(tests/sample_oracle.py).  Inputs are seeded and tiny: at most three rows per launch."""
import numpy as np
import pytest
import torch

from tests import sample_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda"
U_MAX = float(np.float32(1) - np.float32(2.0 ** -24))          # the largest float below 1
VS = (1, 2, 63, 64, 65, 257, 1000, 5000, 8193)
LAYOUTS = ("contig", "pitch", "offset")
# each filter alone, all three together, none; T in {0.05, 0.7, 1.0, 5.0}
SETTINGS = (dict(temperature=0.7), dict(temperature=0.7, top_k=20), dict(temperature=0.7, top_p=0.8), dict(temperature=0.7, min_p=0.05),
            dict(temperature=1.0, top_k=20, top_p=0.8, min_p=0.02), dict(temperature=0.05, top_p=0.95), dict(temperature=5.0, top_k=20, top_p=0.95),
            dict(temperature=1.0, top_k=50))
MARGIN = 1e-4
# |sample_logprob - fp64 oracle| <= LP_FACTOR x LP_FP32 x max(1, |logprob|).  LP_FP32 is the largest such normalised distance of the fp32
# evaluation of the oracle from its fp64 evaluation over the cases of this file (measured on the CPU over cases(V), V in VS, and the rows of
# test_large_vocabulary, where it is largest: the fp32 oracle's running sum over 128256 entries)
LP_FP32, LP_FACTOR = 7.3e-5, 2.0
# 99.9 % quantiles of chi-square, degrees of freedom 1 .. 30
CHI2_999 = (10.828, 13.816, 16.266, 18.467, 20.515, 22.458, 24.322, 26.124, 27.877, 29.588, 31.264, 32.909, 34.528, 36.123, 37.697, 39.252, 40.79,
            42.312, 43.82, 45.315, 46.797, 48.268, 49.728, 51.179, 52.62, 54.052, 55.476, 56.892, 58.301, 59.703)


def make_rows(V, B, seed, first_kind=0):
    """fp32 [B, V]: row b is of kind (first_kind + b) % 3 -- 3 randn; the same with 30 % of the entries at -inf (one finite entry at least);
    the same rounded to multiples of 0.25 (ties everywhere, across the k-th place too)"""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    for b in range(B):
        kind = (first_kind + b) % 3
        if kind == 1:
            hole = rng.random(V) < 0.3
            hole[rng.integers(V)] = False
            x[b, hole] = -np.inf
        elif kind == 2:
            x[b] = np.round(x[b] * 4) / 4
    return x


def place(x, layout):
    """rows on the device: contiguous; with a pitch > V on the 16-byte grid; or from a base 4 bytes off that grid with an odd pitch.  Every
    element of the buffer outside the rows is poison (NaN and 3e38 alternating): read, it would win the maximum or the select"""
    B, V = x.shape
    if layout == "contig":
        return torch.from_numpy(x).to(DEV)
    ld, off = ((V + 3) // 4 * 4 + 8, 0) if layout == "pitch" else (V + 5, 1)
    buf = torch.full((off + B * ld + 3,), float("nan"), device=DEV)
    buf[1::2] = 3e38
    t = buf[off: off + B * ld].view(B, ld)[:, :V]
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == (4 * off) % 16 and t.stride(1) == 1
    return t


def cases(V):
    """the launches of the grid at vocabulary V: (x [B, V], layout, setting, u [B] or None, seeds [B], streams [B], step)"""
    rng, out, n = np.random.default_rng(1000 + V), [], 0
    for B in (1, 3):
        for li, layout in enumerate(LAYOUTS):
            for si, kw in enumerate(SETTINGS):
                x = make_rows(V, B, seed=7919 * V + 31 * B + si, first_kind=n)
                u = rng.random(B).astype(np.float32).clip(0, U_MAX)
                if (n + n // 8) % 8 == 0:
                    u[0] = 0.0
                if (n + n // 8) % 8 == 4:
                    u[0] = U_MAX
                seeds = [int(s) for s in rng.integers(0, 2 ** 63, B)]
                out.append((x, layout, kw, u, None, None, 0))
                out.append((x, LAYOUTS[(li + 1) % 3], kw, None, seeds, [int(s) for s in rng.integers(0, 1000, B)], n % 5))
                n += 1
    return out


def run(x, layout, kw, u, seeds, streams, step):
    import lxt_amd.ops as ops
    t = lambda v, d: None if v is None else torch.tensor(v, dtype=d, device=DEV)          # noqa: E731
    got = ops.sample_rows(place(x, layout), seeds=t(seeds, torch.int64), streams=t(streams, torch.int32), step=step,
                          u=None if u is None else torch.from_numpy(u).to(DEV), **kw)
    return [g.cpu().numpy() for g in got]


def check_against_oracle(all_cases):
    """-> (cases, cases left out as near a boundary).  Every case: idx in the oracle's kept set; away from a boundary: token and n_kept equal,
    sample_logprob within the stated tolerance"""
    total = near = 0
    for x, layout, kw, u, seeds, streams, step in all_cases:
        idx, slp, nk, u_out = run(x, layout, kw, u, seeds, streams, step)
        want_u = u if u is not None else np.array([so.uniform(s, step, st) for s, st in zip(seeds, streams)], dtype=np.float32)
        assert u_out.dtype == np.float32 and np.array_equal(u_out, want_u), (layout, kw, step)
        for b, ref in enumerate(so.sample_rows(x, want_u, margin=MARGIN, **kw)):
            total += 1
            what = (x.shape, layout, kw, b, float(want_u[b]))
            assert 0 <= idx[b] < x.shape[1], what
            if ref["near"]:
                near += 1
                continue
            assert ref["kept"][idx[b]], what
            assert idx[b] == ref["token"] and nk[b] == ref["n_kept"], (what, int(idx[b]), ref["token"], int(nk[b]), ref["n_kept"])
            assert abs(slp[b] - ref["logprob"]) <= LP_FACTOR * LP_FP32 * max(1.0, abs(ref["logprob"])), (what, float(slp[b]), ref["logprob"])
    return total, near


@pytest.mark.parametrize("V", VS)
def test_token_n_kept_and_logprob_equal_the_fp64_oracle(V):
    """The grid: B in {1, 3}, three layouts, eight settings, u given (0.0 and the largest float below 1 among them) and drawn.  A case may be
    left out when the ORACLE says it sits within 1e-4 of a boundary (sample_oracle.sample_row: near); at most 5 % of the cases may be.
    Run on the CPU beforehand over these same inputs (fp64 oracle against its own fp32 evaluation): 20 of 1728 cases are near a boundary
    (1.2 %; 5 at most for one V of 192 cases, V = 8193: 2.6 %; none of the 8 of test_large_vocabulary), most of them a given u of exactly 0.0
    or 1 - 2^-24 beside a token of mass below 1e-4; the fp32 evaluation picks the fp64 token and the fp64 n_kept in every case that is not
    near; its largest |logprob error| / max(1, |logprob|) is LP_FP32."""
    total, near = check_against_oracle(cases(V))
    print(f"[sample_rows V={V}] {total} cases, {near} near a boundary and left out")
    assert total == 192 and near <= 0.05 * total, (total, near)


def test_large_vocabulary():
    """V = 128256, B = 2: the 1024-thread kernel, 501 draw chunks, every filter; the three layouts"""
    x = make_rows(128256, 2, seed=5)
    u = np.array([0.37, 0.81], dtype=np.float32)
    cs = [(x, "contig", dict(temperature=0.7, top_k=20, top_p=0.8, min_p=0.02), u, None, None, 0),
          (x, "offset", dict(temperature=0.7, top_p=0.8), None, [3, 2 ** 40 + 5], [0, 9], 6),
          (x, "pitch", dict(temperature=0.7), u, None, None, 0), (x, "contig", dict(temperature=0.7, top_k=50), None, [11, 12], [0, 0], 1)]
    total, near = check_against_oracle(cs)
    assert total == 8 and near == 0


def test_u_is_philox4x32_10_bitwise():
    """both seed forms (one seed, streams 0 .. B - 1; a seed per row, stream 0), several steps, 64-bit seeds with a non-zero high word and
    the sign bit set"""
    import lxt_amd.ops as ops
    logits = torch.zeros(3, 5, device=DEV)
    big = [0x1234567887654321, 2 ** 63 + 12345, 7]
    for seeds, streams in (([42] * 3, [0, 1, 2]), (big, None), (big, [5, 2 ** 31 - 1, 0]), ([0] * 3, [0] * 3)):
        for step in (0, 1, 7, 2 ** 31 - 1):
            s64 = torch.tensor([((s ^ 2 ** 63) - 2 ** 63) for s in seeds], dtype=torch.int64, device=DEV)
            st = None if streams is None else torch.tensor(streams, dtype=torch.int32, device=DEV)
            u = ops.sample_rows(logits, seeds=s64, streams=st, step=step)[3].cpu().numpy()
            want = np.array([so.uniform(s, step, 0 if streams is None else streams[b]) for b, s in enumerate(seeds)], dtype=np.float32)
            assert np.array_equal(u, want), (seeds, streams, step)
    assert so.uniform(0, 0, 0) == (so.KNOWN_ANSWER_ZERO[0] >> 8) * 2.0 ** -24


def test_exact_cases():
    import lxt_amd.ops as ops
    us = torch.tensor([0.0, 0.5, U_MAX], device=DEV)
    for V in (2, 65, 257, 5000, 8193):
        x = make_rows(V, 3, seed=V)                       # kinds 0, 1, 2
        row = torch.from_numpy(x[:1]).to(DEV).expand(3, V).contiguous()          # a unique maximum (a continuous draw)
        assert (x[0] == x[0].max()).sum() == 1
        am = ops.argmax_rows(row)[0]
        for kw in (dict(top_k=1), dict(top_p=1e-9), dict(min_p=1.0), dict(top_k=1, temperature=5.0)):
            idx, slp, nk, _ = ops.sample_rows(row, u=us, **kw)
            assert torch.equal(idx, am) and nk.tolist() == [1, 1, 1] and slp.tolist() == [0.0, 0.0, 0.0], (V, kw)
        # top_k = 1 on rows with tied maxima: the arg-max's lowest index whatever u, the tie group kept whole
        tied = np.round(x[2:3] * 2) / 2
        tied[0, [V // 3, V - 1]] = tied[0].max()
        t = torch.from_numpy(np.repeat(tied, 3, 0)).to(DEV)
        idx, _, nk, _ = ops.sample_rows(t, u=us, top_k=1)
        assert torch.equal(idx, ops.argmax_rows(t)[0]) and nk.tolist() == [int((tied[0] == tied[0].max()).sum())] * 3 and nk[0] >= 2, V
        # n_kept under top-k alone is an exact count: ties across the k-th place, -inf entries (k beyond the finite ones keeps them all)
        xs = torch.from_numpy(x).to(DEV)
        for k in (1, 2, 20, V // 2, V - 1, V, V + 5):
            if k < 1:
                continue
            nk = ops.sample_rows(xs, u=us, top_k=k, temperature=0.7)[2]
            want = [so.sample_row(x[b], 0.5, top_k=k, temperature=0.7)["n_kept"] for b in range(3)]
            assert nk.tolist() == want, (V, k)
    for kw in SETTINGS:
        idx, slp, nk, _ = ops.sample_rows(torch.tensor([[-3.5]] * 3, device=DEV), u=us, **kw)
        assert idx.tolist() == [0, 0, 0] and nk.tolist() == [1, 1, 1] and slp.tolist() == [0.0, 0.0, 0.0]


def test_determinism_and_row_independence():
    import lxt_amd.ops as ops
    kw = dict(temperature=0.7, top_k=20, top_p=0.8, min_p=0.02)
    for V in (257, 5000, 8193):
        x = make_rows(V, 3, seed=3 * V)
        seeds = torch.tensor([5, 2 ** 40 + 1, -9], dtype=torch.int64, device=DEV)
        for step in (0, 3):
            ref = ops.sample_rows(place(x, "contig"), seeds=seeds, step=step, **kw)
            again = ops.sample_rows(place(x, "contig"), seeds=seeds, step=step, **kw)
            for layout in ("pitch", "offset"):          # a larger pitch, another alignment, poison beyond V: the same bits
                other = ops.sample_rows(place(x, layout), seeds=seeds, step=step, **kw)
                assert all(torch.equal(a, b) for a, b in zip(ref, other)), (V, layout)
            assert all(torch.equal(a, b) for a, b in zip(ref, again)), V
            for b in range(3):                          # a row alone: the row inside the batch (a seed per row, stream 0)
                alone = ops.sample_rows(place(x[b:b + 1], "contig"), seeds=seeds[b:b + 1], step=step, **kw)
                assert all(torch.equal(a[b:b + 1], o) for a, o in zip(ref, alone)), (V, b)


DIST = dict(temperature=0.7, top_k=20, top_p=0.9)
DIST_SEED, DIST_STREAMS, DIST_STEPS = 20240607, 128, 160


def dist_row():
    return (1.5 * np.random.default_rng(64).standard_normal(64)).astype(np.float32)


def test_distribution_of_20480_draws():
    """one row of V = 64 over 128 streams x 160 steps at T = 0.7, top_k = 20, top_p = 0.9: nothing outside the oracle's kept set is ever drawn,
    and Pearson's chi-square of the counts against the oracle's probabilities lies below the 99.9 % quantile.  The seed is fixed, so this is
    one deterministic number: the same draws made on the CPU (the Python Philox through the oracle) gave chi-square 2.20 at 7 degrees of
    freedom (quantile 24.322)."""
    import lxt_amd.ops as ops
    row = dist_row()
    ref = so.sample_row(row, 0.5, **DIST)
    x = torch.from_numpy(row)[None].expand(DIST_STREAMS, 64).contiguous().to(DEV)
    seeds = torch.full((DIST_STREAMS,), DIST_SEED, dtype=torch.int64, device=DEV)
    streams = torch.arange(DIST_STREAMS, dtype=torch.int32, device=DEV)
    draws = torch.stack([ops.sample_rows(x, seeds=seeds, streams=streams, step=t, **DIST)[0] for t in range(DIST_STEPS)])
    counts = np.bincount(draws.cpu().numpy().ravel(), minlength=64)
    assert counts.sum() == 20480 and not counts[~ref["kept"]].any()
    expect = 20480 * ref["probs"][ref["kept"]]
    chi2, dof = float(((counts[ref["kept"]] - expect) ** 2 / expect).sum()), int(ref["kept"].sum()) - 1
    print(f"[sample_rows distribution] chi-square {chi2:.2f} at {dof} degrees of freedom (99.9 %: {CHI2_999[dof - 1]})")
    assert expect.min() >= 5 and chi2 < CHI2_999[dof - 1], (chi2, dof)
