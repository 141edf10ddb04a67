"""GPU: lrp_token_hist_init / lrp_logit_penalty (include/lrp_hip_penalty.h) against the numpy restatement of the header
(tests/penalty_oracle.py): out is BITWISE the fp32 oracle and hist equals the oracle's table after the init and after a sequence of calls,
at every vector / tail / unaligned placement, with poison around the rows and in the pitch padding that must stay untouched."""
import numpy as np
import pytest
import torch

from tests import penalty_oracle as po

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
VS = (1, 2, 63, 64, 65, 257, 1000, 5000, 8193)
PLACEMENTS = ("contiguous", "pitched", "off16")
SETTINGS = dict(repetition=dict(rp=1.3), presence=dict(pp=0.7), frequency=dict(fp=0.3), all_bias=dict(rp=1.1, pp=0.5, fp=0.25, bias=True),
                bias_only=dict(bias=True))
BIG = 2 ** 24 + 1          # a count that fp32 cannot hold: (float)c rounds
GUARD = 64


def placed(B, V, placement, dtype, poison):
    """-> (flat poisoned buffer, [B, V] view into it, bool mask of the view's elements in flat).  contiguous: pitch V; pitched: the next
    multiple of 4 above V, plus 4 (on the 16-byte grid, with padding); off16: pitch V + 3 and the base 4 bytes off the 16-byte grid"""
    ld, off = {"contiguous": (V, 0), "pitched": ((V + 3) // 4 * 4 + 4, 0), "off16": (V + 3, 1)}[placement]
    off += GUARD
    flat = torch.full((off + B * ld + GUARD,), poison, dtype=dtype, device=DEV)
    view = flat.as_strided((B, V), (ld, 1), off)
    mask = torch.zeros_like(flat, dtype=torch.bool)
    mask.as_strided((B, V), (ld, 1), off).fill_(True)
    assert view.data_ptr() % 16 == (4 if placement == "off16" else 0)
    return flat, view, mask


def bits(t):
    return t.contiguous().view(torch.int32)


def untouched(flat, before, mask, what):
    assert torch.equal(bits(flat)[~mask], bits(before)[~mask]), f"{what}: poison outside the rows was overwritten"


def make_case(V, B, seed):
    """logits with -inf, +0, -0 and exact integers among them; a prompt with pads before lo, ids outside [0, V) and a repeated id; bias with a
    banned column"""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    for val in (-np.inf, 0.0, -0.0):
        x[rng.random((B, V)) < 0.08] = val
    S = 7
    ids = rng.integers(0, V, (B, S)).astype(np.int64)
    ids[:, 4] = ids[:, 5]
    ids[0, 6] = V                      # out of range: skipped
    if B > 1:
        ids[1, 3], ids[2, 6] = -1, 2 ** 40 + 3
    lo = np.array([2, 0, 6][:B], np.int32)
    # the special entries sit on columns the prompt (from lo on) holds, where V allows: penalised -inf / 0 / -0
    for b in range(B):
        live = [int(j) for j in ids[b, lo[b]:] if 0 <= j < V]
        for j, val in zip(live, (-np.inf, -0.0, 0.0)):
            x[b, j] = val
    bias = rng.standard_normal(V).astype(np.float32)
    bias[rng.integers(0, V)] = -np.inf
    return x, ids, lo, bias


def lasts(ids, lo, V, B):
    """the `last` of four consecutive calls: none; a prompt column (then both in the prompt and generated) ; the same again for row 0 and
    out-of-range values for the others; a fresh column"""
    first = np.array([ids[b, 5] for b in range(B)], np.int32)
    second = first.copy()
    second[1:] = [V, -1][: B - 1]
    third = np.array([(int(first[b]) + 1) % V for b in range(B)], np.int32)
    return [None, first, second, third]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("V", VS)
def test_out_is_the_oracle_bitwise_and_hist_is_the_oracles_table(V, B, placement, setting):
    import lxt_amd.ops as ops
    kw = dict(SETTINGS[setting])
    x, ids, lo, bias = make_case(V, B, seed=V * 131 + B * 7 + PLACEMENTS.index(placement))
    bias = bias if kw.pop("bias", False) else None
    okw = dict(rp=kw.get("rp", 1.0), pp=kw.get("pp", 0.0), fp=kw.get("fp", 0.0), bias=bias)
    gkw = dict(repetition_penalty=okw["rp"], presence_penalty=okw["pp"], frequency_penalty=okw["fp"],
               bias=None if bias is None else torch.from_numpy(bias).to(DEV))

    lf, lv, lm = placed(B, V, placement, torch.float32, 3e38)
    of, ov, om = placed(B, V, placement, torch.float32, float("nan"))
    hf, hv, hm = placed(B, V, placement, torch.int32, 0x7F7F7F7F)
    lv.copy_(torch.from_numpy(x))
    l0, o0, h0 = lf.clone(), of.clone(), hf.clone()

    # the table of the prompt: pads before lo are no history, ids outside [0, V) are skipped
    ids_d = torch.full((B, ids.shape[1] + 3), 5, dtype=torch.int64, device=DEV)[:, 1:-2]          # (a pitched ids view)
    ids_d.copy_(torch.from_numpy(ids))
    got = ops.token_hist_init(ids_d, torch.from_numpy(lo).to(DEV), V, hist=hv)
    hist = po.hist_init(ids, lo, V)
    assert got.data_ptr() == hv.data_ptr() and np.array_equal(hv.cpu().numpy(), hist)
    untouched(hf, h0, hm, "hist after init")
    if V > 2:          # a count above 2^24, preset on a column the sequence below does not feed
        jb = (int(ids[0, 5]) + 2) % V
        hist[0, jb] = (hist[0, jb] & po.SEEN) | BIG
        hv[0, jb] = int(hist[0, jb])

    for n, last in enumerate(lasts(ids, lo, V, B)):
        want = po.step(x, hist, last, **okw)
        out = ops.logit_penalty(lv, hv, None if last is None else torch.from_numpy(last).to(DEV), out=ov, **gkw)
        assert out.data_ptr() == ov.data_ptr()
        g = ov.cpu().numpy()
        assert np.array_equal(g.view(np.int32), want.view(np.int32)), (n, np.argwhere(g.view(np.int32) != want.view(np.int32))[:4].tolist())
        assert np.array_equal(hv.cpu().numpy(), hist), n
        assert np.array_equal(np.isneginf(g) & np.isneginf(x), np.isneginf(x)), "-inf logits stay -inf"
        if bias is not None:
            assert np.isneginf(g[:, np.isneginf(bias)]).all(), "a banned column is -inf"
    assert (hist[0] < 0).any() and ((hist & po.CMAX) > 0).any() and (V < 3 or (hist[(hist & po.CMAX) > 0] < 0).any())
    untouched(lf, l0, torch.zeros_like(lm), "logits (read-only)")
    untouched(of, o0, om, "out")
    untouched(hf, h0, hm, "hist")

    # twice the same bits (no `last`: the table stands), and a row alone equals the row inside the batch
    a = ops.logit_penalty(lv, hv, out=ov, **gkw).clone()
    b = ops.logit_penalty(lv, hv, **gkw)
    assert torch.equal(bits(a), bits(b)) and np.array_equal(hv.cpu().numpy(), hist)
    r = B - 1
    alone = ops.logit_penalty(lv[r:r + 1].contiguous(), hv[r:r + 1].contiguous(), **gkw)
    assert torch.equal(bits(alone[0]), bits(a[r]))


def test_hist_init_without_lo_and_into_a_fresh_table():
    import lxt_amd.ops as ops
    V = 300
    ids = np.array([[5, 5, 299, 300, -1, 0], [7, 8, 9, 10, 11, 12]], np.int64)
    got = ops.token_hist_init(torch.from_numpy(ids).to(DEV), None, V)
    assert got.shape == (2, V) and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), po.hist_init(ids, None, V))
    assert int((got != 0).sum()) == 3 + 6
    # a table that held another call's history is zeroed first
    again = ops.token_hist_init(torch.from_numpy(ids[:, :2]).to(DEV), None, V, hist=got)
    assert np.array_equal(again.cpu().numpy(), po.hist_init(ids[:, :2], None, V))


def test_a_128k_vocabulary_row():
    import lxt_amd.ops as ops
    V, B = 128256, 3
    x, ids, lo, bias = make_case(V, B, seed=99)
    hist = po.hist_init(ids, lo, V)
    rng = np.random.default_rng(3)
    gen = rng.integers(0, V, 4000)
    np.add.at(hist[0], gen, 1)
    np.add.at(hist[1], gen[:50], 1)
    hist[1, V - 1] = po.SEEN | BIG
    last = np.array([V - 1, int(ids[1, 5]), V], np.int32)
    hv = torch.from_numpy(hist.copy()).to(DEV)
    okw = dict(rp=1.1, pp=0.5, fp=0.25, bias=bias)
    want = po.step(x, hist, last, **okw)
    out = ops.logit_penalty(torch.from_numpy(x).to(DEV), hv, torch.from_numpy(last).to(DEV), repetition_penalty=1.1, presence_penalty=0.5,
                            frequency_penalty=0.25, bias=torch.from_numpy(bias).to(DEV))
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)) and np.array_equal(hv.cpu().numpy(), hist)
