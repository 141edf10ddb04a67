"""GPU parity of the encoder-family row and element-wise kernels (csrc/rowops.hip, csrc/eltwise.hip: LayerNorm, the stand-alone activations,
softmax on materialised rows, add_bcast, eps_scale / eps_scale2d / mul / add2 / cast, readout, head_seed) against the fp64 references of
tests/rowops_ref.py (themselves checked on the CPU by tests/test_rowops_ref_cpu.py), at the edges of their dispatch:

  * the 16-byte vector kernel and the scalar one (ragged widths, and tensors whose base is off the 16-byte grid: `unaligned` below);
  * 64- and 256-thread row blocks on both sides of H / EPC = 64, rows that need several and uneven passes of the block;
  * the grid cap of the element-wise kernels (2048 blocks x 256 threads: a second trip of the grid-stride loop) and their scalar tail launch;
  * strided 2-D views, in-place calls, both storage types, every activation, inv_temp != 1, the tails where exp overflows and tanh saturates.

Bars: TOL of tests/test_kernels_gpu.py (fp32 2e-5, bf16 2e-2: storage rounding) for forwards, 5 x TOL for the rule backwards; row-wise results
also hold 4 x the bar in EVERY row normalised by that row's own maximum, so that a wrong row of small values cannot hide behind the global
maximum.  Outputs the wrappers accept are NaN-guarded views: nothing outside the result may be written.  Every check prints its observed error
next to its bar.
"""
import pytest
import torch

from tests import rowops_ref as R

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}
DTYPES = [torch.float32, torch.bfloat16]
PAD = 64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.ops as o
    return o


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).cuda()


def uni(*shape, dtype=torch.float32, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) + shift).to(dtype).cuda()


def f64(x):
    return x.double()


def off_grid(x):
    """the same values in a contiguous view whose base is one element off the 16-byte grid: the dispatcher has to take the scalar kernel"""
    if x is None:
        return None
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    v = buf[1: 1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def place(unaligned, *ts):
    return tuple(off_grid(x) for x in ts) if unaligned else ts


class Guard:
    """an output view inside a NaN-filled buffer with >= 64 spare elements on each side (one more in front when the view is to sit off the 16-byte
    grid); untouched() asserts that every spare element is still NaN"""

    def __init__(self, shape, dtype, unaligned=False):
        n = 1
        for s in shape:
            n *= s
        self.lead, self.n = PAD + (1 if unaligned else 0), n
        self.buf = torch.full((self.lead + n + PAD,), float("nan"), dtype=dtype, device="cuda")
        self.out = self.buf[self.lead: self.lead + n].view(shape)
        assert (self.out.data_ptr() % 16 != 0) == bool(unaligned)

    def untouched(self):
        assert bool(torch.isnan(self.buf[: self.lead]).all()) and bool(torch.isnan(self.buf[self.lead + self.n:]).all()), "wrote outside the output"


class Guard2d:
    """a [rows, cols] column slice at column `col0` of a NaN-filled [rows, pitch] buffer, itself inside 64 spare NaN elements on each side"""

    def __init__(self, rows, cols, pitch, col0, dtype, fill=None):
        self.buf = torch.full((PAD + rows * pitch + PAD,), float("nan"), dtype=dtype, device="cuda")
        self.wide = self.buf[PAD: PAD + rows * pitch].view(rows, pitch)
        self.view = self.wide[:, col0: col0 + cols]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[PAD: PAD + rows * pitch].view(rows, pitch)[:, col0: col0 + cols] = False
        if fill is not None:
            self.view.copy_(fill)

    def untouched(self):
        assert bool(torch.isnan(self.buf[self.mask]).all()), "wrote outside the column slice"


def nerr(out, ref):
    """normalised max error max|out - ref| / max|ref| (tests/util.nmax, on the device)"""
    return float((out.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(name, out, ref, bar, rows=False):
    """finite; normalised max error below bar; rows: and max_row|out - ref| <= 4 bar max_row|ref| in every row whose reference is not all zero"""
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert bool(torch.isfinite(out).all()), name
    e = nerr(out, ref)
    msg = f"  {name}: max err / max|ref| = {e:.2e} (bar {bar:.0e})"
    ok = e < bar
    if rows:
        err, top = (out.double() - ref).abs().amax(-1), ref.abs().amax(-1)
        nz = top > 0
        worst = float((err[nz] / top[nz]).max()) if bool(nz.any()) else 0.0
        msg += f"; worst row err / row max = {worst:.2e} (bar {4 * bar:.0e})"
        ok = ok and bool((err[nz] <= 4 * bar * top[nz]).all())
    print(msg)
    assert ok, msg
    return e


# ------------------------------------------------------------------------------------------------------------------------- A. LayerNorm
LN_SHAPES = [(3, 48, False), (4, 37, False), (5, 101, False), (3, 512, False), (3, 520, False), (130, 768, False), (4, 1152, False),
             (3, 3080, False), (2, 4104, False), (4, 768, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,H,unaligned", LN_SHAPES)
def test_layernorm(ops, dtype, M, H, unaligned):
    """vector and scalar kernels, 64 / 256 threads on both sides of H / EPC = 64, one to five (uneven) passes over the row; a mean that
    matters (x = 1.5 randn + 0.7); forward with and without affine, the rule backward without stabiliser (y = None), with eps_y on the
    kernel's own y, without w; the full VJP from the forward's mean / rstd against autograd"""
    eps = 1e-6
    x, Gy = rnd(M, H, dtype=dtype, seed=1, scale=1.5, shift=0.7), rnd(M, H, dtype=dtype, seed=2)
    w, b = uni(H, dtype=dtype, seed=3, shift=0.5), rnd(H, dtype=dtype, seed=4)
    x, Gy, w, b = place(unaligned, x, Gy, w, b)
    tag = f"layernorm [{M}, {H}] {'off-grid ' if unaligned else ''}{str(dtype)[6:]}"
    fwd, bwd = TOL[dtype], 5 * TOL[dtype]

    y, mean, rstd = ops.layernorm_fwd(x, w, b, eps)
    check(f"{tag} fwd", y, R.layernorm_fwd(x, w, b, eps), fwd, rows=True)
    mean64, rstd64 = R.layernorm_stats(x, eps)
    assert mean.dtype == rstd.dtype == torch.float32
    check(f"{tag} mean", mean, mean64, 1e-5)
    check(f"{tag} rstd", rstd, rstd64, 1e-5)
    y0, mean0, rstd0 = ops.layernorm_fwd(x, None, None, eps)
    check(f"{tag} fwd, no affine", y0, R.layernorm_fwd(x, None, None, eps), fwd, rows=True)
    assert torch.equal(mean0, mean) and torch.equal(rstd0, rstd)

    check(f"{tag} bwd eps_y=0", ops.layernorm_bwd(Gy, None, w, rstd, 0.0), R.layernorm_bwd(Gy, None, w, x, eps, 0.0), bwd, rows=True)
    check(f"{tag} bwd eps_y=1e-6", ops.layernorm_bwd(Gy, y, w, rstd, 1e-6), R.layernorm_bwd(Gy, y, w, x, eps, 1e-6), bwd, rows=True)
    check(f"{tag} bwd no w", ops.layernorm_bwd(Gy, None, None, rstd, 0.0), R.layernorm_bwd(Gy, None, None, x, eps, 0.0), bwd, rows=True)

    for ww, name in ((w, "w"), (None, "no w")):
        g = Guard((M, H), dtype, unaligned)
        out = ops.layernorm_bwd_plain(Gy, x, ww, mean, rstd, out=g.out)
        assert out.data_ptr() == g.out.data_ptr()
        check(f"{tag} bwd_plain {name}", out, R.layernorm_bwd_plain(Gy, x, ww, eps), bwd, rows=True)
        g.untouched()

    # a centred Gy leaves mean_row(u) at 1/sqrt(H) of the result: inside the bf16 bar, so a backward that lost the term would pass.  Once more
    # with a gradient whose row mean is as large as the result
    Gm, = place(unaligned, rnd(M, H, dtype=dtype, seed=5, scale=0.5, shift=2.0))
    check(f"{tag} bwd eps_y=0, mean(Gy) = 2", ops.layernorm_bwd(Gm, None, w, rstd, 0.0), R.layernorm_bwd(Gm, None, w, x, eps, 0.0), bwd, rows=True)
    check(f"{tag} bwd_plain, mean(Gy) = 2", ops.layernorm_bwd_plain(Gm, x, w, mean, rstd), R.layernorm_bwd_plain(Gm, x, w, eps), bwd, rows=True)


# ----------------------------------------------------------------------------------------------------------------------- B. activations
def _act_inputs(n, dtype, unaligned):
    k = min(n, len(R.SPECIALS))
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3
    x[:k] = torch.tensor(R.SPECIALS[:k])
    Gy = torch.randn(n, generator=g)
    x, Gy = place(unaligned, x.to(dtype).cuda(), Gy.to(dtype).cuda())
    return x, Gy, k


def _check_act(name, out, ref, k, bar):
    """the planted specials and the random body apart, each with its own normaliser"""
    assert out.shape == ref.shape
    check(f"{name} specials", out[:k], ref[:k], bar)
    if out.numel() > k:
        check(f"{name} body", out[k:], ref[k:], bar)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("n,unaligned", [(1, False), (37, False), (4099, False), (100003, False), (100003, True)])
def test_activations(ops, dtype, act, n, unaligned):
    """act_fwd, act_bwd (eps_g = 1e-10 and 0) and act_grad of all four activations: tail-only, ragged, vector body + scalar tail and off-grid
    sizes; a planted head 0, +-1e-3, +-0.5, +-8, +-20, +-90 (exp overflows, tanh / erf saturate) that has to stay finite.

    bf16 act_bwd: the kernel rounds its fp32 act(x) to bf16 where the reference rounds the fp64 value; a one-ulp difference (2^-8 relative
    on that element) is legitimate and inside the bar.  silu(-90) is -7e-38 in fp64 and -0.0 in the kernel: fine under the normalised metric"""
    x, Gy, k = _act_inputs(n, dtype, unaligned)
    tag = f"{act} n={n} {'off-grid ' if unaligned else ''}{str(dtype)[6:]}"
    _check_act(f"act_fwd {tag}", ops.act_fwd(x, act), R.act_fwd(x, act), k, TOL[dtype])
    for eps_g in (1e-10, 0.0):
        Gx = ops.act_bwd(Gy, x, act, eps_g)
        _check_act(f"act_bwd eps_g={eps_g:g} {tag}", Gx, R.act_bwd(Gy, x, act, eps_g), k, 5 * TOL[dtype])
        assert float(x[0]) == 0.0 and float(Gx[0]) == 0.0              # x + eps_g == 0 -> exactly 0; act(0) / 1e-10 = 0 as well
    g = Guard((n,), dtype, unaligned)
    out = ops.act_grad(Gy, x, act, out=g.out)
    _check_act(f"act_grad {tag}", out, R.act_grad(Gy, x, act), k, TOL[dtype])
    g.untouched()


# --------------------------------------------------------------------------------------------------------------------------- C. softmax
SM_ROWS = {12: 2, 64: 3, 65: 4, 257: 5, 1000: 3, 5000: 2}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inv_temp", [1.0, 0.37, 128 ** -0.5])
@pytest.mark.parametrize("n", sorted(SM_ROWS))
def test_softmax_rows(ops, dtype, n, inv_temp):
    """64 threads (n <= 64), 256 threads in one pass (65, 257: a ragged last wave) and in several (1000, 5000); a temperature; -inf masks,
    and a row that sees one entry only (p = 1: per-row normalisers, or it would set the bar for every other row)"""
    rows = SM_ROWS[n]
    x, Rp = rnd(rows, n, dtype=dtype, seed=n, scale=3.0), rnd(rows, n, dtype=dtype, seed=n + 1)
    x[:, 3::7] = float("-inf")
    x[0, 1:] = float("-inf")
    masked = torch.isneginf(x)
    assert bool((~masked).any(-1).all())
    tag = f"[{rows}, {n}] 1/T={inv_temp:.3g} {str(dtype)[6:]}"

    p = ops.softmax_fwd(x, inv_temp)
    check(f"softmax_fwd {tag}", p, R.softmax_fwd(x, inv_temp), TOL[dtype], rows=True)
    assert bool((p[masked] == 0).all())
    dev = float((f64(p).sum(-1) - 1).abs().max())
    sbar = 1e-5 if dtype == torch.float32 else 1e-2
    print(f"  softmax_fwd {tag}: max |row sum - 1| = {dev:.2e} (bar {sbar:.0e})")
    assert dev < sbar

    Rx = ops.softmax_rule_bwd(x, p, Rp, inv_temp)
    check(f"softmax_rule_bwd {tag}", Rx, R.softmax_rule_bwd(x, p, Rp, inv_temp), 5 * TOL[dtype], rows=True)
    assert bool((Rx[masked] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------- D. add_bcast
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,H,period", [(12, 48, 1), (12, 48, 4), (12, 48, 12), (15, 101, 5), (6000, 768, 200)])
def test_add_bcast(ops, dtype, M, H, period):
    """a row vector, per-position rows, a full residual sum; the scalar kernel; more vector chunks than 2048 x 256 threads (a second trip of
    the grid-stride loop); into a guarded output and in place.  One exact fp32 add and one round-to-nearest-even: bit for bit"""
    x, y = rnd(M, H, dtype=dtype, seed=1), rnd(period, H, dtype=dtype, seed=2)
    ref = R.add_bcast(x, y)
    g = Guard((M, H), dtype)
    out = ops.add_bcast(x, y, out=g.out)
    print(f"  add_bcast [{M}, {H}] period {period} {str(dtype)[6:]}: {int((out != ref).sum())} elements differ (bar 0)")
    assert torch.equal(out, ref)
    g.untouched()
    g = Guard((M, H), dtype)
    g.out.copy_(x)
    out = ops.add_bcast(g.out, y, out=g.out)
    assert out.data_ptr() == g.out.data_ptr() and torch.equal(out, ref)
    g.untouched()


# ----------------------------------------------------------------------------------------------------------------------- E. eps_scale2d
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,pitch,col0", [(7, 96, 160, 16), (7, 100, 136, 16), (5, 96, 101, 3), (300, 768, 2304 + 64, 768)])
def test_eps_scale2d(ops, dtype, rows, cols, pitch, col0):
    """g, z and out are column slices of wider NaN-filled buffers (row pitch != width): the vector kernel, the scalar one by width (bf16:
    100 % 8 != 0) and by an odd pitch, the BERT k slice of a fused qkv buffer; both modes; the engines' in-place exact doubling"""
    g0 = rnd(rows, cols, dtype=dtype, seed=1)
    sign = torch.where(rnd(rows, cols, seed=2) < 0, -1.0, 1.0)
    z0 = (uni(rows, cols, seed=3, shift=0.1) * sign).to(dtype)           # |z| >= 0.1: away from the pole z = -eps / c
    g, z = Guard2d(rows, cols, pitch, col0, dtype, g0), Guard2d(rows, cols, pitch, col0, dtype, z0)
    tag = f"[{rows}, {cols}] pitch {pitch} {str(dtype)[6:]}"
    for relevance in (False, True):
        for c, eps in ((1.0, 1e-6), (2.0, 1e-8), (1.0, 0.0)):
            o = Guard2d(rows, cols, pitch, col0, dtype)
            ops.eps_scale2d(g.view, z.view, o.view, c, eps, relevance=relevance)
            check(f"eps_scale2d {tag} mode {int(relevance)} c={c:g} eps={eps:g}", o.view, R.eps_scale(g0, z0, c, eps, relevance), TOL[dtype])
            o.untouched()
    a = Guard2d(rows, cols, pitch, col0, dtype, g0)
    ops.eps_scale2d(a.view, a.view, a.view, 0.5, 0.0)
    print(f"  eps_scale2d {tag} in place, c = 0.5, eps = 0: {int((a.view != 2 * g0).sum())} elements differ from 2 a (bar 0)")
    assert torch.equal(a.view, 2 * g0)
    a.untouched()
    g.untouched()
    z.untouched()


# ------------------------------------------------------------------------------------------------ F. grid-stride second trip and the tail
BIG = 2 ** 22 + 2 ** 17 + 3          # more 16-byte chunks than 2048 blocks x 256 threads in fp32 (1081344) and bf16 (540672), + 3 tail elements
LAST = 2 ** 17 + 3                   # what only the second trip of the grid-stride loop and the tail launch write


def _check_big(name, out, ref, bar):
    assert out.shape == ref.shape == (BIG,)
    check(name, out, ref, bar)
    check(f"{name}, last {LAST}", out[-LAST:], ref[-LAST:], bar)


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_kernels_past_the_grid_cap(ops, dtype):
    """eps_scale (both modes), mul, add2_rule_bwd (with and without Rb), act_fwd / act_bwd / act_grad (erf-GELU) and cast at n = 2^22 + 2^17 + 3;
    the bars of test_eps_scale_mul_add2 and of the activation test; the last 2^17 + 3 elements once more on their own"""
    assert BIG // (16 // 2) > 2048 * 256 and BIG % 8 == 3 and BIG % 4 == 3
    tol = TOL[dtype]
    g = rnd(BIG, dtype=dtype, seed=1)
    sign = torch.where(rnd(BIG, seed=2) < 0, -1.0, 1.0)
    z = (uni(BIG, seed=3, shift=0.1) * sign).to(dtype)
    tag = str(dtype)[6:]
    for c, eps in ((1.0, 1e-6), (2.0, 1e-8), (1.0, 0.0)):
        gd = Guard((BIG,), dtype)
        _check_big(f"eps_scale {tag} c={c:g} eps={eps:g}", ops.eps_scale(g, z, c, eps, out=gd.out), R.eps_scale(g, z, c, eps), tol)
        gd.untouched()
    gd = Guard((BIG,), dtype)
    _check_big(f"eps_scale {tag} relevance", ops.eps_scale(g, z, 2.0, 1e-3, relevance=True, out=gd.out), R.eps_scale(g, z, 2.0, 1e-3, True), tol)
    gd.untouched()
    gd = Guard((BIG,), dtype)
    _check_big(f"mul {tag}", ops.mul(g, z, out=gd.out), R.mul(g, z), tol)
    gd.untouched()
    # summands of one sign: a + b + eps stays away from zero, so the normaliser is not a pole's
    a, b = uni(BIG, dtype=dtype, seed=4, shift=0.1), uni(BIG, dtype=dtype, seed=5, shift=0.1)
    Ra64, Rb64 = R.add2_rule_bwd(a, b, g, 1e-6)
    Ra, Rb = ops.add2_rule_bwd(a, b, g, 1e-6)
    _check_big(f"add2_rule_bwd {tag} Ra", Ra, Ra64, 50 * tol)
    _check_big(f"add2_rule_bwd {tag} Rb", Rb, Rb64, 50 * tol)
    Ra1, none = ops.add2_rule_bwd(a, b, g, 1e-6, need_b=False)
    assert none is None and torch.equal(Ra1, Ra)
    x = rnd(BIG, dtype=dtype, seed=6, scale=3.0)
    _check_big(f"act_fwd gelu {tag}", ops.act_fwd(x, "gelu"), R.act_fwd(x, "gelu"), tol)
    _check_big(f"act_bwd gelu {tag}", ops.act_bwd(g, x, "gelu", 1e-10), R.act_bwd(g, x, "gelu", 1e-10), 5 * tol)
    gd = Guard((BIG,), dtype)
    _check_big(f"act_grad gelu {tag}", ops.act_grad(g, x, "gelu", out=gd.out), R.act_grad(g, x, "gelu"), tol)
    gd.untouched()
    other = torch.bfloat16 if dtype == torch.float32 else torch.float32
    xc = ops.cast(x, other)
    print(f"  cast {tag} -> {str(other)[6:]}: {int((xc != x.to(other)).sum())} elements differ (bar 0)")
    assert xc.dtype == other and torch.equal(xc, x.to(other)) and torch.equal(xc[-LAST:], x.to(other)[-LAST:])


# ---------------------------------------------------------------------------------------------------------------- G. readout, head_seed
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("M,H", [(50, 264), (9, 101)])
def test_readout(ops, dtype, M, H, unaligned):
    """vector kernel at 256 threads with an idle tail of the block (264 / EPC = 66 or 33 chunks), scalar kernel by width and by base address"""
    e, G = place(unaligned, rnd(M, H, dtype=dtype, seed=1), rnd(M, H, dtype=dtype, seed=2))
    g = Guard((M,), torch.float32)
    out = ops.readout(e, G, out=g.out)
    assert out.dtype == torch.float32
    check(f"readout [{M}, {H}] {'off-grid ' if unaligned else ''}{str(dtype)[6:]}", out, R.readout(e, G),
          1e-5 if dtype == torch.float32 else TOL[dtype])
    g.untouched()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("eps_lin", [0.0, 1e-8])
@pytest.mark.parametrize("w_offset", [0.0, 1.0])
@pytest.mark.parametrize("H", [264, 101])
def test_head_seed(ops, dtype, H, w_offset, eps_lin):
    B, V = 3, 1000
    W, wn = rnd(V, H, dtype=dtype, seed=4), rnd(H, dtype=dtype, seed=5)
    logits, rstd = rnd(B, V, seed=3, scale=4.0), uni(B, seed=6, shift=0.5)
    idx = torch.tensor([5, V - 1, 0], dtype=torch.int32, device="cuda")
    g = Guard((B, H), dtype)
    out = ops.head_seed(W, logits, idx, wn, rstd, g.out, w_offset, eps_lin)
    check(f"head_seed H={H} w_offset={w_offset:g} eps_lin={eps_lin:g} {str(dtype)[6:]}", out,
          R.head_seed(W, logits, idx, wn, rstd, w_offset, eps_lin), TOL[dtype], rows=True)
    g.untouched()
