"""GPU: the dense GEMM family (lrp_gemm_nt, lrp_gemm_nn, lrp_gemm_skinny, the nine fused-epilogue entry points of the ping-pong kernel, the tail
split of ops.linear_fwd / linear_dgrad, the small-M and the weight-streaming Linears) against the element-wise bounds of tests/gemm_bound.py, through lxt_amd.ops, on the smallest shapes that reach every kernel form, tile seam and
epilogue (the big shapes, the row chunks and the 2^30 offsets stay with tests/test_kernels_gpu.py / tests/test_kernel_edges_gpu.py).
  Every case: operands are [:rows, :cols] views of wider NaN-filled storage (row pitch > K; the pad columns and two rows past the last are NaN,
  so a read past K or past M / N shows); outputs are NaN-prefilled and over-wide, and afterwards every spare column and spare row is still NaN.
  Every element goes through gemm_bound.evaluate: finite, |x - fp64 reference| <= bound, exact zeros where nothing is summed (an all-zero
  activation row, rs = 0).  The worst err / bound per output is printed next to the torch model's on the same operands; on bf16 outputs the signed
  bias must stay under half of what the truncating model shows.  Shapes that depend on the number of compute units take it from the device and
  assert the path they mean to take."""
import pytest
import torch

from tests import gemm_bound as gb

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")
    from lxt_amd import ops
    return ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pitched(t, pad=None):
    """a device tensor as the [..., :rows, :cols] view of NaN-filled storage [..., rows + 2, cols + pad] (row pitch on the 16-byte grid)"""
    e = 16 // t.element_size()
    pad = e + (-t.shape[-1]) % e if pad is None else pad
    store = torch.full((*t.shape[:-2], t.shape[-2] + 2, t.shape[-1] + pad), NAN, dtype=t.dtype, device="cuda")
    store[..., :t.shape[-2], :t.shape[-1]] = t
    return store[..., :t.shape[-2], :t.shape[-1]]


def _nan_out(rows, cols, pad, dtype, lead=()):
    store = torch.full((*lead, rows + 1, cols + pad), NAN, dtype=dtype, device="cuda")
    return store, store[..., :rows, :cols]


def _spare(name, store, rows, cols):
    assert bool(torch.isnan(store[..., cols:]).all()), f"{name}: a spare column was written"
    assert bool(torch.isnan(store[..., rows:, :]).all()), f"{name}: a row past the last was written"


def _judge(form, g, outs, label, split=None):
    """the kernel's outputs (device tensors in the output's own type) of one case: gemm_bound.evaluate, the model's ratios beside them, the bias bar"""
    x = {n: t.double() for n, t in outs.items()}
    if form == "res_ssq":
        g = dict(g, stored=outs["out"])
    print(f"[{label}]")
    log = gb.evaluate(form, g, x, split=split)
    model = gb.model(form, g)
    mlog = gb.evaluate(form, dict(g, stored=model["out"]) if form == "res_ssq" else g, model, strict=False)
    line = f"kernels / model {label}: " + " ".join(f"{n} {log[n]:.3f} / {mlog[n]:.3f}" for n in mlog)
    line += "".join(f" {n} {r:.3f}" for n, r in log.items() if "[" in n)
    if gb.bias_case(form, g):
        R = gb.references(form, g)
        bad = gb.model(form, g, rnd=gb.trunc)
        bias = {n: (gb.signed_bias(x[n], R[n][0]), 0.5 * abs(gb.signed_bias(bad[n], R[n][0]))) for n in x if n != "ssq"}
        line += " | bias / bar, in u: " + " ".join(f"{n} {b:+.3f} / {bar:.3f}" for n, (b, bar) in bias.items())
        print(line)
        for n, (b, bar) in bias.items():
            assert abs(b) <= bar, (label, n, b, bar)
    else:
        print(line)
    return log


# ---- lrp_gemm_nt: the register-staged kernel and the 32 / 64 / 128 / 256 direct-to-LDS tiles -----------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K,batch,f_bf16,f_fp32", gb.NT_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" + ("xb3" if c[3] else "") for c in gb.NT_CASES])
def test_gemm_nt_forms(ops, M, N, K, batch, f_bf16, f_fp32, dtype):
    e = 16 // dtype.itemsize
    d = gb.operands(M, N, K, dtype=dtype, seed=1, batch=batch, block=(16, 16) if M >= 48 else None, with_res=False)
    g = gb.to(d, "cuda")
    a, b = _pitched(g["A"]), _pitched(g["B"])
    assert a.stride(-2) > K and gb.nt_form(M, N, K, dtype, a.stride(-2), b.stride(-2), batch or 1) == (f_bf16 if dtype == BF16 else f_fp32)
    lead = () if batch is None else (batch,)
    for odt, with_bias in ((dtype, False), (dtype, True)) + (((F32, True),) if dtype == BF16 else ()):
        store, out = _nan_out(M, N, e, odt, lead)
        if batch is None:
            ops.gemm_nt_2d(a, b, out, g["bias"] if with_bias else None)
        else:
            assert ops.gemm_nt(a, b, g["bias"] if with_bias else None, out=out) is out
        torch.cuda.synchronize()
        _spare("out", store, M, N)
        form = f_bf16 if dtype == BF16 else f_fp32
        _judge("nt", dict(g, odt=odt, with_bias=with_bias), {"out": out},
               f"nt {form} {M}x{N}x{K}{'' if batch is None else ' batch 3'} {'bf16' if dtype == BF16 else 'fp32'}->{'bf16' if odt == BF16 else 'fp32'}{' +bias' if with_bias else ''}")


# ---- the ping-pong kernel, NT and NN: 2 .. 9 K tiles, one and two tiles per workgroup -------------------------------------------------------
@pytest.mark.parametrize("nn", [False, True], ids=["nt", "nn"])
@pytest.mark.parametrize("K", gb.PP_K)
@pytest.mark.parametrize("shape", ["one_round", "two_rounds"])
def test_ping_pong_tiles_and_seams(ops, shape, K, nn):
    cus = _cus()
    M, N = gb.pp_shapes(cus)[shape]
    tm, tn = gb.cdiv(M, 256), gb.cdiv(N, 256)
    assert (190 <= tm * tn <= cus) if shape == "one_round" else (cus < tm * tn < 2 * cus), (tm * tn, cus)
    turn, _ = gb.walk(tm, tn, cus)
    later = (turn > 0).repeat_interleave(256, 0).repeat_interleave(256, 1)[:M, :N].cuda()
    assert bool(later.any()) == (shape == "two_rounds")
    g = gb.to(gb.operands(M, N, K, nn=nn, seed=2, block=(272, 300), with_res=False), "cuda")
    a, b = _pitched(g["A"]), _pitched(g["B"])
    if nn:
        assert ops.gemm_nn_ok(a, b)
    else:
        assert gb.nt_form(M, N, K, BF16, a.stride(0), b.stride(0)) == "pp"
    for odt in (BF16, F32):
        with_bias = (odt == F32) != nn
        store, out = _nan_out(M, N, 8, odt)
        (ops.gemm_nn_2d if nn else ops.gemm_nt_2d)(a, b, out, g["bias"] if with_bias else None)
        torch.cuda.synchronize()
        _spare("out", store, M, N)
        _judge("nn" if nn else "nt", dict(g, odt=odt, with_bias=with_bias, cus=cus), {"out": out},
               f"pp {'nn' if nn else 'nt'} {shape} {M}x{N}x{K} ->{'bf16' if odt == BF16 else 'fp32'}{' +bias' if with_bias else ''}",
               split=("later tile", "first tile", later) if shape == "two_rounds" else None)


# ---- lrp_gemm_skinny: the SK form, the K splits, the slab reduction ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(gb.SKINNY_SHAPES))
@pytest.mark.parametrize("M", gb.SKINNY_M)
def test_gemm_skinny_splits_and_reduce(ops, M, shape):
    import lxt_amd._lib as L
    N, K, plan = gb.SKINNY_SHAPES[shape]
    assert N % 4 and gb.skinny_plan(M, N, K) == plan and L.lib.lrp_gemm_skinny_splits(M, N, K) == gb.skinny_splits(M, N, K)
    pad = 3 if (N + 3) % 4 else 2
    for nn in (False, True):
        g = gb.to(gb.operands(M, N, K, nn=nn, seed=3, plan=plan, with_res=False), "cuda")
        a, b = _pitched(g["A"]), _pitched(g["B"])
        assert not nn or ops.gemm_nn_ok(a, b)
        for odt in (BF16, F32):
            with_bias = (odt == F32) != nn
            store, out = _nan_out(M, N, pad, odt)
            assert out.stride(0) % 4
            ops.gemm_skinny(a, b, out, nn=nn, bias=g["bias"] if with_bias else None)
            torch.cuda.synchronize()
            _spare("out", store, M, N)
            _judge("skinny", dict(g, odt=odt, with_bias=with_bias), {"out": out},
                   f"skinny {'nn' if nn else 'nt'} {shape} M {M} N {N} K {K} splits {plan[0]} x {plan[1]} ->{'bf16' if odt == BF16 else 'fp32'}{' +bias' if with_bias else ''}")


# ---- the fused-epilogue entry points --------------------------------------------------------------------------------------------------------
from tests.test_kernels_gpu import FUSED_FORMS      # noqa: E402

PLAIN_FUSED = [f for f in FUSED_FORMS if not f.startswith("gemm_gated")]
FORM_OF = {"gemm_res_ssq": "res_ssq", "gemm_nt_rs": "nt_rs", "gemm_nt_rs_rope": "rope", "gemm_nt_rs_bias": "nt_rs_bias", "gemm_nt_rs_bias_rope": "bias_rope",
           "gemm_nn_rs": "nn_rs", "gemm_nn_rs_res": "nn_rs_res"}


def test_every_fused_form_is_covered():
    assert set(FUSED_FORMS) == set(FORM_OF) | {"gemm_gated_fwd_coef", "gemm_gated_bwd_coef"}


def _tiles_path(M, ncols, size, cus):
    tiles = gb.cdiv(M, 256) * gb.cdiv(ncols, 256)
    assert (190 <= tiles <= cus) if size in ("le", "pair") else tiles > cus, (tiles, cus)


@pytest.mark.parametrize("size", ["le", "gt"])
@pytest.mark.parametrize("K", gb.FUSED_K)
@pytest.mark.parametrize("entry", PLAIN_FUSED)
def test_fused_epilogues(ops, entry, K, size):
    cus, form = _cus(), FORM_OF[entry]
    s = gb.fused_shapes(cus)[size]
    rope, nn = form in ("rope", "bias_rope"), form.startswith("nn")
    M, N = (s["Mr"] if rope else s["M"]), s["N"]
    _tiles_path(M, N, size, cus)
    extra = {}
    if rope:
        cos, sin = gb.rope_tables(s["seq"])
        extra = dict(seq=s["seq"], rope_cols=s["rope_cols"], cos=cos, sin=sin)
    g = gb.to(gb.operands(M, N, K, nn=nn, seed=4, block=(272, 300), with_res=form in ("res_ssq", "nn_rs_res"), **extra), "cuda")
    a, b = _pitched(g["A"]), _pitched(g["B"])
    assert ops.norm_fused_ok(M, N, K, a.stride(0), b.stride(0), nn, BF16)
    store, out = _nan_out(M, N, 8, BF16)
    outs = {"out": out}
    label = f"{entry} {M}x{N}x{K} tiles {'<=' if size == 'le' else '>'} CUs"
    if form == "res_ssq":
        res = _pitched(g["res"])
        raw_store, raw = _nan_out(M, N, 16, BF16)
        ssq_store = torch.full((N // 64 + 1, M + 5), NAN, dtype=F32, device="cuda")
        ssq = ssq_store[:N // 64, :M]
        ops.gemm_res_ssq(a, b, res, out, ssq, raw=raw)
        torch.cuda.synchronize()
        _spare("raw", raw_store, M, N)
        _spare("ssq", ssq_store, N // 64, M)
        outs.update(raw=raw, ssq=ssq)
    elif form == "nt_rs":
        ops.gemm_nt_rs(a, b, g["rs"], out)
    elif form == "nn_rs":
        ops.gemm_nn_rs(a, b, g["rs"], out)
    elif form == "nt_rs_bias":
        ops.gemm_nt_rs_bias(a, b, g["rs"], g["bias"], out)
    elif form == "nn_rs_res":
        res = _pitched(g["res"])
        ops.gemm_nn_rs_res(a, b, g["rs"], res, out)
        inpl = _pitched(g["res"])
        ops.gemm_nn_rs_res(a, b, g["rs"], inpl, inpl)
        torch.cuda.synchronize()
        assert torch.equal(inpl, out), "in place on res: not the same bits"
    elif form == "rope":
        assert ops.gemm_nt_rs_rope_ok(a, b, out, s["seq"], s["rope_cols"], 128)
        ops.gemm_nt_rs_rope(a, b, g["rs"], g["cos"], g["sin"], out, s["seq"], s["rope_cols"], 128)
    else:
        assert ops.gemm_nt_rs_bias_rope_ok(a, b, out, s["seq"], s["rope_cols"], 128)
        ops.gemm_nt_rs_bias_rope(a, b, g["rs"], g["bias"], g["cos"], g["sin"], out, s["seq"], s["rope_cols"], 128)
    torch.cuda.synchronize()
    _spare("out", store, M, N)
    _judge(form, g, outs, label)


@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
@pytest.mark.parametrize("size", ["le", "gt"])
@pytest.mark.parametrize("K", gb.FUSED_K)
def test_gated_forward_coefficients(ops, K, size, act):
    cus = _cus()
    s = gb.fused_shapes(cus)[size]
    M, N = s["M"], s["N"]
    I = N // 2
    _tiles_path(M, N, size, cus)
    g = gb.to(gb.operands(M, N, K, seed=5, block=(272, 300), with_res=False, act=act), "cuda")
    a, b = _pitched(g["A"]), _pitched(g["B"])
    for eps_g, eps_lin in gb.STABS:
        for with_rs in (False, True):
            cstore, coef = _nan_out(M, N, 8, BF16)
            mstore, m = _nan_out(M, I, 16, BF16)
            ops.gemm_gated_fwd_coef(a, b, coef, m, eps_g, eps_lin, act, rs=g["rs"] if with_rs else None)
            torch.cuda.synchronize()
            _spare("coef", cstore, M, N)
            _spare("m", mstore, M, I)
            cg, cu = gb.coef_split(coef)
            _judge("gated_fwd", dict(g, eps_g=eps_g, eps_lin=eps_lin, with_rs=with_rs), {"m": m, "cg": cg, "cu": cu},
                   f"gemm_gated_fwd_coef {act} eps ({eps_g:g}, {eps_lin:g}){' rs' if with_rs else ''} {M}x{N}x{K} tiles {'<=' if size == 'le' else '>'} CUs")


@pytest.mark.parametrize("size", ["pair", "gt"])
@pytest.mark.parametrize("K", gb.FUSED_K)
def test_gated_backward_on_the_stash(ops, K, size):
    """Agu = Gm (*) coef in the NN dgrad's epilogue: on the stash the forward just wrote (pair) and on a planted one (both)"""
    cus = _cus()
    M, I = gb.gated_bwd_shapes(cus)[size]
    _tiles_path(M, I, size, cus)
    g = gb.to(gb.operands(M, I, K, nn=True, seed=6, block=(272, 300), with_res=False), "cuda")
    a, b = _pitched(g["A"]), _pitched(g["B"])
    gen = torch.Generator().manual_seed(K)
    stashes = {"planted": _pitched((0.5 * torch.randn(M, 2 * I, generator=gen)).to(BF16).cuda())}
    if size == "pair":
        f = gb.to(gb.operands(M, 2 * I, K, seed=7, with_res=False), "cuda")
        coef, m = _nan_out(M, 2 * I, 8, BF16)[1], _nan_out(M, I, 8, BF16)[1]
        ops.gemm_gated_fwd_coef(_pitched(f["A"]), _pitched(f["B"]), coef, m, 1e-10, 0.0, "silu")
        stashes["forward's"] = coef
    for name, coef in stashes.items():
        store, Agu = _nan_out(M, 2 * I, 8, BF16)
        ops.gemm_gated_bwd_coef(a, b, coef, Agu)
        torch.cuda.synchronize()
        _spare("Agu", store, M, 2 * I)
        assert bool(torch.isfinite(coef).all())
        Ag, Au = gb.il_split(Agu)
        _judge("gated_bwd", dict(g, coef=coef), {"Ag": Ag, "Au": Au}, f"gemm_gated_bwd_coef {name} stash {M}x{I}x{K} tiles {'<=' if size == 'pair' else '>'} CUs")


# ---- the tail split of ops.linear_fwd / ops.linear_dgrad ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", [False, True], ids=["linear_fwd", "linear_dgrad"])
def test_tail_split_halves_and_their_seam(ops, nn):
    """the smallest shape ops.tail_split_cols admits: 128 x 3 tiles, K = 1024 -- two tile columns through the ping-pong kernel, the third (8 columns
    wide here) through the split-K path; both halves against their own bound, the columns 511 | 512 where they meet among them"""
    M, N, K = 127 * 256 + 8, 520, 1024
    main = ops.tail_split_cols(M, N, K)
    assert main == 512
    plan = gb.skinny_plan(M, N - main, K)
    assert plan[0] > 1
    g = gb.to(gb.operands(M, N, K, nn=nn, seed=8, with_res=False), "cuda")
    a, b = _pitched(g["A"]), _pitched(g["B"])
    store, out = _nan_out(M, N, 8, BF16)
    assert (ops.linear_dgrad if nn else ops.linear_fwd)(a, b, out=out) is out
    torch.cuda.synchronize()
    _spare("out", store, M, N)
    cols = (lambda t, c: t[:, c]) if nn else (lambda t, c: t[c])
    for name, form, c, extra in (("main", "nn" if nn else "nt", slice(0, main), {}), ("tail", "skinny", slice(main, N), dict(plan=plan))):
        _judge(form, dict(g, B=cols(g["B"], c), N=c.stop - c.start, **extra), {"out": out[:, c]}, f"tail split {'linear_dgrad' if nn else 'linear_fwd'} {name} {M}x{N}x{K}")


# ---- the small-M and the weight-streaming Linears ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M", gb.SMALLM_M)
def test_linear_smallm(ops, M, dtype):
    N, K = gb.SMALLM_SHAPE
    e = 16 // dtype.itemsize
    name = "bf16" if dtype == BF16 else "fp32"
    g = gb.to(gb.operands(M, N, K, dtype=dtype, seed=9, with_res=False), "cuda")
    x, W = _pitched(g["A"]), _pitched(g["B"], 0)
    assert ops.smallm_ok(M, W, x)
    for odt, with_bias in ((dtype, False), (dtype, True)) + (((F32, True),) if dtype == BF16 else ()):
        store, out = _nan_out(M, N, e, odt)
        assert ops.linear_smallm_fwd(x, W, g["bias"] if with_bias else None, out=out) is out
        torch.cuda.synchronize()
        _spare("out", store, M, N)
        _judge("smallm_fwd", dict(g, odt=odt, with_bias=with_bias), {"out": out},
               f"linear_smallm_fwd M {M} W {N}x{K} {name}->{'bf16' if odt == BF16 else 'fp32'}{' +bias' if with_bias else ''}")
    # the dgrad: c[M, K] = s[M, N] W[N, K], s = g, g z / (z + eps) or g / (z + eps) (* x)
    g = gb.to(gb.operands(M, K, N, nn=True, dtype=dtype, seed=10, with_z=True), "cuda")
    gg, z, W = _pitched(g["A"]), _pitched(g["z"]), _pitched(g["B"], 0)
    for kind, kw in (("s = g", {}), ("s = g z / (z + eps)", dict(eps=1e-6)), ("s = g / (z + eps), * x", dict(eps=1e-6, rel_in=True, rel_out=True))):
        for odt in (dtype,) + ((F32,) if dtype == BF16 else ()):
            # (lrp_linear_smallm_dgrad takes no output pitch -- it writes out as one flat [M K] array, include/lrp_hip.h -- and W without a row
            # pitch: neither can be over-wide.  What can be shown is shown: the row behind the last one keeps its NaN)
            store = torch.full((M + 1, K), NAN, dtype=odt, device="cuda")
            out = store[:M]
            ops.linear_smallm_dgrad(gg, W, z=z if kw else None, x=g["res"] if kw.get("rel_out") else None, eps=kw.get("eps", 0.0),
                                    relevance_in=bool(kw.get("rel_in")), relevance_out=bool(kw.get("rel_out")), out=out)
            torch.cuda.synchronize()
            assert bool(torch.isnan(store[M:]).all()), "out: a row past the last was written"
            _judge("smallm_dgrad", dict(g, odt=odt, **kw), {"out": out}, f"linear_smallm_dgrad M {M} W {N}x{K} {name}->{'bf16' if odt == BF16 else 'fp32'} {kind}")


@pytest.mark.parametrize("shape", list(gb.STREAM_FWD))
@pytest.mark.parametrize("M", gb.STREAM_M)
def test_linear_stream_fwd(ops, M, shape):
    import lxt_amd._lib as L
    N, K, splits = gb.STREAM_FWD[shape]
    g = gb.to(gb.operands(M, N, K, seed=11, with_res=False, chain=K // splits, adds=splits if splits > 1 else 0), "cuda")
    x, W = _pitched(g["A"]), _pitched(g["B"])
    assert ops.linear_stream_ok(x, W) and L.lib.lrp_linear_stream_fwd_splits(M, N, K) == splits
    for odt in (BF16, F32):
        with_bias = odt == F32
        outs = []
        for _ in range(2):          # the second call finds the tickets the first one re-armed
            store, out = _nan_out(M, N, 8, odt)
            assert ops.linear_stream_fwd(x, W, g["bias"] if with_bias else None, out=out) is out
            torch.cuda.synchronize()
            _spare("out", store, M, N)
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "second call on the same tickets: not the same bits"
        _judge("skinny", dict(g, odt=odt, with_bias=with_bias), {"out": outs[1]},
               f"linear_stream_fwd {shape} M {M} W {N}x{K} splits {splits} ->{'bf16' if odt == BF16 else 'fp32'}{' +bias' if with_bias else ''}")


@pytest.mark.parametrize("M", gb.STREAM_M)
def test_linear_stream_dgrad(ops, M):
    N, Kout, splits = gb.STREAM_DGRAD
    g = gb.to(gb.operands(M, Kout, N, nn=True, seed=12, with_res=False, chain=N // (4 * splits), adds=3 + splits, group=4), "cuda")
    s2, W = _pitched(g["A"]), _pitched(g["B"])
    assert ops.linear_stream_dgrad_ok(s2, W) == (M <= 32)          # (33 rows: the kernel still applies -- four row blocks per wave --, the policy prefers the split-K path)
    for odt in (BF16, F32):
        outs = []
        for _ in range(2):
            store, out = _nan_out(M, Kout, 8, odt)
            assert ops.linear_stream_dgrad(s2, W, out=out) is out
            torch.cuda.synchronize()
            _spare("out", store, M, Kout)
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "second call on the same tickets: not the same bits"
        _judge("skinny", dict(g, odt=odt), {"out": outs[1]}, f"linear_stream_dgrad M {M} W {N}x{Kout} splits {splits} ->{'bf16' if odt == BF16 else 'fp32'}")


@pytest.mark.parametrize("rel_in", [False, True], ids=["gradient", "relevance"])
@pytest.mark.parametrize("M", gb.STREAM_M)
def test_linear_stream_dgrad_fused_stabiliser(ops, M, rel_in):
    """z given: s = g z / (z + eps) or g / (z + eps) is formed and rounded to bf16 inside the kernel (the form the engines run).  The entry takes z
    at 32 rows at most: 33 rows are refused before a launch"""
    N, Kout, splits = gb.STREAM_DGRAD
    eps = 1e-6
    g = gb.to(gb.operands(M, Kout, N, nn=True, seed=13, with_res=False, with_z=True, chain=N // (4 * splits), adds=3 + splits, group=4, eps=eps,
                          rel_in=rel_in), "cuda")
    s2, z, W = _pitched(g["A"]), _pitched(g["z"], 16), _pitched(g["B"])
    assert z.stride(0) != s2.stride(0)
    if M > 32:
        with pytest.raises(RuntimeError, match="lrp_linear_stream_dgrad_tk"):
            ops.linear_stream_dgrad(s2, W, out=_nan_out(M, Kout, 8, BF16)[1], z=z, eps=eps, relevance_in=rel_in)
        return
    for odt in (BF16, F32):
        outs = []
        for _ in range(2):          # the second call finds the tickets the first one re-armed
            store, out = _nan_out(M, Kout, 8, odt)
            assert ops.linear_stream_dgrad(s2, W, out=out, z=z, eps=eps, relevance_in=rel_in) is out
            torch.cuda.synchronize()
            _spare("out", store, M, Kout)
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "second call on the same tickets: not the same bits"
        _judge("stream_dgrad", dict(g, odt=odt), {"out": outs[1]},
               f"linear_stream_dgrad M {M} W {N}x{Kout} splits {splits} s = g {'' if rel_in else 'z '}/ (z + eps) ->{'bf16' if odt == BF16 else 'fp32'}")
