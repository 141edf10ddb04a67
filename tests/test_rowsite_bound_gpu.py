"""The decoder-family row and site kernels against the element-wise bounds of tests/rowsite_bound.py (which derives them and lists the rounding
points; tests/test_rowsite_bound_cpu.py shows that they are sound, that they discriminate and that the shapes below reach what they claim):
lrp_add_rmsnorm_fwd, lrp_rmsnorm_bwd_add2, lrp_rms_rstd, lrp_head_rmsnorm_fwd / _bwd, lrp_rope_fwd / _bwd, lrp_gqa_reduce_rope,
lrp_gated_act_fwd / _bwd and their _il forms, lrp_gated_cp_bwd_il, lrp_add2_rule_bwd, lrp_sandwich_norm_fwd / _bwd, lrp_qk_norm_rope_fwd,
lrp_qkv_bwd_pack, in both storage types, at the edges of their dispatch (rowsite_bound.cases; the table in DESIGN.md).

Every output is a NaN-guarded view (Guard / Guard2d of tests/test_rowops_gpu.py: nothing outside the result may be written) and goes through
moe_bound.check: finite, within the bound on EVERY element, exact zeros where the reference is a zero under a zero bound.  The row-wise outputs
keep the per-row check of tests/test_rowops_gpu.py beside it, the site kernels their bit-identity to the launch sequences they replace.  Each
case prints `RATIO <case> <dtype> <output> <worst err / bound>`; profiles/rowsite_bound_ratios.txt is that output.

The wrapper contracts of lxt_amd.ops (no row pitch in the C ABI of the row norms; table shapes of RoPE; shapes and strides of the gated forms)
are held by refusal tests at the end: a refused call raises before any launch and leaves its sentinel-filled output untouched."""
import pytest
import torch

from tests import rowsite_bound as rb
from tests.gemm_bound import il_join, il_split
from tests.test_rowops_gpu import Guard, Guard2d, off_grid

pytestmark = pytest.mark.gpu

BF16, F32 = rb.BF16, rb.F32
DT = {"bf16": BF16, "fp32": F32}
TOL = {F32: 2e-5, BF16: 2e-2}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.ops as o
    return o


# ---- placement ---------------------------------------------------------------------------------------------------------------------------------
def put(t, place, dtype=None):
    """a logical CPU tensor as the device tensor the case asks for: flattened to 2-D [rows, cols]; contiguous, one element off the 16-byte grid
    (off), or a column slice of a wider NaN-filled buffer (pad: extra elements of row pitch; the slice starts one 16-byte chunk in when the
    pitch keeps the chunks aligned)"""
    if t is None:
        return None
    t = t.reshape(t.shape[0], -1).cuda()
    if place["off"]:
        return off_grid(t)
    if place["pad"]:
        W = 16 // t.element_size()
        return Guard2d(t.shape[0], t.shape[1], t.shape[1] + place["pad"], W if place["pad"] % W == 0 else 0, t.dtype, t).view
    return t.contiguous()


def vec(t, place):
    if t is None:
        return None
    return off_grid(t.cuda()) if place["off"] else t.cuda()


class Outs:
    """the guarded outputs of one call"""

    def __init__(self, place):
        self.place, self.guards = place, {}

    def new(self, name, rows, cols, dtype):
        if self.place["pad"] and not self.place["off"]:
            W = 16 // torch.empty((), dtype=dtype).element_size()
            g = Guard2d(rows, cols, cols + self.place["pad"], W if self.place["pad"] % W == 0 else 0, dtype)
            g.out = g.view
        else:
            g = Guard((rows, cols), dtype, self.place["off"])
        self.guards[name] = g
        return g.out

    def stat(self, name, n):
        g = Guard((n,), torch.float32)
        self.guards[name] = g
        return g.out

    def untouched(self):
        for g in self.guards.values():
            g.untouched()

    def __getitem__(self, name):
        return self.guards[name].out


# ---- one call per op -----------------------------------------------------------------------------------------------------------------------------
def run(ops, op, d, place, dtype):
    """-> ({output: device tensor}, Outs, {output: the launch sequence's result, to be bit-identical})"""
    o, same = Outs(place), {}
    P = lambda k: put(d.get(k), place)      # noqa: E731
    cs = lambda: (vec(d["cos"], place), vec(d["sin"], place))      # noqa: E731
    if op == "add_rmsnorm_fwd":
        M, H = d["h"].shape
        h, w = P("h"), vec(d["w"], place)
        hs = None
        if d["hsum_out"]:
            hs = o.new("hsum", M, H, dtype)
            if d["inplace"]:
                hs.copy_(h)
                h = hs
        y = o.new("y", M, H, dtype) if d["norm_out"] else None
        yy, rstd = ops.add_rmsnorm_fwd(h, P("branch"), w, d["eps"], d["w_off"], hsum_out=hs, y=y, rstd=o.stat("rstd", M), norm_out=d["norm_out"])
        assert (yy is None) == (not d["norm_out"]) and rstd.data_ptr() == o["rstd"].data_ptr()
        return {k: o[k] for k in o.guards}, o, same
    if op == "rmsnorm_bwd_add2":
        M, H = (d["Gx"] if d["Gx"] is not None else d["Gres"]).shape
        A = o.new("A", M, H, dtype) if d["branch"] is not None else None
        rel = o.stat("rel", M) if d["rel"] else None
        ops.rmsnorm_bwd_add2(P("Gres"), P("Gx"), vec(d["w"], place), None if d["rstd"] is None else d["rstd"].cuda(), P("hsum"), P("branch"),
                             o.new("Gs", M, H, dtype), A, rel, d["w_off"], d["eps_add"], d["eps_lin"])
        return {k: o[k] for k in o.guards}, o, same
    if op == "rms_rstd":
        ops.rms_rstd(d["ssq"].cuda(), d["M"], d["H"], d["eps"], o.stat("rstd", d["M"]))
        return {"rstd": o["rstd"]}, o, same
    if op == "head_rmsnorm_fwd":
        rows, heads, dd = d["x"].shape
        ops.head_rmsnorm_fwd(P("x"), d["w"].cuda(), o.new("y", rows, heads * dd, dtype), o.stat("rstd", rows * heads), heads, dd, d["eps"], d["w_off"])
        return {"y": o["y"], "rstd": o["rstd"]}, o, same
    if op == "head_rmsnorm_bwd":
        rows, heads, dd = d["G"].shape
        ops.head_rmsnorm_bwd(P("G"), d["w"].cuda(), d["rstd"].reshape(-1).cuda(), o.new("out", rows, heads * dd, dtype), heads, dd, d["w_off"])
        return {"out": o["out"]}, o, same
    if op == "rope_fwd":
        rows, nh, dd = d["x"].shape
        ops.rope_fwd(P("x"), o.new("xr", rows, nh * dd, dtype), *cs(), d["seq"], nh, dd)
        return {"xr": o["xr"]}, o, same
    if op == "rope_bwd":
        rows, nh, dd = d["Gr"].shape
        ops.rope_bwd(P("Gr"), P("xr") if d["eps_rope"] else None, P("x") if d["eps_lin"] else None, o.new("A", rows, nh * dd, dtype), *cs(), d["seq"],
                     nh, dd, d["eps_rope"], d["eps_lin"])
        return {"A": o["A"]}, o, same
    if op == "gqa_reduce_rope":
        rows, nh, dd = d["x"].shape
        hk = nh // d["rep"]
        ops.gqa_reduce_rope(P("x"), o.new("out", rows, hk * dd, dtype), rows, d["seq"], hk, d["rep"], dd, *cs())
        return {"out": o["out"]}, o, same
    if op in ("gated_fwd", "gated_bwd", "gated_cp"):
        M, I = d["g"].shape
        il = place["form"] == "il"
        if il:
            gu = put(il_join(d["g"], d["u"]), place)
        if op == "gated_fwd":
            m = o.new("m", M, I, dtype)
            if il:
                ops.gated_act_fwd_il(gu, m, d["act"])
            else:
                ops.gated_act_fwd(P("g"), P("u"), m, d["act"])
            return {"m": m}, o, same
        if il:
            Agu = o.new("Agu", M, 2 * I, dtype)
            if op == "gated_cp":
                ops.gated_cp_bwd_il(P("Gm"), gu, Agu, d["act"])
            else:
                ops.gated_act_bwd_il(P("Gm"), gu, Agu, d["eps_g"], d["eps_lin"], d["act"])
            ag, au = il_split(Agu)
            return {"Ag": ag, "Au": au}, o, same
        ops.gated_act_bwd(P("Gm"), P("g"), P("u"), o.new("Ag", M, I, dtype), o.new("Au", M, I, dtype), d["eps_g"], d["eps_lin"], d["act"])
        return {"Ag": o["Ag"], "Au": o["Au"]}, o, same
    if op == "add2":
        a, b, R = (vec(d[k][0], place) for k in ("a", "b", "R"))
        Ra, Rb = ops.add2_rule_bwd(a, b, R, d["eps"])
        Ra1, none = ops.add2_rule_bwd(a, b, R, d["eps"], need_b=False)
        assert none is None and torch.equal(Ra1, Ra)
        return {"Ra": Ra[None], "Rb": Rb[None]}, o, same
    if op == "sandwich_fwd":
        M, H = d["x"].shape
        x, res, w1, w2 = P("x"), P("res"), d["w_post"].cuda(), d["w_pre"].cuda()
        e = lambda: torch.empty(M, H, dtype=dtype, device="cuda")      # noqa: E731
        pa, r1 = ops.add_rmsnorm_fwd(x, None, w1, d["eps"], d["w_off"])
        h_ref, y_ref, r2 = e(), e(), torch.empty(M, device="cuda")
        ops.add_rmsnorm_fwd(res, pa, w2, d["eps"], d["w_off"], hsum_out=h_ref, y=y_ref, rstd=r2)
        seq = dict(rstd_post=r1, hsum=h_ref, rstd_pre=r2, y=y_ref)
        assert ops.sandwich_norm_ok(x) == rb.sandwich_ok(H, dtype)
        if not ops.sandwich_norm_ok(x):          # one step beyond the gate: the pair is what runs, and what is held to the bound
            return seq, o, same
        ops.sandwich_norm_fwd(x, res, w1, w2, d["eps"], d["w_off"], o.new("hsum", M, H, dtype), o.new("y", M, H, dtype), o.stat("rstd_post", M),
                              o.stat("rstd_pre", M))
        hb, qb1, qb2 = e(), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        ops.sandwich_norm_fwd(x, res, w1, None, d["eps"], d["w_off"], hb, None, qb1, qb2)          # without the pre-norm's output
        assert torch.equal(hb, o["hsum"]) and torch.equal(qb1, o["rstd_post"]) and torch.equal(qb2, o["rstd_pre"])
        return {k: o[k] for k in o.guards}, o, seq
    if op == "sandwich_bwd":
        M, H = d["Gx"].shape
        Gx, Gres, w1, w2 = P("Gx"), P("Gres"), d["w_post"].cuda(), d["w_pre"].cuda()
        r1, r2 = d["rstd_post"].cuda(), d["rstd_pre"].cuda()
        if place["big"]:
            seq = {}
        else:
            Gs_ref, Ga_ref = torch.empty_like(Gx), torch.empty_like(Gx)
            ops.rmsnorm_bwd_add2(Gres, Gx, w2, r2, None, None, Gs_ref, None, None, d["w_off"], 0.0, 0.0)
            ops.rmsnorm_bwd_add2(None, Gs_ref, w1, r1, None, None, Ga_ref, None, None, d["w_off"], 0.0, 0.0)
            seq = dict(Gs=Gs_ref, Ga=Ga_ref)
        if not ops.sandwich_norm_ok(Gx):
            with pytest.raises(ValueError):
                ops.sandwich_norm_bwd(Gres, Gx, w2, r2, w1, r1, torch.empty_like(Gx), torch.empty_like(Gx), d["w_off"])
            return seq, o, same
        ops.sandwich_norm_bwd(Gres, Gx, w2, r2, w1, r1, o.new("Gs", M, H, dtype), o.new("Ga", M, H, dtype), d["w_off"])
        return {"Gs": o["Gs"], "Ga": o["Ga"]}, o, seq
    if op == "qk_norm_rope":
        rows, nq, dd = d["q"].shape
        nk = d["k"].shape[1]
        v = torch.full((rows, nk * dd), float("nan"), dtype=dtype)          # the v heads behind q and k are not this kernel's to read
        qkv = put(torch.cat((d["q"].reshape(rows, -1), d["k"].reshape(rows, -1), v), 1), place)
        wq, wk, (cos, sin) = d["wq"].cuda(), d["wk"].cuda(), cs()
        ops.qk_norm_rope_fwd(qkv, wq, wk, o.new("qr", rows, nq * dd, dtype), o.new("kr", rows, nk * dd, dtype), o.stat("rstd_q", rows * nq),
                             o.stat("rstd_k", rows * nk), cos, sin, d["seq"], nq, nk, dd, d["eps"], d["w_off"])
        seq = {}
        if not place["big"]:
            e = lambda n: torch.empty(rows, n, dtype=dtype, device="cuda")      # noqa: E731
            rq, rk = torch.empty(rows * nq, device="cuda"), torch.empty(rows * nk, device="cuda")
            qn, kn = e(nq * dd), e(nk * dd)
            ops.head_rmsnorm_fwd(qkv[:, : nq * dd], wq, qn, rq, nq, dd, d["eps"], d["w_off"])
            ops.head_rmsnorm_fwd(qkv[:, nq * dd: (nq + nk) * dd], wk, kn, rk, nk, dd, d["eps"], d["w_off"])
            seq = dict(qr=ops.rope_fwd(qn, e(nq * dd), cos, sin, d["seq"], nq, dd), kr=ops.rope_fwd(kn, e(nk * dd), cos, sin, d["seq"], nk, dd),
                       rstd_q=rq, rstd_k=rk)
        return {k: o[k] for k in o.guards}, o, seq
    if op == "qkv_bwd_pack":
        rows, nq, dd = d["dq"].shape
        nk = d["rstd_k"].shape[1]
        rep = nq // nk
        dq, dk_h, dv_h, wq, wk, (cos, sin) = P("dq"), P("dk_h"), P("dv_h"), d["wq"].cuda(), d["wk"].cuda(), cs()
        rq, rk = d["rstd_q"].reshape(-1).cuda(), d["rstd_k"].reshape(-1).cuda()
        A = o.new("A", rows, (nq + 2 * nk) * dd, dtype)
        ops.qkv_bwd_pack(dq, dk_h, dv_h, wq, wk, rq, rk, cos, sin, A, d["seq"], nq, nk, dd, d["w_off"])
        outs = {"Aq": A[:, : nq * dd], "Ak": A[:, nq * dd: (nq + nk) * dd], "Av": A[:, (nq + nk) * dd:]}
        seq = {}
        if not place["big"]:
            e = lambda n: torch.empty(rows, n, dtype=dtype, device="cuda")      # noqa: E731
            dk = ops.gqa_reduce(dk_h, e(nk * dd), rows, nk, rep, dd)
            seq["Av"] = ops.gqa_reduce(dv_h, e(nk * dd), rows, nk, rep, dd)
            Gqn = ops.rope_bwd(dq, None, None, e(nq * dd), cos, sin, d["seq"], nq, dd, 0.0, 0.0)
            Gkn = ops.rope_bwd(dk, None, None, e(nk * dd), cos, sin, d["seq"], nk, dd, 0.0, 0.0)
            seq["Aq"] = ops.head_rmsnorm_bwd(Gqn, wq, rq, e(nq * dd), nq, dd, d["w_off"])
            seq["Ak"] = ops.head_rmsnorm_bwd(Gkn, wk, rk, e(nk * dd), nk, dd, d["w_off"])
        return outs, o, seq
    raise KeyError(op)


ROW_WISE = {"add_rmsnorm_fwd": (("y",), 1), "rmsnorm_bwd_add2": (("Gs", "A"), 5), "head_rmsnorm_fwd": (("y",), 1), "head_rmsnorm_bwd": (("out",), 1),
            "sandwich_fwd": (("hsum", "y"), 1), "sandwich_bwd": (("Gs", "Ga"), 5)}


def judge(ops, tag, op, kw, place, dt):
    dtype = DT[dt]
    d = rb.operands(op, dtype, **kw)
    outs, guards, seq = run(ops, op, d, place, dtype)
    torch.cuda.synchronize()
    guards.untouched()
    dev = rb.to(d, "cuda")
    R = rb.references(op, dev)
    x64 = {n: t.double().reshape(R[n][0].shape) for n, t in outs.items()}
    assert set(x64) == set(R), (tag, set(x64), set(R))
    log = rb.evaluate(op, dev, x64, tag=f"{tag} {dt} ")
    for n in ROW_WISE.get(op, ((), 1))[0]:          # the per-row check of tests/test_rowops_gpu.py rides along
        if n in x64:
            rb.row_check(f"{tag} {dt} {n}", x64[n], R[n][0], ROW_WISE[op][1] * TOL[dtype])
    for n, t in seq.items():          # the site kernels: bit-identical to the launch sequence they replace
        assert torch.equal(outs[n].reshape(-1), t.reshape(-1)), f"{tag} {n}: not bit-identical to the launch sequence"
    for n, r in log.items():
        print(f"RATIO {tag} {dt} {n.split()[-1]} {r:.3f}")
    return log


def _run_family(ops, dt, family, pick=lambda c: True):
    n = 0
    for tag, op, kw, place in rb.cases(DT[dt], family):
        if pick((tag, op, kw, place)):
            judge(ops, tag, op, kw, place, dt)
            n += 1
    assert n


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("width", range(len(rb.ROW_WIDTHS)))
def test_row_norms(ops, dt, width):
    """lrp_add_rmsnorm_fwd in its six call forms and lrp_rmsnorm_bwd_add2 in the six operand subsets the engines use, both weight conventions,
    every stabiliser pair, at one width of rowsite_bound.ROW_WIDTHS"""
    k, M, off = rb.ROW_WIDTHS[width]
    H = -k if k < 0 else k * rb.epc(DT[dt])
    _run_family(ops, dt, "rownorm", lambda c: c[1] != "rms_rstd" and c[2]["H"] == H and c[2]["M"] == M and c[3]["off"] == off)


@pytest.mark.parametrize("dt", list(DT))
def test_rms_rstd(ops, dt):
    _run_family(ops, dt, "rownorm", lambda c: c[1] == "rms_rstd")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("big", [False, True], ids=["edges", "past_cap"])
def test_head_norms(ops, dt, big):
    _run_family(ops, dt, "head", lambda c: c[3]["big"] == big)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("big", [False, True], ids=["edges", "past_cap"])
def test_rope(ops, dt, big):
    _run_family(ops, dt, "rope", lambda c: c[3]["big"] == big)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("part", ["split", "il", "past_cap"])
def test_gated(ops, dt, part):
    _run_family(ops, dt, "gated", lambda c: (part == "past_cap") == c[3]["big"] and (c[3]["big"] or c[3]["form"] == part))


@pytest.mark.parametrize("dt", list(DT))
def test_add2(ops, dt):
    _run_family(ops, dt, "add2")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("big", [False, True], ids=["edges", "past_cap"])
def test_sandwich(ops, dt, big):
    _run_family(ops, dt, "sandwich", lambda c: c[3]["big"] == big)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("part", ["qk_norm_rope", "qkv_bwd_pack", "past_cap"])
def test_qk_site_kernels(ops, dt, part):
    _run_family(ops, dt, "qk", lambda c: (part == "past_cap") == c[3]["big"] and (c[3]["big"] or c[1] == part))


# ---- wrapper contracts: refused before any launch ------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def _sent(*shape, dtype=BF16):
    return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")


def _refused(fn, *outs, exc=ValueError):
    with pytest.raises(exc):
        fn()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), "a refused call wrote its output"


@pytest.mark.parametrize("dt", list(DT))
def test_row_norm_wrappers_refuse_views_without_a_pitch(ops, dt):
    """lrp_add_rmsnorm_fwd, lrp_rmsnorm_bwd_add2 and lrp_sandwich_norm_fwd index row * H: a column slice (or a tensor of another shape) as any
    operand would be read and written at the wrong addresses and past the view"""
    dtype, M, H = DT[dt], 5, 64
    wide = lambda: _sent(M, 2 * H, dtype=dtype)      # noqa: E731
    full = lambda: _sent(M, H, dtype=dtype)      # noqa: E731
    w, st = torch.ones(H, dtype=dtype, device="cuda"), lambda n=M: _sent(n, dtype=torch.float32)      # noqa: E731
    for bad in ("h", "branch", "hsum_out", "y"):
        t = {k: (wide() if k == bad else full()) for k in ("h", "branch", "hsum_out", "y")}
        v = {k: (x[:, :H] if k == bad else x) for k, x in t.items()}
        r = st()
        _refused(lambda: ops.add_rmsnorm_fwd(v["h"], v["branch"], w, 1e-6, 0.0, hsum_out=v["hsum_out"], y=v["y"], rstd=r), t["hsum_out"], t["y"], r)
    r, y = st(), full()
    _refused(lambda: ops.add_rmsnorm_fwd(full(), full()[:3], w, 1e-6, y=y, rstd=r), y, r)          # branch of another row count
    r, y = st(M - 1), full()
    _refused(lambda: ops.add_rmsnorm_fwd(full(), None, w, 1e-6, y=y, rstd=r), y, r)                # rstd shorter than M
    names = ("Gres", "Gx", "hsum", "branch", "Gs_out", "A_out")
    for bad in names:
        t = {k: (wide() if k == bad else full()) for k in names}
        v = {k: (x[:, :H] if k == bad else x) for k, x in t.items()}
        rel = st()
        _refused(lambda: ops.rmsnorm_bwd_add2(v["Gres"], v["Gx"], w, st(), v["hsum"], v["branch"], v["Gs_out"], v["A_out"], rel, 0.0, 1e-8, 1e-8),
                 t["Gs_out"], t["A_out"], rel)
    gs, a = full(), full()
    _refused(lambda: ops.rmsnorm_bwd_add2(full(), full(), w, st(M - 1), full(), full(), gs, a, None), gs, a)
    names = ("x", "res", "hsum_out", "y")
    for bad in names:
        t = {k: (wide() if k == bad else full()) for k in names}
        v = {k: (x[:, :H] if k == bad else x) for k, x in t.items()}
        r1, r2 = st(), st()
        _refused(lambda: ops.sandwich_norm_fwd(v["x"], v["res"], w, w, 1e-6, 1.0, v["hsum_out"], v["y"], r1, r2), t["hsum_out"], t["y"], r1, r2)
    # the by-hand .contiguous() of the call sites is what a caller has to do: a copy of the slice is accepted
    y, _ = ops.add_rmsnorm_fwd(wide()[:, :H].contiguous(), None, w, 1e-6)
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("dt", list(DT))
def test_rope_wrappers_refuse_short_and_strided_tables(ops, dt):
    dtype, rows, seq, nh, d = DT[dt], 10, 5, 2, 16
    x = torch.randn(rows, nh * d, device="cuda").to(dtype)
    tab = lambda n=seq, w=d: torch.ones(n, w, device="cuda")      # noqa: E731
    cases = {"short": (tab(seq - 1), tab(seq - 1)), "strided": (tab(seq, 2 * d)[:, :d], tab()), "wide": (tab(), tab(seq, 2 * d)),
             "transposed": (tab(d, seq).T, tab())}
    for name, (cos, sin) in cases.items():
        out = _sent(rows, nh * d, dtype=dtype)
        _refused(lambda: ops.rope_fwd(x, out, cos, sin, seq, nh, d), out)
        _refused(lambda: ops.rope_bwd(x, None, None, out, cos, sin, seq, nh, d, 0.0, 0.0), out)
        _refused(lambda: ops.gqa_reduce_rope(x, out[:, :d], rows, seq, 1, nh, d, cos, sin), out)
    out = _sent(rows, nh * d, dtype=dtype)
    _refused(lambda: ops.rope_fwd(x[:, : d], out, tab(), tab(), seq, nh, d), out)                  # fewer columns than n_heads d
    _refused(lambda: ops.rope_fwd(x.T.contiguous().T, out, tab(), tab(), seq, nh, d), out)         # column stride != 1
    _refused(lambda: ops.rope_bwd(x, None, None, out[:5], tab(), tab(), seq, nh, d, 0.0, 0.0), out)
    ok = ops.rope_fwd(x, torch.empty_like(x), tab(seq + 3), tab(seq + 3), seq, nh, d)             # a longer table is fine
    assert bool(torch.isfinite(ok).all())


@pytest.mark.parametrize("dt", list(DT))
def test_gated_wrappers_refuse_wrong_shapes_and_strides(ops, dt):
    dtype, M, I = DT[dt], 6, 64
    t = lambda r=M, c=I: torch.randn(r, c, device="cuda").to(dtype)      # noqa: E731
    out = _sent(M, I, dtype=dtype)
    _refused(lambda: ops.gated_act_fwd(t(), t(M, I // 2), out), out)                               # u narrower than g
    _refused(lambda: ops.gated_act_fwd(t(), t(M - 1), out), out)
    _refused(lambda: ops.gated_act_fwd(t(I, M).T, t(), out), out)                                  # column stride != 1
    ag, au = _sent(M, I, dtype=dtype), _sent(M, I, dtype=dtype)
    _refused(lambda: ops.gated_act_bwd(t(), t(), t(M, I // 2), ag, au, 1e-10, 0.0), ag, au)
    _refused(lambda: ops.gated_act_bwd(t(M, I // 2), t(), t(), ag, au, 1e-10, 0.0), ag, au)
    _refused(lambda: ops.gated_act_bwd(t(), t(), t(), ag, au[:, : I // 2], 1e-10, 0.0), ag, au)
    _refused(lambda: ops.gated_act_fwd_il(t(M, I), out), out)                                      # gu holds I columns, not 2 I
    _refused(lambda: ops.gated_act_fwd_il(t(M - 1, 2 * I), out), out)
    agu = _sent(M, 2 * I, dtype=dtype)
    _refused(lambda: ops.gated_act_bwd_il(t(), t(M, I), agu, 1e-10, 0.0), agu)
    _refused(lambda: ops.gated_act_bwd_il(t(), t(M, 2 * I), agu[:, :I], 1e-10, 0.0), agu)
    _refused(lambda: ops.gated_cp_bwd_il(t(), t(M, I), agu), agu)
    _refused(lambda: ops.gated_cp_bwd_il(t(), t(2 * I, M).T, agu), agu)
    # the library states the same for a caller of the C ABI: a row of gu shorter than 2 I
    import lxt_amd._lib as L
    code = L.BF16 if dtype == BF16 else L.F32
    gu = t(M, 2 * I)
    assert L.lib.lrp_gated_act_fwd_il(gu.data_ptr(), out.data_ptr(), M, I, I, I, 0, code, None) == -3
    assert L.lib.lrp_gated_act_bwd_il(t().data_ptr(), gu.data_ptr(), agu.data_ptr(), M, I, I, I, 2 * I, 1e-10, 0.0, 0, code, None) == -3
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((agu == SENTINEL).all())
