"""GPU: every routed-expert kernel of csrc/moe.hip on its own against the element-wise bounds of tests/moe_bound.py -- the four grouped GEMMs,
lrp_moe_combine, lrp_moe_gw_reduce -- and lrp_moe_plan at its chunk and scan edges.
  (1) every op of every case of moe_bound.CASES (bf16 and fp32; both activations on `edges`) through moe_bound.evaluate: finite,
      |x - fp64 reference| <= bound on EVERY element, the exact zeros.  Inputs are [:, :cols] views of wider storage (pitches off the row width,
      on the 16-byte grid); outputs go into sentinel-filled pitched buffers, and afterwards every pad column and every row at or past off[E]
      still holds the sentinel's bits.  The rows nothing may read are NaN (moe_bound.inputs): none reaches an output;
  (2) position independence on `edges`: 1 / 127 / 128 tokens routed to one expert are prepended, so each of its rows moves to another MFMA row,
      another tile or both (and every later expert's p0 moves); the original rows' coef, m, y, Agu, gw, gx_rows and their tokens' out, G_x are
      bit-identical, op by op and through MoEExpertsFn;
  (3) the plan at R in {255, 256, 257, 513} x E in {1, 257, 1024} with ids < 0, == E and > E as skipped slots: cnt, off, toff, perm, inv."""
import pytest
import torch

from tests import moe_bound as mb

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SENT = {BF16: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC12345)}          # a NaN with a payload no kernel produces


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")
    from lxt_amd import ops
    return ops


def _sentinel(rows, cols, pad, dtype):
    """-> (storage [rows, cols + pad] filled with the sentinel, its [:, :cols] view)"""
    it, bits = SENT[dtype]
    store = torch.full((rows, cols + pad), bits, dtype=it, device="cuda").view(dtype)
    return store, store[:, :cols]


def _untouched(name, store, cols, n):
    """the pad columns of every row and every column of the rows >= n still hold the sentinel's bits"""
    it, bits = SENT[store.dtype]
    b = store.view(it)
    assert bool((b[:, cols:] == bits).all()), f"{name}: a pad column was written"
    assert bool((b[n:] == bits).all()), f"{name}: a row at or past off[E] was written"
    if n:
        assert not bool((b[:n, :cols] == bits).any()), f"{name}: a live element was left unwritten"


def _view(t, pad):
    """a CPU tensor as a [:, :cols] view of NaN-filled device storage [rows, cols + pad]"""
    store = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device="cuda")
    store[:, :t.shape[1]] = t.cuda()
    return store[:, :t.shape[1]]


def _plan_matches(plan, P):
    cnt, off, perm, inv = (v.long().cpu() for v in plan.views())
    E = P.E
    assert cnt.tolist() == P.cnt.tolist() and off.tolist() == P.off.tolist() and perm[:P.n].tolist() == P.src.tolist()
    assert inv.tolist() == P.inv.tolist() and plan.buf[2 * E + 1:3 * E + 2].long().cpu().tolist() == P.toff.tolist()


def _run_ops(ops, d, act):
    """every op of one case on its own inputs -> fp64 CPU outputs under the keys of moe_bound.evaluate; the untouched-sentinel checks"""
    name, dtype = d["name"], d["dtype"]
    c, P = mb.CASES[name], mb.plan_of(name)
    E, T, k, H, I, R, n = c["E"], c["T"], c["k"], c["H"], c["I"], P.R, P.n
    v = 16 // dtype.itemsize
    plan = ops.MoePlan(mb.routing(name).cuda(), E)
    _plan_matches(plan, P)
    x, G, m_in = _view(d["x"], v), _view(d["G"], 3 * v), _view(d["m_in"], v)
    coef_in, Agu_in, rows_in = _view(d["coef_in"], 3 * v), _view(d["Agu_in"], v), _view(d["rows_in"], 3 * v)
    Wgu, Wd, w = d["Wgu"].cuda(), d["Wd"].cuda(), d["w"].cuda()
    for t in (x, G, m_in, coef_in, Agu_in, rows_in):
        assert t.stride(0) != t.shape[1] and (t.stride(0) * dtype.itemsize) % 16 == 0
    S = {}
    for key, rows, cols, pad in (("coef", R, 2 * I, v), ("m", R, I, 3 * v), ("y", R, H, v), ("Agu", R, 2 * I, 3 * v), ("gx_rows", R, H, 3 * v),
                                 ("out_w", T, H, v), ("out_1", T, H, 3 * v)):
        S[key] = _sentinel(rows, cols, pad, dtype)
    part_s, part = _sentinel(R, I // 128, 0, F32)
    gw_s, gw = _sentinel(T, k, 0, dtype)
    coef, m = ops.moe_gate_up_fwd(x, Wgu, plan, act, coef=S["coef"][1], m=S["m"][1])
    assert coef is S["coef"][1] and m is S["m"][1]
    assert ops.moe_down_fwd(m_in, Wd, plan, out=S["y"][1]) is S["y"][1]
    Agu, gw_out = ops.moe_down_dgrad(G, Wd, coef_in, m_in, w, plan, Agu=S["Agu"][1], part=part, gw=gw)
    assert Agu is S["Agu"][1] and gw_out is gw
    assert ops.moe_gate_up_dgrad(Agu_in, Wgu, plan, out=S["gx_rows"][1]) is S["gx_rows"][1]
    assert ops.moe_combine(rows_in, plan, w, out=S["out_w"][1]) is S["out_w"][1]
    assert ops.moe_combine(rows_in, plan, out=S["out_1"][1]) is S["out_1"][1]
    torch.cuda.synchronize()
    for key in ("coef", "m", "y", "Agu", "gx_rows"):
        _untouched(key, S[key][0], S[key][1].shape[1], n)
    _untouched("gw_part", part_s, I // 128, n)
    for key in ("out_w", "out_1"):
        _untouched(key, S[key][0], H, T)
    assert not bool((gw_s.view(SENT[dtype][0]) == SENT[dtype][1]).any()), "gw: an element was left unwritten"
    live = lambda t: t[:n].double().cpu()      # noqa: E731
    return dict(m=live(m), cg=live(coef[:, :I]), cu=live(coef[:, I:]), y=live(S["y"][1]), Agu=live(Agu), gw=gw.double().cpu(),
                gx_rows=live(S["gx_rows"][1]), out_w=S["out_w"][1].double().cpu(), out_1=S["out_1"][1].double().cpu())


@pytest.mark.parametrize("name,dtype,act", mb.RUNS, ids=mb.RUN_IDS)
def test_every_op_within_its_bound(ops, name, dtype, act):
    d = mb.inputs(name, dtype)
    c, P = mb.CASES[name], mb.plan_of(name)
    print(f"[{name} {dtype} {act}] rows per expert {P.cnt.tolist() if c['E'] <= 8 else 'max %d' % int(P.cnt.max())}, {P.R - P.n} skipped slots")
    if name == "wrap":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        items = {"gate_up_fwd": int(P.toff[-1]) * (2 * c["I"] // 128), "down_dgrad": int(P.toff[-1]) * (c["I"] // 128)}
        print(f"  work items {items} on a grid of at most {2 * cus} blocks")
        assert all(i > 2 * cus for i in items.values()), (items, cus)
    out = _run_ops(ops, d, act)
    log = mb.evaluate(d, act, out)
    print(f"kernels {name} {dtype} {act}: worst err / bound per output: " + " ".join(f"{n} {r:.3f}" for n, r in log.items()))
    assert set(log) == {"m", "cg", "cu", "y", "Agu", "gw", "gx_rows", "out_w", "out_1"}
    if name == "none":          # (the four GEMMs left their buffers untouched: _run_ops with off[E] = 0)
        assert P.n == 0 and not bool(out["gw"].any()) and not bool(out["out_w"].any()) and not bool(out["out_1"].any())


def test_output_buffers_are_checked(ops):
    """a handed buffer of the wrong type, device, shape or row layout is refused before any kernel"""
    name = "seams"
    d, c = mb.inputs(name, BF16), mb.CASES[name]
    T, k, H, I, R = c["T"], c["k"], c["H"], c["I"], c["T"] * c["k"]
    plan = ops.MoePlan(mb.routing(name).cuda(), c["E"])
    x, G, w, Wgu, Wd = (d[key].cuda() for key in ("x", "G", "w", "Wgu", "Wd"))
    m_in, coef_in, Agu_in, rows_in = (d[key].cuda() for key in ("m_in", "coef_in", "Agu_in", "rows_in"))
    buf = lambda rows, cols, dtype=BF16, device="cuda": torch.zeros(rows, cols, dtype=dtype, device=device)      # noqa: E731
    with pytest.raises(TypeError):
        ops.moe_gate_up_fwd(x, Wgu, plan, coef=buf(R, 2 * I, F32))
    with pytest.raises(TypeError):
        ops.moe_gate_up_fwd(x, Wgu, plan, m=buf(R, I, device="cpu"))
    with pytest.raises(ValueError):
        ops.moe_gate_up_fwd(x, Wgu, plan, m=buf(R - 1, I))
    with pytest.raises(ValueError):
        ops.moe_down_fwd(m_in, Wd, plan, out=buf(H, R).T)
    with pytest.raises(ValueError):
        ops.moe_down_dgrad(G, Wd, coef_in, m_in, w, plan, Agu=buf(R, I))
    with pytest.raises(TypeError):
        ops.moe_down_dgrad(G, Wd, coef_in, m_in, w, plan, part=buf(R, I // 128))
    with pytest.raises(ValueError):
        ops.moe_down_dgrad(G, Wd, coef_in, m_in, w, plan, gw=buf(T, k + 2)[:, :k])
    with pytest.raises(ValueError):
        ops.moe_gate_up_dgrad(Agu_in, Wgu, plan, out=buf(R, 2 * H)[:, ::2])
    with pytest.raises(TypeError):
        ops.moe_combine(rows_in, plan, w, out=[buf(T, H)])
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):               # a row pitch off the 16-byte grid reaches the C entry's own check
        ops.moe_combine(rows_in, plan, w, out=buf(T, H + 4)[:, :H])


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("extra", [1, 127, 128])
def test_rows_do_not_depend_on_their_position(ops, extra, dtype):
    """`edges`, target expert 2 (127 rows): `extra` tokens routed to it (their other slot skipped) are prepended.  The plan is stable, so row i
    of the expert becomes row extra + i -- another MFMA row (1), another tile and MFMA row (127), another tile (128) -- and every later
    expert's p0 moves by `extra`.  The same operand bits reach the same accumulator in the same order: bit-identical"""
    from lxt_amd.efficient.moe import MoEExpertsFn
    name, target = "edges", 2
    d, c, P = mb.inputs(name, dtype), mb.CASES[name], mb.plan_of(name)
    E, T, k, H, I = c["E"], c["T"], c["k"], c["H"], c["I"]
    gen = torch.Generator().manual_seed(extra)
    idx1 = mb.routing(name)
    idx2 = torch.cat([torch.tensor([[target, E]]).repeat(extra, 1), idx1])
    plan1, plan2 = ops.MoePlan(idx1.cuda(), E), ops.MoePlan(idx2.cuda(), E)
    inv1, inv2 = plan1.views()[3].long(), plan2.views()[3].long()[extra * k:]
    live = inv1 >= 0
    assert torch.equal(live, inv2 >= 0)
    r1, r2 = inv1[live], inv2[live]
    n1, n2 = int(plan1.views()[1][E]), int(plan2.views()[1][E])
    assert n2 == n1 + extra
    off1, off2 = plan1.views()[1].long(), plan2.views()[1].long()
    ex = torch.tensor(P.expert.tolist(), device="cuda")[r1]          # expert of every original live row (r1 runs over plan 1's rows)
    pos1, pos2 = r1 - off1[ex], r2 - off2[ex]
    assert torch.equal(pos2 - pos1, torch.where(ex == target, extra, 0))
    moved = ex == target
    assert bool(((pos1[moved] % 16 != pos2[moved] % 16) | (pos1[moved] // 128 != pos2[moved] // 128)).all())
    assert bool((r2[ex > target] - r1[ex > target] == extra).all())

    def tokens(key):          # [T, .] -> [extra + T, .]
        t = d[key]
        return torch.cat([torch.randn(extra, t.shape[1], generator=gen).to(dtype), t]).cuda()

    def plan_rows(key):       # [R, .] in plan 1's rows -> plan 2's rows: the originals moved, finite filler on the new rows, NaN past off[E]
        t = d[key].cuda()
        out = torch.randn(2 * (T + extra), t.shape[1], generator=gen).to(dtype).cuda()
        out[n2:] = float("nan")
        out[r2] = t[r1]
        return out

    x1, G1, w1 = d["x"].cuda(), d["G"].cuda(), d["w"].cuda()
    x2, G2 = tokens("x"), tokens("G")
    w2 = torch.cat([torch.full((extra, k), 0.25).to(dtype), d["w"]]).cuda()
    Wgu, Wd = d["Wgu"].cuda(), d["Wd"].cuda()
    one = dict(m_in=d["m_in"].cuda(), coef_in=d["coef_in"].cuda(), Agu_in=d["Agu_in"].cuda(), rows_in=d["rows_in"].cuda())
    two = {key: plan_rows(key) for key in one}

    def run(plan, x, G, w, a):
        coef, m = ops.moe_gate_up_fwd(x, Wgu, plan)
        y = ops.moe_down_fwd(a["m_in"], Wd, plan)
        Agu, gw = ops.moe_down_dgrad(G, Wd, a["coef_in"], a["m_in"], w, plan)
        gx = ops.moe_gate_up_dgrad(a["Agu_in"], Wgu, plan)
        return dict(coef=coef, m=m, y=y, Agu=Agu, gx_rows=gx), dict(gw=gw, out_w=ops.moe_combine(a["rows_in"], plan, w),
                                                                    out_1=ops.moe_combine(a["rows_in"], plan))

    (rows_a, tok_a), (rows_b, tok_b) = run(plan1, x1, G1, w1, one), run(plan2, x2, G2, w2, two)
    torch.cuda.synchronize()
    for key in rows_a:
        assert bool(torch.isfinite(rows_a[key][r1]).all()) and torch.equal(_bits(rows_a[key][r1]), _bits(rows_b[key][r2])), key
    for key in tok_a:
        assert torch.equal(_bits(tok_a[key]), _bits(tok_b[key][extra:])), key

    def chain(x, idx, w, G):
        x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
        out = MoEExpertsFn.apply(x, idx, w, Wgu, Wd, "silu")
        out.backward(G)
        torch.cuda.synchronize()
        return out.detach(), x.grad, w.grad

    a, b = chain(x1, idx1.cuda(), w1, G1), chain(x2, idx2.cuda(), w2, G2)
    for key, u, v in zip(("out", "G_x", "G_w"), a, b):
        assert bool(torch.isfinite(u).all()) and torch.equal(_bits(u), _bits(v[extra:])), key


@pytest.mark.parametrize("E", [1, 257, 1024])
@pytest.mark.parametrize("R", [255, 256, 257, 513])
def test_plan_at_its_chunk_and_scan_edges(ops, R, E):
    """one row short of, exactly and one row past one 256-row histogram chunk, and past two; E on both sides of the scan loops' strides (256
    threads per histogram block, 1024 in the scan block, MOE_EMAX = 1024).  As test_plan_is_a_stable_sort_of_the_expert_ids, plus toff"""
    gen = torch.Generator().manual_seed(R * 2048 + E)
    idx = torch.randint(0, E, (R, 1), generator=gen)
    idx[0], idx[R - 1], idx[R // 2] = E - 1, E - 1, 0                # the last expert in the first and in the last chunk
    dead = torch.randperm(R, generator=gen)[:R // 8]
    idx[dead, 0] = torch.tensor([-1, E, E + 5, -(2 ** 40), 2 ** 40])[torch.arange(dead.numel()) % 5]
    P = mb.Plan(idx, E)
    assert P.n == R - dead.numel()
    plan = ops.MoePlan(idx.cuda(), E)
    _plan_matches(plan, P)
    assert plan.buf[2 * E + 1:3 * E + 2].long().cpu().tolist() == [0] + torch.cumsum((P.cnt + 127) // 128, 0).tolist()
