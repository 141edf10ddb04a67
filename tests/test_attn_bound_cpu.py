"""Is the element-wise bound of tests/attn_bound.py sound, and does it discriminate?  No GPU: a torch model of the bf16 attention kernels'
arithmetic -- fp32 math with a bf16 rounding at exactly the rounding points listed in tests/attn_bound.py -- stands in for the kernels.

  a. soundness: on every case of tests/test_attn_bound_gpu.py the faithful model is within the bound of every output;
  b. discrimination: each planted fault (a mask or an index map applied to the model) is OUTSIDE the bound on at least one element of every output
     it touches, at every head dim and GQA ratio; which of them today's nmax bars (3e-2 / 9e-2 of the global maximum, 4 x that per 128-row block)
     would have let through is printed for the record;
  c. rounding mode: the magnitude bound cannot see truncation in place of round-to-nearest (the truncating model reaches about 1 of it), a signed
     mean relative error can.  Its bar is half the truncating model's value on the same case, computed here from the model; the test asserts that
     this bar is at least 3 x the round-to-nearest model's value.  S = 1 and the q_begin cases are too small for that margin (one key per row;
     dq with S - q_begin live rows) and are left out of the bias check only (tests/attn_bound.py: bias_case)."""
import pytest
import torch

from tests import attn_bound as ab
from tests.test_kernels_gpu import _intervals

BF = torch.bfloat16
rne, trunc, model, references, biases = ab.rne, ab.trunc, ab.model, ab.references, ab.biases


def operands(S, Hq, Hkv, d, q_begin=0, device="cpu"):
    """the draws of tests/test_kernel_edges_gpu.py::_qkv_slices (seed 1, one fused buffer) and its Go (seed 4, zero below q_begin)
    -> q, k, v, Go as bf16-valued fp32 [B, H, S, d]"""
    Bn = ab.B
    buf = torch.randn(Bn * S, (Hq + 2 * Hkv) * d + 64, generator=torch.Generator().manual_seed(1)).to(BF).to(device)
    Go = torch.randn(Bn * S, Hq * d, generator=torch.Generator().manual_seed(4)).to(BF).to(device)
    Go.view(Bn, S, Hq * d)[:, :q_begin] = 0
    h = lambda x, H: x.float().reshape(Bn, S, H, d).permute(0, 2, 1, 3)      # noqa: E731
    return h(buf[:, : Hq * d], Hq), h(buf[:, Hq * d: (Hq + Hkv) * d], Hkv), h(buf[:, (Hq + Hkv) * d: (Hq + 2 * Hkv) * d], Hkv), h(Go, Hq)


def case_vis(S, d, causal, window, kind, device="cpu"):
    """-> (vis without q_begin, does the dV-only kernel run: its head dims, causal, no window)"""
    row_iv = None
    if kind is not None:
        lo, hi, causal = _intervals(kind, ab.B, S)
        row_iv = (lo, hi)
    return ab.visible(ab.B, S, causal, window, row_iv, device=device), bool(d in ab.CP_DV_D and causal and not window)


def run_case(S, Hq, Hkv, d, mask, rnd=rne, strict=True, fault=None):
    """-> (ratios of attn_bound.evaluate, the model's outputs, the fp64 operands, vis, scale)"""
    name, causal, window, kind, q_begin = mask
    scale = d ** -0.5
    q, k, v, Go = operands(S, Hq, Hkv, d, q_begin)
    vis, cp = case_vis(S, d, causal, window, kind)
    i = torch.arange(S)
    vis_m, kw = vis & (i >= q_begin)[None, None, :, None], {}
    if fault is not None:
        vis_m, kw = fault(vis_m, S, Hq, Hkv)
    out = model(q, k, v, Go, vis_m, scale, rnd=rnd, cp=cp, **kw)
    ratios = ab.evaluate(out, q.double(), k.double(), v.double(), vis, scale, q_begin=q_begin, strict=strict)
    return ratios, out, (q.double(), k.double(), v.double()), vis, scale


# ------------------------------------------------------------------------------------------------------------------ a. soundness
@pytest.mark.parametrize("Hq,Hkv", ab.HEADS)
@pytest.mark.parametrize("d", ab.D_ALL)
def test_model_within_bound(d, Hq, Hkv):
    """the faithful model on every case of the GPU test: every output within its bound (attn_bound.check asserts it element-wise, with the exact
    zeros of the empty sums)"""
    worst = {}
    for S in ab.S_ALL:
        for mask in ab.masks(S):
            print(f"[d {d} heads {Hq}/{Hkv} S {S} {mask[0]}]")
            for key, r in run_case(S, Hq, Hkv, d, mask)[0].items():
                worst[key] = max(worst.get(key, 0.0), r)
    print(f"model d {d} heads {Hq}/{Hkv}: worst err / bound per output: " + " ".join(f"{k_} {r:.3f}" for k_, r in worst.items()))


def test_exp2_of_the_model():
    """the exp2 that the MODEL uses (torch's fp32 exp2 on the host) against fp64 over the exponents the cases produce, [-60, 8] (8: the lazy
    maximum's 2^8): within 2 f element-wise, so the model's own exp2 takes no more of E_s's 8 roundings than the 1 ulp assumed for v_exp_f32.
    This says nothing about the hardware instruction: its accuracy is an assumption of tests/attn_bound.py, held to account by the GPU test alone."""
    x = torch.linspace(-60, 8, 2_000_001, dtype=torch.float32)
    e = float(((torch.exp2(x).double() - torch.exp2(x.double())).abs() / torch.exp2(x.double())).max())
    print(f"the model's fp32 exp2 vs fp64: max relative error {e:.2e} = {e / ab.F:.2f} f")
    assert e <= 2 * ab.F


# -------------------------------------------------------------------------------------------------------------- b. discrimination
FWD, BWD, CP = ("o",), ("dq", "dk_h", "dv_h", "dk", "dv"), ("cp_dv",)
S_FAULT = 300
CAUSAL, FULL, W48 = ("causal", True, 0, None, 0), ("full", False, 0, None, 0), ("w48", True, 48, None, 0)
RANDOM, QB37 = ("random", None, 0, "random", 0), ("qb37", True, 0, None, 37)


def _edit(fn):
    """a fault that rewrites the mask: fn(vis [B, 1, S, S] clone, i [S, 1], j [1, S]) -> vis"""
    def fault(vis, S, Hq, Hkv):
        i = torch.arange(S)
        return fn(vis.clone(), i[:, None], i[None, :]), {}
    return fault


def _f_tile_skipped(vis, i, j):
    vis &= ~((i >= 256) & (j < 64))                                   # the query block from row 256 on never visits key tile [0, 64)
    return vis


def _f_diag_block_end(vis, i, j):
    vis &= ~((i == j) & (i % 32 == 31))
    return vis


def _f_last_key(vis, i, j):
    vis &= j != vis.shape[-1] - 1                                     # S = 300: key 299, the last of the partial tile [256, 300)
    return vis


def _f_causal_strict(vis, i, j):
    vis &= j < i
    return vis


def _f_window(w):
    def fn(vis, i, j):
        return ((j <= i) & (j > i - w))[None, None].expand_as(vis).clone()
    return fn


def _f_hi_inclusive(vis, i, j):
    lo, hi, _ = _intervals("random", ab.B, vis.shape[-1])
    return ((j[None] >= lo[:, :, None]) & (j[None] <= hi[:, :, None]))[:, None]


def _f_q_begin(vis, i, j):
    vis &= i >= 38                                                    # q_begin = 37 taken for 38: row 37 is skipped
    return vis


def _f_neighbour_kv(vis, S, Hq, Hkv):
    kv_map = torch.arange(Hq) // (Hq // Hkv)
    kv_map[Hq // Hkv - 1] = 1                                         # the last head of group 0 reads kv head 1
    return vis, dict(kv_map=kv_map)


def _f_dv_head_dropped(vis, S, Hq, Hkv):
    return vis, dict(dv_skip=Hq // Hkv - 1)                           # the last head of group 0 is not summed into dv


FAULTS = [
    ("a key tile skipped for a later query block", CAUSAL, _edit(_f_tile_skipped), FWD + BWD + CP),
    ("the diagonal key dropped on the last row of each 32-row block", CAUSAL, _edit(_f_diag_block_end), FWD + BWD + CP),
    ("the last key of a partial tile dropped", FULL, _edit(_f_last_key), FWD + BWD),
    ("causal < in place of <=", CAUSAL, _edit(_f_causal_strict), FWD + BWD + CP),
    ("window one too wide", W48, _edit(_f_window(49)), FWD + BWD),
    ("window one too narrow", W48, _edit(_f_window(47)), FWD + BWD),
    ("row_hi treated as inclusive", RANDOM, _edit(_f_hi_inclusive), FWD + BWD),
    ("q_begin off by one row", QB37, _edit(_f_q_begin), FWD + BWD + CP),
    ("a query head reads the neighbouring kv head", CAUSAL, _f_neighbour_kv, FWD + BWD + CP),
    ("a head left out of the dv group sum", CAUSAL, _f_dv_head_dropped, ("dv",) + CP),
]


def _todays_bars(out, refs, S):
    """would today's checks pass?  nmax < 3e-2 (o) / 9e-2 (dq, dk, dv) AND, as tests/test_kernel_edges_gpu.py::_check, 4 x that per (head, 128-row
    block) of the block's own maximum -> {name: (passes nmax, passes both)}"""
    res = {}
    for name, bar in (("o", 3e-2), ("dq", 9e-2), ("dk", 9e-2), ("dv", 9e-2), ("cp_dv", 9e-2)):
        if name not in out or name not in refs:
            continue
        x, ref = out[name], refs[name]
        err, top = (x - ref).abs().amax(-1), ref.abs().amax(-1)
        pad = (-S) % 128
        blk = lambda t: torch.nn.functional.pad(t, (0, pad)).reshape(*t.shape[:2], -1, 128).amax(-1)      # noqa: E731
        glob = bool(err.max() < bar * ref.abs().max())
        res[name] = (glob, glob and bool((blk(err) <= 4 * bar * blk(top)).all()))
    return res


@pytest.mark.parametrize("Hq,Hkv", ab.HEADS)
@pytest.mark.parametrize("d", ab.D_ALL)
def test_planted_faults_exceed_bound(d, Hq, Hkv):
    """each fault of FAULTS, planted into the model at S = 300 (three 128-row blocks, a partial tile, rows past 256): some element of every
    output it touches is outside the bound.  Printed, not asserted: which of them today's nmax bars would have let through."""
    let_through = []
    for title, mask, fault, touched in FAULTS:
        ratios, out, (q, k, v), vis, scale = run_case(S_FAULT, Hq, Hkv, d, mask, strict=False, fault=fault)
        touched = [t for t in touched if t in ratios]
        print(f"[d {d} heads {Hq}/{Hkv}] {title}: " + " ".join(f"{t} {ratios[t]:.1f}" for t in touched))
        for t in touched:
            assert ratios[t] > 1.0, (title, t, ratios[t])
        # today's bars against the same fp64 references
        vis_b = vis & (torch.arange(S_FAULT) >= mask[4])[None, None, :, None]
        for name, (glob, both) in _todays_bars(out, references(out, q, k, v, vis_b, scale), S_FAULT).items():
            if name in touched and glob:
                let_through.append(f"{title} / {name}" + ("" if both else " (nmax only: the per-block bar catches it)"))
    print(f"[d {d} heads {Hq}/{Hkv}] passes today's nmax bars: " + ("; ".join(let_through) if let_through else "none"))


# --------------------------------------------------------------------------------------------------------------- c. rounding mode
BIAS_OUT = ("o", "dq", "dk", "dv", "cp_dv")


def model_bias(S, Hq, Hkv, d, mask, rnd):
    _, out, (q, k, v), vis, scale = run_case(S, Hq, Hkv, d, mask, rnd=rnd, strict=False)
    return biases(out, q, k, v, vis, scale)


def bias_bars(S, Hq, Hkv, d, mask):
    """-> {output: half the truncating model's |bias|} on this case, in units of u: computed from the model, not typed in"""
    return {name: 0.5 * abs(b) for name, b in model_bias(S, Hq, Hkv, d, mask, trunc).items()}


@pytest.mark.parametrize("Hq,Hkv", ab.HEADS)
@pytest.mark.parametrize("d", ab.D_ALL)
def test_bias_tells_truncation(d, Hq, Hkv):
    """on every admitted case (attn_bound.bias_case) the bar -- half the truncating model's bias -- is at least 3 x the round-to-nearest model's"""
    worst = {}
    for S in ab.S_ALL:
        for mask in ab.masks(S):
            if not ab.bias_case(S, mask):
                continue
            bars, near = bias_bars(S, Hq, Hkv, d, mask), model_bias(S, Hq, Hkv, d, mask, rne)
            print(f"[d {d} heads {Hq}/{Hkv} S {S} {mask[0]}] bar / round-to-nearest model, in u: " +
                  " ".join(f"{n} {bars[n]:.3f} / {near[n]:+.3f}" for n in bars))
            for name, bar in bars.items():
                assert bar >= 3 * abs(near[name]), (S, mask[0], name, bar, near[name])
                worst[name] = max(worst.get(name, 0.0), abs(near[name]))
    print(f"model d {d} heads {Hq}/{Hkv}: largest round-to-nearest |bias| per output, in u: " + " ".join(f"{n} {b:.3f}" for n, b in worst.items()))
