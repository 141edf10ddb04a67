"""Element-wise rounding bounds for the decoder-family row and site kernels of csrc/rowops.hip, csrc/eltwise.hip, csrc/sandwich.hip (and
lrp_gqa_reduce_rope of csrc/attention.hip, which tests/attn_bound.py does NOT bound: it holds lrp_gqa_reduce and lrp_attn_bwd_prep only):
lrp_add_rmsnorm_fwd, lrp_rmsnorm_bwd_add2, lrp_rms_rstd, lrp_head_rmsnorm_fwd / _bwd, lrp_rope_fwd / _bwd, lrp_gated_act_fwd / _bwd with their
_il forms, lrp_gated_cp_bwd_il, lrp_add2_rule_bwd, lrp_sandwich_norm_fwd / _bwd, lrp_qk_norm_rope_fwd, lrp_qkv_bwd_pack.  Plain torch, any
device; used by tests/test_rowsite_bound_cpu.py (is the bound sound, does it discriminate, do the shapes reach what they claim) and
tests/test_rowsite_bound_gpu.py (the kernels against it).  Layout as tests/gemm_bound.py; check, ratio, rne, trunc, the bias statistic and
the activation's pieces (act64, act_arith) are tests/moe_bound.py's, imported.

Per operation there are two things, written apart and held against each other by the CPU test:

  REFERENCES (header_*): the formula of include/lrp_hip.h in fp64 on the STORED inputs, no intermediate rounded.  The stabiliser constants and
  the norm eps enter as the fp32 values the C ABI receives (f32c).

  TRACES (trace_*): the kernel's sequence of fp32 operations, written once over a number type.  Run on V it carries, next to the fp64 value
  of the same expression (which must equal the header's: test (a) asserts it), a WORST-CASE bound on how far the kernel's fp32 value can
  lie from it; run on X it is the torch model of the kernel's arithmetic (fp32, storage round trips exactly where the kernel stores), in
  which the structural faults are planted.

u is the largest relative error of ONE round-to-nearest store: 2^-8 for bf16 storage, f for fp32 storage.  f = 2^-24 is one fp32 operation.
Every bound ends in the form e + u (|ref| + e) of tests/gemm_bound.py, e the fp32 error of the value before its store.  V's rules (no
fitted constant: every term is u, f, a reduction length or a count of roundings):

    x + y, x y      : the operands' errors propagated exactly (|x| e_y + |y| e_x + e_x e_y for the product), then one rounding f (|v| + e)
    x / y           : (e_x + |x / y| e_y) / (|y| - e_y), then one rounding (IEEE division); the v_rcp_f32 form a rcp(b) of bf16 storage
                      (csrc/common.hpp:154, :161): three (rcp 2 f, the product f)
    rsqrt(x)        : 1/2 e_x (x - e_x)^-3/2, then 2 f
    sum of n terms  : the terms' errors, then (n + 8) f over the absolute sum -- n - 1 additions IN ANY ORDER (lane partials, shuffles, LDS) and
                      8 f of head room for the second order, as the K-term sums of tests/moe_bound.py
    store           : e + u (|v| + e)
    act(g)          : moe_bound.act_arith at the stored g (E_g = 0)

The rounding points, read out of the kernels (paths below lrp-explains-transformers_amd/csrc/):

  lrp_add_rmsnorm_fwd      rowops.hip:47, :64   the residual add h + branch ROUNDED TO STORAGE before the sum of squares (and before y)
                           rowops.hip:51, :53   H squares and their sum, in the order of the lanes, the shuffles and the 1 or 4 waves (common.hpp:102-121)
                           rowops.hip:54        ss / H (one division), + eps, one rsqrtf; rstd stored as fp32
                           rowops.hip:68        w_offset == 0 (HF Llama): (x rstd) rounded to storage, THEN times w
                           rowops.hip:69        w_offset != 0 (Gemma-3): (x rstd) (w_offset + w) in fp32: two products, one addition
                           rowops.hip:71        the store of y
  lrp_rmsnorm_bwd_add2     rowops.hip:93-94     Gx (w + w_offset) rstd: an addition and two products; + Gres
                           rowops.hip:95, :107  rel: H products hsum Gh and their sum
                           rowops.hip:98-99     eps_ratio (common.hpp:135-138): z / (1 z + eps): an addition, an IEEE division; the product.  A is
                                                formed from the UNROUNDED Gs
                           rowops.hip:103-104   the two stores
  lrp_rms_rstd             rowops.hip:446, :449 `parts` additions, the host's 1 / H (rowops.hip:455: one division), a product, + eps, rsqrtf
  lrp_head_rmsnorm_fwd     rowops.hip:384-386, :389-390, :392   as lrp_add_rmsnorm_fwd without a residual, d terms per (row, head)
  lrp_head_rmsnorm_bwd     rowops.hip:409-410   G (w + w_offset) rstd, one store
  lrp_rope_fwd             eltwise.hip:305-306  two products and one addition per output; :308-309 the store
  lrp_rope_bwd             eltwise.hip:338      Gr times eps_ratio(xr) (eps_rope != 0)        :339-340 two products and one addition
                           eltwise.hip:341      times eps_ratio(x) (eps_lin != 0)               :345-346 the store
  lrp_gated_act_fwd[_il]   eltwise.hip:197      act(g) ROUNDED TO STORAGE before the product     :198 the product   :200 the store
  lrp_gated_act_bwd[_il]   bf16: common.hpp:189 act(g) rounded to bf16; :190 g + eps_g; LEAN (eps_g >= 1e-30 and eps_lin == 0, eltwise.hip:219):
                           :192 y rcp(den), :193 (1/2 Gm) u q, :194 (1/2 Gm) y; general: :196 fdiv_small_t (a power-of-two rescue of a denormal
                           denominator: no rounding more), :197 eps_ratio_t = u rcp(u + eps_lin), exactly 1 for eps_lin = 0
                           fp32: eltwise.hip:229 act(g) NOT rounded, :231-233 IEEE divisions                 eltwise.hip:236-237 the stores
  lrp_gated_cp_bwd_il      eltwise.hip:257 act(g) rounded to storage, :259 the product, :258 exact zeros in the gate slots, :261-262 the stores
  lrp_add2_rule_bwd        eltwise.hip:107-109  a + b, + eps, the division, one product each; :111-112 the stores
  lrp_sandwich_norm_fwd    sandwich.hip:64, :67-68 rstd_post as above;  :80 the post-norm's output rounded to storage (norm_scale :34-36 in either
                           convention);  :81 res + that, rounded to storage;  :82, :87-88 rstd_pre from the STORED sums;  :98-99 y
  lrp_sandwich_norm_bwd    sandwich.hip:122-124 Gs = T(Gx (w_pre + w_offset) rstd_pre + Gres);  :126 Ga from the ROUNDED Gs;  :128-129 the stores
  lrp_qk_norm_rope_fwd     sandwich.hip:152-154 rstd per (row, head);  :165 the normed head rounded to storage;  :167 RoPE on it;  :169-170 the store
  lrp_qkv_bwd_pack         sandwich.hip:204, :207 the group sum: `rep` additions, rounded to storage;  :222 RoPE's transpose, rounded to storage;
                           :223 (w + w_offset) rstd;  :209, :225 the stores
  lrp_gqa_reduce_rope      attention.hip:954 the group sum in fp32, NOT rounded;  :961-962 RoPE's transpose;  :965-966 the store

ASSUMED, not measured (as tests/moe_bound.py): v_rsq_f32 (rsqrtf), v_rcp_f32 and v_exp_f32 are accurate to 1 ulp = 2 f each; the fp32-storage
tanh-GELU goes through the math library's tanhf at OpenCL's published 5 ulp = 10 f (inside moe_bound.act_arith).  `/` on floats is the
correctly rounded IEEE division (the compiler's default for HIP).  Nothing else is assumed.

NEAR A POLE.  Every stabiliser quotient of these kernels -- z / (z + eps), act(g) / (g + eps_g) -- takes its z or g FROM MEMORY: the operand
is exact, fl(z + eps) is one rounding of the exact sum whatever cancels in it, and the quotient therefore carries a RELATIVE error of a few f
everywhere, the neighbourhood of the pole included.  No floor is needed for them and none is used.  The one denominator that is computed
from a rounded intermediate is lrp_add2_rule_bwd's fl(fl(a + b) + eps): its bound holds where |a + b + eps| > f |a + b| (V.div: the
denominator's own error must not reach it) and is infinite elsewhere; the share left out is capped at moe_bound.EXCLUDED_CAP per output and
case and asserted, and what is left out must still be finite or the header's own +-inf.  Exact zeros are planted and asserted: zero rows
(every output of the row is 0), g = 0 (act(0) = 0), z = 0 under a stabiliser (0 / eps = 0), and g = -eps_g where the storage type can hold
it (fp32; bf16(1e-10) is not 1e-10), for which the header defines the result 0.  Sites where the header defines NO value at a zero
denominator -- nothing is planted there -- are listed in DESIGN.md.

The CPU model stays within these forms on every case, so no term was added because a bound was exceeded."""
import math

import torch

from tests import moe_bound as mb
from tests.attn_bound import bias as signed_bias      # noqa: F401  (re-exported with the rest: the tests take everything from here)
from tests.moe_bound import ACTS, EXCLUDED_CAP, F, U, check, ratio, rne, trunc, unit      # noqa: F401

BF16, F32 = torch.bfloat16, torch.float32
SMALL = 2.0 ** -6         # scale of the rows / heads the structural faults are planted on
STABS = ((1e-10, 0.0), (1e-8, 1e-8), (0.0, 0.0))          # (eps_g, eps_lin): lxt.efficient (the LEAN form), lxt.explicit, no stabiliser
NORM_EPS = 1e-6


def act64(g, act):
    """moe_bound.act64, with the tanh-GELU in its equal form g sigmoid(2 z) (0.5 (1 + tanh z) = sigmoid(2 z)): 1 + tanh z cancels in fp64 itself
    for g < -6 (3.5 % at g = -7, where 1 + tanh z = 1e-15), which the gates of this module's cases reach and those of tests/moe_bound.py do not"""
    if act == "silu":
        return mb.act64(g, act)
    return g * torch.sigmoid(2.0 * mb.K0 * (g + mb.K1 * g ** 3))


def f32c(x):
    """a Python float as the fp32 value the C ABI receives"""
    return float(torch.tensor(x, dtype=torch.float32))


def epc(dtype):
    return 16 // (2 if dtype == BF16 else 4)


def cdiv(a, b):
    return -(-a // b)


# ---- the host rules, mirrored (tests/test_rowsite_bound_cpu.py holds them against the library's own answer where it exports one) -------------
def row_threads(H, W):
    """csrc/rowops.hip:11, csrc/sandwich.hip:16"""
    return 64 if H // W <= 64 else 256


def row_plan(H, dtype, aligned=True):
    """lrp_add_rmsnorm_fwd / lrp_rmsnorm_bwd_add2 (csrc/rowops.hip:428-430, :470-472) -> (W, threads, passes of the block over the row, is the last
    pass uneven)"""
    W = epc(dtype) if aligned and H % epc(dtype) == 0 else 1
    nt = row_threads(H, W)
    chunks = cdiv(H, W)
    return W, nt, cdiv(chunks, nt), chunks % nt != 0


def grid_for(work):
    """csrc/eltwise.hip:10-13: blocks of 256 threads, at most 2048"""
    return max(1, min(2048, cdiv(work, 256)))


def elt_plan(work_elems, dtype, vec):
    """the 2-D element-wise kernels (gated, RoPE; work = elements one thread-iteration covers times their count) -> (W, blocks, trips)"""
    W = epc(dtype) if vec else 1
    chunks = work_elems // W
    g = grid_for(chunks)
    return W, g, cdiv(chunks, g * 256)


def group_plan(groups, d, dtype, cap):
    """the lane-group kernels (per-head norms: cap 8192, csrc/rowops.hip:606-608; q/k site kernels: cap 16384, csrc/sandwich.hip:301-303) ->
    (lanes per group, blocks, trips)"""
    lpg = d // epc(dtype)
    gpb = 256 // lpg
    nb = min(cap, cdiv(groups, gpb))
    return lpg, nb, cdiv(groups, nb * gpb)


def head_shape_ok(d, dtype, least=1):
    lpg = d // epc(dtype)
    return d % epc(dtype) == 0 and least <= lpg <= 64 and lpg & (lpg - 1) == 0


def sandwich_ok(H, dtype):
    """lrp_sandwich_norm_ok (csrc/sandwich.hip:249-253)"""
    W = epc(dtype)
    return H >= W and H % W == 0 and cdiv(H // W, row_threads(H, W)) <= 4


def sandwich_chunks(H, dtype):
    """(threads, chunks a thread needs, the kernel's CH, is some thread's last chunk idle) of launch_sandwich_fwd (csrc/sandwich.hip:233-238)"""
    W = epc(dtype)
    nt = row_threads(H, W)
    need = cdiv(H // W, nt)
    ch = 1 if need <= 1 else 2 if need <= 2 else 4
    return nt, need, ch, (H // W) % nt != 0 or need != ch


def sandwich_bwd_plan(M, H, dtype):
    chunks = M * (H // epc(dtype))
    nb = min(16384, cdiv(chunks, 256))
    return nb, cdiv(chunks, nb * 256)


# ---- the two number types --------------------------------------------------------------------------------------------------------------------
def _t(x, like):
    return x if torch.is_tensor(x) else torch.tensor(float(x), dtype=like.dtype, device=like.device)


class V:
    """fp64 value v of an expression and a bound e on |the kernel's fp32 value - v| (module docstring)"""

    def __init__(self, v, e=None):
        self.v, self.e = v, (torch.zeros_like(v) if e is None else e)

    def _of(self, o):
        return o if isinstance(o, V) else V(_t(o, self.v))

    def _r(self, v, e, n=1):
        return V(v, e + n * F * (v.abs() + e))

    def __add__(self, o):
        o = self._of(o)
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = self._of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = self._of(o)
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def half(self):
        return V(0.5 * self.v, 0.5 * self.e)

    def div(self, o, fast=False):
        o = self._of(o)
        bmin = o.v.abs() - o.e
        q = self.v / torch.where(o.v == 0, torch.ones_like(o.v), o.v)
        e = torch.where(bmin > 0, (self.e + q.abs() * o.e) / bmin.clamp_min(1e-300), torch.full_like(q, math.inf))
        return self._r(q, e, 3 if fast else 1)

    def rsqrt(self):
        lo = (self.v - self.e).clamp_min(1e-300)
        return self._r(self.v ** -0.5, 0.5 * self.e * lo ** -1.5, 2)

    def sum(self, n):
        return V(self.v.sum(-1, keepdim=True), self.e.sum(-1, keepdim=True) + (n + 8) * F * (self.v.abs() + self.e).sum(-1, keepdim=True))

    def st(self, u):
        return V(self.v, self.e + u * (self.v.abs() + self.e))

    def zero_where(self, m):
        return V(torch.where(m, torch.zeros_like(self.v), self.v), torch.where(m, torch.zeros_like(self.e), self.e))

    def is0(self):
        return self.v == 0

    def map(self, fn):
        return V(fn(self.v), fn(self.e))

    def val(self):
        return self.v


class X:
    """the same operations as the kernel runs them: fp32 torch, `rnd` (rne, or trunc for the bias statistic) where it stores bf16"""

    def __init__(self, x, rnd):
        self.x, self.rnd = x, rnd

    def _of(self, o):
        return o.x if isinstance(o, X) else _t(o, self.x)

    def __add__(self, o):
        return X(self.x + self._of(o), self.rnd)

    def __sub__(self, o):
        return X(self.x - self._of(o), self.rnd)

    def __mul__(self, o):
        return X(self.x * self._of(o), self.rnd)

    def half(self):
        return X(0.5 * self.x, self.rnd)

    def div(self, o, fast=False):
        o = self._of(o)
        return X(self.x * (torch.ones_like(o) / o) if fast else self.x / o, self.rnd)

    def rsqrt(self):
        return X(torch.rsqrt(self.x), self.rnd)

    def sum(self, n):
        return X(self.x.sum(-1, keepdim=True), self.rnd)

    def st(self, u):
        return X(self.rnd(self.x), self.rnd)

    def zero_where(self, m):
        return X(torch.where(m, torch.zeros_like(self.x), self.x), self.rnd)

    def is0(self):
        return self.x == 0

    def map(self, fn):
        return X(fn(self.x), self.rnd)

    def val(self):
        return self.x.double()


def cat(parts, dim=-1):
    if isinstance(parts[0], V):
        return V(torch.cat([p.v for p in parts], dim), torch.cat([p.e for p in parts], dim))
    return X(torch.cat([p.x for p in parts], dim), parts[0].rnd)


class Ctx:
    """dtype, u and the number type of one run of a trace: Ctx(dtype) bounds, Ctx(dtype, model=True[, rnd=trunc][, fault=...]) models"""

    def __init__(self, dtype, model=False, rnd=rne, fault=None):
        self.dtype, self.u, self.model, self.fault = dtype, unit(dtype), model, fault
        self.rnd = (rnd if dtype == BF16 else (lambda t: t))

    def lift(self, t):
        if t is None:
            return None
        return X(t.float(), self.rnd) if self.model else V(t.double())

    def const(self, x, like, rel=0.0):
        """a host constant as the kernel holds it in fp32 (rel: its own relative error against the header's value, e.g. the host's 1 / H)"""
        if self.model:
            return X(torch.tensor(x, dtype=torch.float32, device=like.device), self.rnd)
        v = torch.tensor(float(x), dtype=torch.float64, device=like.device)
        return V(v, rel * v.abs())

    def act(self, g, act):
        """act(g) at a stored g: csrc/common.hpp:141-144 (fp32 storage), :169-172 (bf16 storage)"""
        if not self.model:
            a = act64(g.v, act)
            return V(a, mb.act_arith(g.v.abs(), a.abs(), act, self.dtype))
        x, one = g.x, torch.ones((), device=g.x.device)
        if self.dtype == BF16:
            w = x if act == "silu" else (2.0 * mb.K0) * (x + mb.K1 * x * x * x)
            return X(x * (one / (one + torch.exp(-w))), self.rnd)
        if act == "silu":
            return X(x / (one + torch.exp(-x)), self.rnd)
        return X(0.5 * x * (one + torch.tanh(mb.K0 * (x + mb.K1 * x * x * x))), self.rnd)


def _ratio(c, z, eps):
    """eps_ratio(z, 1, eps) of csrc/common.hpp:135-138 for eps != 0"""
    return z.div(z + eps)


# ---- traces: the kernels' operation sequences ------------------------------------------------------------------------------------------------
def _norm_scale(c, x, r, w, w_off):
    """csrc/rowops.hip:68-69 = csrc/sandwich.hip:34-36"""
    if w_off == 0.0 or c.fault == "w_offset":
        return w * (x * r).st(c.u)
    return (x * r) * (w + w_off)


def _rstd(c, x, n, eps, skip=None):
    sq = x * x
    if skip is not None:          # (a planted fault: the columns from `skip` on are left out of the sum of squares)
        sq = sq.map(lambda t: torch.cat((t[..., :skip], torch.zeros_like(t[..., skip:])), -1))
    return (sq.sum(n).div(float(n)) + eps).rsqrt()


def _neighbour(c, r, d):
    """fault rstd_neighbour: the planted (small) rows / heads take the statistic of the row / head before them"""
    if c.fault != "rstd_neighbour":
        return r
    rows = d["small"]
    return r.map(lambda t: torch.index_put(t.clone(), (torch.tensor(rows, device=t.device),), t.roll(1, 0)[rows]))


def trace_add_rmsnorm_fwd(c, d):
    """h [M, H], branch or None, w [H]; d["hsum_out"], d["norm_out"] say what the caller asked for -> hsum, rstd [M, 1], y"""
    h, b, H, eps = c.lift(d["h"]), c.lift(d.get("branch")), d["h"].shape[1], f32c(d["eps"])
    s = h if b is None else (h + b).st(c.u)
    skip = H - H % (epc(c.dtype) * 256) if c.fault == "skip_ragged" else None
    r = _neighbour(c, _rstd(c, s, H, eps, skip), d)
    out = {"rstd": r}
    if d.get("hsum_out", True):
        out["hsum"] = s
    if d.get("norm_out", True):
        out["y"] = _norm_scale(c, s, r, c.lift(d["w"]), d["w_off"]).st(c.u)
        if skip is not None:
            out["y"] = out["y"].map(lambda t: torch.cat((t[..., :skip], torch.full_like(t[..., skip:], math.nan)), -1))
    return out


def trace_rmsnorm_bwd_add2(c, d):
    """Gres, Gx, w, rstd [M], hsum, branch (any may be None as the C entry allows), rel (bool) -> Gs, A, rel [M, 1]"""
    gh = None
    if d.get("Gx") is not None:
        r = _neighbour(c, c.lift(d["rstd"][:, None]), d)
        w = c.lift(d["w"])
        gh = c.lift(d["Gx"]) * (w if c.fault == "w_offset" else w + d["w_off"]) * r
    if d.get("Gres") is not None:
        gh = c.lift(d["Gres"]) if gh is None else gh + c.lift(d["Gres"])
    out = {}
    hs, br = c.lift(d.get("hsum")), c.lift(d.get("branch"))
    if d.get("rel"):
        out["rel"] = (hs * gh).sum(gh.val().shape[1])
    gs = gh
    if br is not None:
        if d["eps_add"]:
            gs = gh * _ratio(c, hs, f32c(d["eps_add"]))
        out["A"] = (gs * _ratio(c, br, f32c(d["eps_lin"])) if d["eps_lin"] else gs).st(c.u)
    out["Gs"] = gs.st(c.u)
    return out


def trace_rms_rstd(c, d):
    """ssq [parts, M] fp32 -> rstd [M, 1]"""
    s = c.lift(d["ssq"].T.contiguous())
    parts = s.val().shape[1]
    inv = c.const(1.0, d["ssq"]).div(float(d["H"]))
    return {"rstd": (s.sum(parts) * inv + f32c(d["eps"])).rsqrt()}


def trace_head_rmsnorm_fwd(c, d):
    """x [rows, heads, d], w [d] -> y, rstd [rows, heads, 1]"""
    x, n = c.lift(d["x"]), d["x"].shape[-1]
    r = _rstd(c, x, n, f32c(d["eps"]))
    if c.fault == "rstd_neighbour":
        r = r.map(lambda t: t.roll(1, 1) if t.shape[1] > 1 else t.roll(1, 0))
    return {"y": _norm_scale(c, x, r, c.lift(d["w"]), d["w_off"]).st(c.u), "rstd": r}


def trace_head_rmsnorm_bwd(c, d):
    w = c.lift(d["w"])
    return {"out": (c.lift(d["G"]) * (w if c.fault == "w_offset" else w + d["w_off"]) * c.lift(d["rstd"][..., None])).st(c.u)}


def _tables(c, d, rows):
    """cos / sin [seq, d] at the position r % seq of every row -> the four half tables [rows, 1, d / 2]"""
    seq = d["seq"]
    pos = torch.arange(rows, device=d["cos"].device) % seq
    if c.fault == "rope_pos":          # one position too far on the first two rows behind a sequence boundary (the rows of scale 2^-6)
        r = torch.arange(rows, device=pos.device)
        pos = torch.where((r >= seq) & (r < seq + 2), (pos + 1) % seq, pos)
    cs, sn = c.lift(d["cos"][pos][:, None]), c.lift(d["sin"][pos][:, None])
    hd = d["cos"].shape[1] // 2
    lo, hi = (lambda t: t[..., :hd]), (lambda t: t[..., hd:])
    return cs.map(lo), cs.map(hi), sn.map(lo), sn.map(hi)


def _halves(x):
    hd = x.val().shape[-1] // 2
    return x.map(lambda t: t[..., :hd]), x.map(lambda t: t[..., hd:])


def _rope(c, d, x):
    """x [rows, heads, d]: xr = x cos + rotate_half(x) sin"""
    c1, c2, s1, s2 = _tables(c, d, x.val().shape[0])
    x1, x2 = _halves(x)
    if c.fault == "rope_sign":
        return cat([x1 * c1 + x2 * s1, x2 * c2 - x1 * s2])
    return cat([x1 * c1 - x2 * s1, x2 * c2 + x1 * s2])


def _rope_t(c, d, p):
    """the transposed rotation: a1 = p1 cos1 + p2 sin2, a2 = p2 cos2 - p1 sin1"""
    c1, c2, s1, s2 = _tables(c, d, p.val().shape[0])
    p1, p2 = _halves(p)
    if c.fault == "rope_sign":
        return cat([p1 * c1 - p2 * s2, p2 * c2 + p1 * s1])
    return cat([p1 * c1 + p2 * s2, p2 * c2 - p1 * s1])


def trace_rope_fwd(c, d):
    return {"xr": _rope(c, d, c.lift(d["x"])).st(c.u)}


def trace_rope_bwd(c, d):
    p = c.lift(d["Gr"])
    if d["eps_rope"]:
        p = p * _ratio(c, c.lift(d["xr"]), f32c(d["eps_rope"]))
    a = _rope_t(c, d, p)
    if d["eps_lin"]:
        a = a * _ratio(c, c.lift(d["x"]), f32c(d["eps_lin"]))
    return {"A": a.st(c.u)}


def _gu(c, d):
    g, u = c.lift(d["g"]), c.lift(d["u"])
    if c.fault == "swap_gu":          # gate and up swapped inside the second 32-column interleave block
        j = slice(32, 64)
        ga, ua = g.x.clone(), u.x.clone()
        ga[:, j], ua[:, j] = u.x[:, j], g.x[:, j]
        g, u = X(ga, g.rnd), X(ua, u.rnd)
    return g, u


def trace_gated_fwd(c, d):
    g, u = _gu(c, d)
    return {"m": (c.act(g, d["act"]).st(c.u) * u).st(c.u)}


def trace_gated_bwd(c, d):
    g, u = _gu(c, d)
    gmh = c.lift(d["Gm"]).half()
    eps_g, eps_lin = f32c(d["eps_g"]), f32c(d["eps_lin"])
    den = g + eps_g
    den0 = den.is0()
    if c.dtype == BF16:
        y = c.act(g, d["act"]).st(c.u)
        q = y.div(den, fast=True).zero_where(den0)
        ag = (gmh * u * q).zero_where(den0)
        au = gmh * y
        if eps_lin:
            au = au * u.div(u + eps_lin, fast=True)
    else:
        y = c.act(g, d["act"])
        ag = (gmh * u * y.div(den)).zero_where(den0)
        au = gmh * y
        if eps_lin:
            au = au * _ratio(c, u, eps_lin)
    return {"Ag": ag.st(c.u), "Au": au.st(c.u)}


def trace_gated_cp(c, d):
    g = c.lift(d["g"])
    up = (c.act(g, d["act"]).st(c.u) * c.lift(d["Gm"])).st(c.u)
    return {"Ag": up.map(torch.zeros_like), "Au": up}


def trace_add2(c, d):
    a, b, R = c.lift(d["a"]), c.lift(d["b"]), c.lift(d["R"])
    s = R.div(a + b + f32c(d["eps"]))
    return {"Ra": (s * a).st(c.u), "Rb": (s * b).st(c.u)}


def trace_sandwich_fwd(c, d):
    """x, res [M, H], w_post, w_pre [H] -> rstd_post, hsum, rstd_pre, y"""
    x, H, eps = c.lift(d["x"]), d["x"].shape[1], f32c(d["eps"])
    skip = None
    if c.fault == "skip_ragged":          # the idle part of the last chunk round taken for the whole round
        nt, need, ch, _ = sandwich_chunks(H, c.dtype)
        skip = (need - 1) * nt * epc(c.dtype)
    ra = _neighbour(c, _rstd(c, x, H, eps, skip), d)
    pa = _norm_scale(c, x, ra, c.lift(d["w_post"]), d["w_off"]).st(c.u)
    hs = (c.lift(d["res"]) + pa).st(c.u)
    rh = _rstd(c, hs, H, eps)
    return {"rstd_post": ra, "hsum": hs, "rstd_pre": rh, "y": _norm_scale(c, hs, rh, c.lift(d["w_pre"]), d["w_off"]).st(c.u)}


def trace_sandwich_bwd(c, d):
    w_off = 0.0 if c.fault == "w_offset" else d["w_off"]
    gh = c.lift(d["Gx"]) * (c.lift(d["w_pre"]) + w_off) * _neighbour(c, c.lift(d["rstd_pre"][:, None]), d)
    if d.get("Gres") is not None:
        gh = gh + c.lift(d["Gres"])
    gs = gh.st(c.u)
    return {"Gs": gs, "Ga": (gs * (c.lift(d["w_post"]) + w_off) * c.lift(d["rstd_post"][:, None])).st(c.u)}


def trace_qk_norm_rope(c, d):
    """q [rows, nq, d], k [rows, nk, d] (the q and k heads of the fused projection output) -> qr, kr, rstd_q, rstd_k"""
    out = {}
    for n, w in (("q", "wq"), ("k", "wk")):
        x = c.lift(d[n])
        r = _rstd(c, x, d[n].shape[-1], f32c(d["eps"]))
        if c.fault == "rstd_neighbour":
            r = r.map(lambda t: t.roll(1, 1) if t.shape[1] > 1 else t.roll(1, 0))
        out["rstd_" + n] = r
        out[n + "r"] = _rope(c, d, _norm_scale(c, x, r, c.lift(d[w]), d["w_off"]).st(c.u)).st(c.u)
    return out


def _group_sum(c, x, rep, drop=False):
    """x [rows, nk rep, d] -> [rows, nk, d]: acc = 0; acc += x_j in order (the first addition is exact)"""
    rows, nh, dd = x.val().shape
    parts = [x.map(lambda t, j=j: t.reshape(rows, nh // rep, rep, dd)[:, :, j]) for j in range(rep - 1 if drop else rep)]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def trace_qkv_bwd_pack(c, d):
    """dq [rows, nq, d], dk_h, dv_h [rows, nq, d], rstd_q [rows, nq], rstd_k [rows, nk] -> Aq, Ak, Av"""
    rep = d["dq"].shape[1] // d["rstd_k"].shape[1]
    w_off = 0.0 if c.fault == "w_offset" else d["w_off"]
    drop = c.fault == "drop_replica"
    out = {"Av": _group_sum(c, c.lift(d["dv_h"]), rep, drop).st(c.u)}
    for n, p, w, r in (("Aq", c.lift(d["dq"]), "wq", "rstd_q"), ("Ak", _group_sum(c, c.lift(d["dk_h"]), rep, drop).st(c.u), "wk", "rstd_k")):
        a = _rope_t(c, d, p).st(c.u)
        out[n] = (a * (c.lift(d[w]) + w_off) * c.lift(d[r][..., None])).st(c.u)
    return out


def trace_gqa_reduce_rope(c, d):
    """x [rows, Hkv rep, d] -> out [rows, Hkv, d]"""
    return {"out": _rope_t(c, d, _group_sum(c, c.lift(d["x"]), d["rep"], c.fault == "drop_replica")).st(c.u)}


TRACES = {"add_rmsnorm_fwd": trace_add_rmsnorm_fwd, "rmsnorm_bwd_add2": trace_rmsnorm_bwd_add2, "rms_rstd": trace_rms_rstd,
          "head_rmsnorm_fwd": trace_head_rmsnorm_fwd, "head_rmsnorm_bwd": trace_head_rmsnorm_bwd, "rope_fwd": trace_rope_fwd,
          "rope_bwd": trace_rope_bwd, "gated_fwd": trace_gated_fwd, "gated_bwd": trace_gated_bwd, "gated_cp": trace_gated_cp, "add2": trace_add2,
          "sandwich_fwd": trace_sandwich_fwd, "sandwich_bwd": trace_sandwich_bwd, "qk_norm_rope": trace_qk_norm_rope,
          "qkv_bwd_pack": trace_qkv_bwd_pack, "gqa_reduce_rope": trace_gqa_reduce_rope}


# ---- the header's formulas in fp64 (include/lrp_hip.h; the reference project's lxt/efficient/patches.py:111-123, :145-157,
# lxt/explicit/functional.py:266-273, :430-459, lxt/explicit/models/llama.py:226-260) -------------------------------------------------------
def _q(z, eps):
    """the unsigned stabiliser z / (z + eps); eps == 0: no stabiliser at all (exactly 1)"""
    return z / (z + f32c(eps)) if eps else torch.ones_like(z)


def _rot64(x, d, transpose=False):
    rows, hd = x.shape[0], x.shape[-1] // 2
    pos = torch.arange(rows, device=x.device) % d["seq"]
    cs, sn = d["cos"].double()[pos][:, None], d["sin"].double()[pos][:, None]
    if not transpose:
        return x * cs + torch.cat((-x[..., hd:], x[..., :hd]), -1) * sn
    t = x * sn
    return x * cs + torch.cat((t[..., hd:], -t[..., :hd]), -1)


def _rms64(x, eps):
    return torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + f32c(eps))


def header(op, d):
    """-> {output: fp64 reference} of one case, from the header's formulas alone"""
    D = lambda k: None if d.get(k) is None else d[k].double()      # noqa: E731
    if op == "add_rmsnorm_fwd":
        s = D("h") + (D("branch") if d.get("branch") is not None else 0.0)
        r = _rms64(s, d["eps"])
        return {"hsum": s, "rstd": r, "y": (D("w") + d["w_off"]) * s * r}
    if op == "rmsnorm_bwd_add2":
        gh = (D("Gx") * (D("w") + d["w_off"]) * D("rstd")[:, None] if d.get("Gx") is not None else 0.0) + (D("Gres") if d.get("Gres") is not None else 0.0)
        out = {}
        if d.get("rel"):
            out["rel"] = (D("hsum") * gh).sum(-1, keepdim=True)
        gs = gh
        if d.get("branch") is not None:
            gs = gh * (_q(D("hsum"), d["eps_add"]) if d["eps_add"] else 1.0)
            out["A"] = gs * _q(D("branch"), d["eps_lin"])
        out["Gs"] = gs
        return out
    if op == "rms_rstd":
        return {"rstd": torch.rsqrt(D("ssq").sum(0)[:, None] / d["H"] + f32c(d["eps"]))}
    if op == "head_rmsnorm_fwd":
        r = _rms64(D("x"), d["eps"])
        return {"y": (D("w") + d["w_off"]) * D("x") * r, "rstd": r}
    if op == "head_rmsnorm_bwd":
        return {"out": D("G") * (D("w") + d["w_off"]) * D("rstd")[..., None]}
    if op == "rope_fwd":
        return {"xr": _rot64(D("x"), d)}
    if op == "rope_bwd":
        gp = D("Gr") * (_q(D("xr"), d["eps_rope"]) if d["eps_rope"] else 1.0)
        return {"A": _rot64(gp, d, True) * (_q(D("x"), d["eps_lin"]) if d["eps_lin"] else 1.0)}
    if op == "gated_fwd":
        return {"m": act64(D("g"), d["act"]) * D("u")}
    if op == "gated_bwd":
        g, u, a = D("g"), D("u"), act64(D("g"), d["act"])
        den = g + f32c(d["eps_g"])
        ag = 0.5 * D("Gm") * u * a / torch.where(den == 0, torch.ones_like(den), den)
        return {"Ag": torch.where(den == 0, torch.zeros_like(ag), ag), "Au": 0.5 * D("Gm") * a * (_q(u, d["eps_lin"]) if d["eps_lin"] else 1.0)}
    if op == "gated_cp":
        up = act64(D("g"), d["act"]) * D("Gm")
        return {"Ag": torch.zeros_like(up), "Au": up}
    if op == "add2":
        s = D("R") / (D("a") + D("b") + f32c(d["eps"]))
        return {"Ra": s * D("a"), "Rb": s * D("b")}
    if op == "sandwich_fwd":
        ra = _rms64(D("x"), d["eps"])
        hs = D("res") + (D("w_post") + d["w_off"]) * D("x") * ra
        rh = _rms64(hs, d["eps"])
        return {"rstd_post": ra, "hsum": hs, "rstd_pre": rh, "y": (D("w_pre") + d["w_off"]) * hs * rh}
    if op == "sandwich_bwd":
        gs = D("Gx") * (D("w_pre") + d["w_off"]) * D("rstd_pre")[:, None] + (D("Gres") if d.get("Gres") is not None else 0.0)
        return {"Gs": gs, "Ga": gs * (D("w_post") + d["w_off"]) * D("rstd_post")[:, None]}
    if op == "qk_norm_rope":
        out = {}
        for n, w in (("q", "wq"), ("k", "wk")):
            r = _rms64(D(n), d["eps"])
            out["rstd_" + n], out[n + "r"] = r, _rot64((D(w) + d["w_off"]) * D(n) * r, d)
        return out
    if op in ("qkv_bwd_pack", "gqa_reduce_rope"):
        gsum = lambda t, rep: t.reshape(t.shape[0], t.shape[1] // rep, rep, t.shape[2]).sum(2)      # noqa: E731
        if op == "gqa_reduce_rope":
            return {"out": _rot64(gsum(D("x"), d["rep"]), d, True)}
        rep = d["dq"].shape[1] // d["rstd_k"].shape[1]
        return {"Aq": _rot64(D("dq"), d, True) * (D("wq") + d["w_off"]) * D("rstd_q")[..., None],
                "Ak": _rot64(gsum(D("dk_h"), rep), d, True) * (D("wk") + d["w_off"]) * D("rstd_k")[..., None], "Av": gsum(D("dv_h"), rep)}
    raise KeyError(op)


def references(op, d):
    """-> {output: (ref, bound, zero, where)}: ref the header's formula, bound the trace's; zero = where the output must be an exact 0 (reference
    0 under a bound of 0); where = the elements the bound is held on (None: all)"""
    tr, hd = TRACES[op](Ctx(d["dtype"]), d), header(op, d)
    out = {}
    for n, t in tr.items():
        ref = hd[n]
        assert ref.shape == t.v.shape, (op, n, ref.shape, t.v.shape)
        where = torch.isfinite(t.e)
        out[n] = (ref, torch.nan_to_num(t.e, posinf=0.0), (ref == 0) & (t.e == 0), None if bool(where.all()) else where)
    return out


def model(op, d, rnd=rne, fault=None):
    """the kernel's arithmetic in fp32 torch -> {output: fp64}"""
    return {n: t.val() for n, t in TRACES[op](Ctx(d["dtype"], True, rnd, fault), d).items()}


def evaluate(op, d, outs, log=None, strict=True, tag="", only=None):
    """every output of one case against its bound (moe_bound.check: finite, inside the bound on every element, the exact zeros; prints the worst
    err / bound).  outs: {output: fp64 tensor shaped as the reference}.  The share of elements a bound is not held on is asserted under
    EXCLUDED_CAP.  -> {tag + output: worst err / bound}"""
    log = {} if log is None else log
    for n, (ref, bound, zero, where) in references(op, d).items():
        if n not in outs or (only is not None and n not in only):
            continue
        x = outs[n].reshape(ref.shape)
        if where is not None:          # (lrp_add2_rule_bwd next to its pole: the header's own quotient may be +-inf there)
            x = torch.where(where, x, torch.zeros_like(x))
            ref = torch.where(where, ref, torch.zeros_like(ref))
            if strict:
                left = float((~where).double().mean())
                print(f"  {tag}{n}: {100 * left:.3f} % of the elements sit next to the pole")
                assert left <= EXCLUDED_CAP, (n, left)
        check(tag + n, x, ref, bound, zero=zero, log=log, strict=strict, where=where)
    return log


def excluded(op, d):
    return {n: float((~v[3]).double().mean()) for n, v in references(op, d).items() if v[3] is not None}


def row_check(name, out, ref, bar):
    """the per-row check of tests/test_rowops_gpu.py::check(rows=True): max_row |out - ref| <= 4 bar max_row |ref| in every row whose reference
    is not all zero"""
    err, top = (out.double() - ref).abs().amax(-1), ref.abs().amax(-1)
    nz = top > 0
    worst = float((err[nz] / top[nz]).max()) if bool(nz.any()) else 0.0
    print(f"  {name}: worst row err / row max = {worst:.2e} (bar {4 * bar:.0e})")
    assert bool((err[nz] <= 4 * bar * top[nz]).all()), (name, worst)


def todays_bars(x, ref, mult, dtype):
    """would the bar of tests/test_kernels_gpu.py pass this output?  nmax = max |err| / max |ref| < mult TOL (TOL 2e-2 bf16, 2e-5 fp32; mult 1 for
    the forwards, 5 / 20 / 50 for the rule backwards) -> (passes, nmax)"""
    x, ref = x.double(), ref.double()
    if not bool(torch.isfinite(x).all()):
        return False, math.inf
    nm = float((x - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
    return nm < mult * (2e-2 if dtype == BF16 else 2e-5), nm


TODAY = {"add_rmsnorm_fwd": 1, "rmsnorm_bwd_add2": 5, "head_rmsnorm_fwd": 1, "head_rmsnorm_bwd": 1, "rope_fwd": 1, "rope_bwd": 5, "gated_fwd": 1,
         "gated_bwd": 20, "gated_cp": 20, "add2": 50, "sandwich_fwd": 1, "sandwich_bwd": 5, "qk_norm_rope": 1, "qkv_bwd_pack": 5,
         "gqa_reduce_rope": 5, "rms_rstd": 1}

FAULTS = {          # name -> {op: outputs it must drive out of the bound}
    "rstd_neighbour": {"add_rmsnorm_fwd": ("y",), "rmsnorm_bwd_add2": ("Gs",), "head_rmsnorm_fwd": ("y",), "sandwich_fwd": ("hsum",),
                       "sandwich_bwd": ("Gs", "Ga"), "qk_norm_rope": ("qr", "kr")},
    "w_offset": {"add_rmsnorm_fwd": ("y",), "rmsnorm_bwd_add2": ("Gs",), "head_rmsnorm_bwd": ("out",), "sandwich_bwd": ("Gs", "Ga"),
                 "qkv_bwd_pack": ("Aq", "Ak")},
    "rope_pos": {"rope_fwd": ("xr",), "rope_bwd": ("A",), "qk_norm_rope": ("qr", "kr"), "qkv_bwd_pack": ("Aq", "Ak"), "gqa_reduce_rope": ("out",)},
    "rope_sign": {"rope_fwd": ("xr",), "rope_bwd": ("A",), "qk_norm_rope": ("qr", "kr"), "qkv_bwd_pack": ("Aq", "Ak"), "gqa_reduce_rope": ("out",)},
    "swap_gu": {"gated_fwd": ("m",), "gated_bwd": ("Ag", "Au")},
    "skip_ragged": {"add_rmsnorm_fwd": ("rstd", "y"), "sandwich_fwd": ("rstd_post", "hsum")},
    "drop_replica": {"qkv_bwd_pack": ("Ak", "Av"), "gqa_reduce_rope": ("out",)},
}
# "second grid trip skipped" and "a truncating store" are planted by the CPU test itself: the first leaves the elements past a (shrunk) grid's
# first trip unwritten, the second is told by the bias statistic, not by the bound


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _rows(M):
    """(the small rows the faults are planted on, the zero row) of an M-row operand"""
    if M < 3:
        return [], None
    return [1], M // 2


def rope_tables(seq, d, gen):
    """fp32 [seq, d] tables at HF's angles; the two halves of a row are NOT equal (the second half's angles are offset): the header's tables are
    plain [seq, d] arrays and a kernel that read the wrong half would otherwise pass"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
    ang = torch.arange(seq, dtype=torch.float64)[:, None] * inv[None]
    emb = torch.cat((ang, ang + 0.3), -1)
    return emb.cos().float().contiguous(), emb.sin().float().contiguous()


def operands(op, dtype, **k):
    """seeded CPU operands of one case, rounded to dtype, in the LOGICAL shapes of the traces.  Row 1 (head 1 of every row for the per-head
    kernels) carries the scale 2^-6; row M // 2 is all zero where the op turns a zero row into exact zeros; single planted zeros elsewhere"""
    g = _seed(op, dtype, sorted(k.items()))
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    d = dict(op=op, dtype=dtype, small=[], zero_row=None, **k)
    w_small = lambda n: (rn(n) * (0.1 if k.get("w_off") else 1.0)).to(dtype)      # noqa: E731

    def rows2(M, H, zero=True):
        t = rn(M, H)
        small, z = _rows(M)
        for r in small:
            t[r] *= SMALL
        if zero and z is not None:
            t[z] = 0
        return t.to(dtype)

    if op in ("add_rmsnorm_fwd", "rmsnorm_bwd_add2", "sandwich_fwd", "sandwich_bwd"):
        M, H = k["M"], k["H"]
        d["small"], d["zero_row"] = _rows(M)
    if op == "add_rmsnorm_fwd":
        d.update(h=rows2(M, H), branch=rows2(M, H) if k.get("res", True) else None, w=w_small(H), eps=NORM_EPS)
    elif op == "rmsnorm_bwd_add2":
        sub = k["subset"]          # letters: r = Gres, x = Gx, h = hsum, b = branch, l = rel
        d.update(Gres=rows2(M, H) if "r" in sub else None, Gx=rows2(M, H) if "x" in sub else None, w=w_small(H) if "x" in sub else None,
                 rstd=(torch.rand(M, generator=g) + 0.5) if "x" in sub else None, hsum=rows2(M, H, False) if "h" in sub else None,
                 branch=rows2(M, H, False) if "b" in sub else None, rel="l" in sub)
        for t in (d["hsum"], d["branch"]):          # z = 0 under a stabiliser: the quotient is an exact 0
            if t is not None:
                t[0, H // 2] = 0
                if H > 2:
                    t[0, 0], t[0, 1] = 3e-8, -3e-8          # |z| of the stabiliser's own size: z / (z + 1e-8) = 0.75 and 1.5
    elif op == "rms_rstd":
        d.update(ssq=torch.rand(k["parts"], k["M"], generator=g) * 64, eps=NORM_EPS)
    elif op in ("head_rmsnorm_fwd", "head_rmsnorm_bwd"):
        rows, heads, dd = k["rows"], k["heads"], k["d"]
        x = rn(rows, heads, dd)
        x[:, heads - 1 if heads > 1 else 0][1::2] *= SMALL
        if rows >= 3:
            x[rows // 2] = 0
        d.update(w=w_small(dd), eps=NORM_EPS)
        if op == "head_rmsnorm_fwd":
            d["x"] = x.to(dtype)
        else:
            d.update(G=x.to(dtype), rstd=torch.rand(rows, heads, generator=g) + 0.5)
    elif op in ("rope_fwd", "rope_bwd", "gqa_reduce_rope"):
        rows, nh, dd, seq = k["rows"], k["nh"], k["d"], k["seq"]
        d["cos"], d["sin"] = rope_tables(seq, dd, g)
        x = rn(rows, nh * k.get("rep", 1), dd)
        x[seq:seq + 2] *= SMALL          # the first rows of the second prompt: where a position off by one shows
        if rows >= 3:
            x[rows - 1] = 0
        if op == "rope_fwd":
            d["x"] = x.to(dtype)
        elif op == "gqa_reduce_rope":
            d["x"] = x.to(dtype)
        else:
            sign = lambda: torch.where(rn(rows, nh, dd) < 0, -1.0, 1.0)      # noqa: E731
            d.update(Gr=x.to(dtype), xr=((torch.rand(rows, nh, dd, generator=g) + 0.05) * sign()).to(dtype),
                     x=((torch.rand(rows, nh, dd, generator=g) + 0.05) * sign()).to(dtype))
            d["xr"][0, 0, 0] = 0
            d["x"][0, 0, 1] = 0
            d["xr"][0, 0, 2], d["x"][0, 0, 3] = 3e-8, -3e-8          # |z| of the stabiliser's own size: z / (z + 1e-8) = 0.75 and 1.5
    elif op in ("gated_fwd", "gated_bwd", "gated_cp"):
        M, I = k["M"], k["I"]
        gg, uu = rn(M, I) * 2, rn(M, I)
        small, z = _rows(M)
        for r in small:
            gg[r] *= SMALL
            uu[r] *= SMALL
        gg[0, 0] = 0
        if z is not None:
            uu[z] = 0
        gg[0, 2], uu[0, 3] = -3e-8, -3e-8          # next to the poles g = -eps_g, u = -eps_lin of the explicit placement
        gg = gg.to(dtype)
        if dtype == F32 and k.get("eps_g"):
            gg[0, 1] = -f32c(k["eps_g"])          # g + eps_g == 0: the header's 0
        d.update(g=gg, u=uu.to(dtype), Gm=rows2(M, I, False))
    elif op == "add2":
        n = k["n"]
        sign = torch.where(rn(n) < 0, -1.0, 1.0)
        d.update(a=((torch.rand(n, generator=g) + 0.1) * sign).to(dtype)[None], b=((torch.rand(n, generator=g) + 0.1) * sign).to(dtype)[None],
                 R=rn(n).to(dtype)[None])
        d["a"][0, 0] = 0
        if n > 4:
            d["a"][0, 1] = -d["b"][0, 1]          # a + b = 0: the quotient is R / eps
        d["R"][0, n // 2] = 0
    elif op == "sandwich_fwd":
        d.update(x=rows2(M, H), res=rows2(M, H), w_post=w_small(H), w_pre=w_small(H), eps=NORM_EPS)
    elif op == "sandwich_bwd":
        d.update(Gx=rows2(M, H), Gres=rows2(M, H) if k.get("gres", True) else None, w_post=w_small(H), w_pre=w_small(H),
                 rstd_pre=torch.rand(M, generator=g) + 0.5, rstd_post=torch.rand(M, generator=g) + 0.5)
    elif op in ("qk_norm_rope", "qkv_bwd_pack"):
        rows, nq, nk, dd, seq = k["rows"], k["nq"], k["nk"], k["d"], k["seq"]
        d["cos"], d["sin"] = rope_tables(seq, dd, g)
        d.update(wq=w_small(dd), wk=w_small(dd), eps=NORM_EPS)

        def heads(n):
            t = rn(rows, n, dd)
            t[seq:seq + 2] *= SMALL
            if rows >= 3:
                t[rows - 1] = 0
            return t.to(dtype)
        if op == "qk_norm_rope":
            d.update(q=heads(nq), k=heads(nk))
        else:
            d.update(dq=heads(nq), dk_h=heads(nq), dv_h=heads(nq), rstd_q=torch.rand(rows, nq, generator=g) + 0.5,
                     rstd_k=torch.rand(rows, nk, generator=g) + 0.5)
    else:
        raise KeyError(op)
    return d


def to(d, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}


def bias_case(op, d):
    """is the signed-bias statistic admitted?  It reads the mean signed error of many independent bf16 roundings"""
    return d["dtype"] == BF16


def bias_view(op, t):
    """the elements the statistic is taken over: all, but for lrp_add2_rule_bwd without its two planted ones (a = 0 and a + b = 0: the second is
    R / eps, 1e8 times the rest, and the statistic's floor of 1e-3 max |ref| would leave it alone with its single rounding)"""
    return t[..., 2:] if op == "add2" else t


# ---- the shapes of tests/test_rowsite_bound_gpu.py (tests/test_rowsite_bound_cpu.py evaluates the host rules on them without a GPU) --------------
def width(k, dtype):
    """a row of k 16-byte chunks"""
    return k * epc(dtype)


# (chunks per row or a ragged width as -H, M, base off the 16-byte grid) -> what it reaches: (W is vector, threads, passes, uneven last pass)
ROW_WIDTHS = [(1, 3, False), (64, 130, False), (65, 3, False), (257, 1, False), (515, 3, False), (-101, 3, False), (-301, 130, False),
              (64, 3, True)]
ROW_REACH = {1: (True, 64, 1, True), 64: (True, 64, 1, False), 65: (True, 256, 1, True), 257: (True, 256, 2, True), 515: (True, 256, 3, True),
             -101: (False, 256, 1, True), -301: (False, 256, 2, True), "off": (False, 256, None, None)}
BWD_SUBSETS = ("rxhbl", "rhbl", "rx", "rxhl", "x", "rxhb")          # engine.py:1718, :1510, :1622, :1714, ops.head_norm_bwd, :1626
HEAD_CASES = [(77, 1, 1), (77, 3, 2), (77, 3, 16), (77, 1, 64), (5, 3, 64)]          # (rows, heads, d / EPC)
HEAD_BIG = (10923, 3, 64)          # rows heads = 32769 = 8192 (256 / 64) + 1: a second trip of the grid-stride loop for ONE group
ROPE_D = (16, 64, 128, 256)
ROPE_STABS = ((0.0, 0.0), (1e-8, 0.0), (0.0, 1e-8), (1e-8, 1e-8))
ROPE_ROWS, ROPE_SEQ, ROPE_NH = 79, 37, 3
GATED_I = (32, 96, 1024)
GATED_M = (5, 130)
SANDWICH_K = (8, 200, 300, 672, 1000, 1024)          # chunks per row: 64 threads; 1, 2, 3 (-> 4, ragged), 4 (ragged), 4 chunks per thread of 256
SANDWICH_REACH = {8: (64, 1, 1), 200: (256, 1, 1), 300: (256, 2, 2), 672: (256, 3, 4), 1000: (256, 4, 4), 1024: (256, 4, 4)}
SANDWICH_NO = 1025          # one step beyond the gate
QK_CASES = [(16, 2, 2), (64, 4, 1), (128, 8, 1), (256, 4, 1)]          # (d, nq, nk): nq / nk = 1, 4, 8, 4
QK_ROWS, QK_SEQ = 79, 37


def past_cap(kind, dtype):
    """the smallest case whose grid-stride loop makes a second trip, per kernel family -> the keyword arguments of operands()"""
    W = epc(dtype)
    if kind == "gated":          # 2048 x 256 chunks of I = 1024
        return dict(M=2048 * 256 * W // 1024 + 1, I=1024)
    if kind == "rope":           # chunks = rows nh (d / 2) / W
        return dict(rows=2048 * 256 * W // (8 * 64) + 1, nh=8, d=128, seq=2048)
    if kind == "add2":
        return dict(n=2048 * 256 * W + 3 * W + 3)
    if kind == "sandwich_bwd":   # 16384 x 256 chunks of rows of 1024 chunks
        return dict(M=16384 * 256 // 1024 + 1, H=1024 * W)
    if kind == "qk":             # 16384 blocks of 256 / lpg groups at d = 256: lpg = 32 (bf16) / 64 (fp32)
        lpg = 256 // W
        return dict(rows=cdiv(16384 * (256 // lpg) + 1, 5), nq=4, nk=1, d=256, seq=2048)
    raise KeyError(kind)


FWD_VARIANTS = {          # name -> (branch, hsum_out, norm_out, hsum_out is h itself)
    "plain": (False, False, True, False), "copy": (False, True, True, False), "res": (True, True, True, False),
    "inplace": (True, True, True, True), "nonorm": (True, True, False, False), "res_nohsum": (True, False, True, False)}


def _h(k, dtype):
    return -k if k < 0 else width(k, dtype)


def cases(dtype, family=None):
    """the cases of tests/test_rowsite_bound_gpu.py -> [(id, op, keyword arguments of operands(), placement)].  placement: off = every operand's base
    sits one element off the 16-byte grid; pad = elements added to every row pitch; big = past a grid cap (GPU only: the CPU test asserts its
    trip count and plants the skipped second trip on a small case)"""
    W, out = epc(dtype), []

    def add(fam, tag, op, place=None, **kw):
        if family is None or fam == family:
            out.append((f"{tag}", op, kw, {**dict(off=False, pad=0, big=False), **(place or {})}))

    for k, M, off in ROW_WIDTHS:
        H, pl = _h(k, dtype), dict(off=off)
        for w_off in (0.0, 1.0):
            for v, (res, hs, no, ip) in FWD_VARIANTS.items():
                add("rownorm", f"fwd-H{H}{'off' if off else ''}-M{M}-w{w_off:g}-{v}", "add_rmsnorm_fwd", pl, M=M, H=H, w_off=w_off, res=res, hsum_out=hs,
                    norm_out=no, inplace=ip)
            for sub in BWD_SUBSETS:
                for ea, el in (((0.0, 0.0), (1e-8, 0.0), (0.0, 1e-8), (1e-8, 1e-8)) if "b" in sub else ((0.0, 0.0),)):
                    add("rownorm", f"bwd-H{H}{'off' if off else ''}-M{M}-w{w_off:g}-{sub}-{ea:g}-{el:g}", "rmsnorm_bwd_add2", pl, M=M, H=H,
                        w_off=w_off, subset=sub, eps_add=ea, eps_lin=el)
    for parts, M in ((1, 1), (9, 70), (64, 130)):
        add("rownorm", f"rms_rstd-{parts}-{M}", "rms_rstd", parts=parts, M=M, H=64 * parts)
    for rows, heads, k in HEAD_CASES + [HEAD_BIG]:
        pl = dict(pad=2 * W, big=(rows, heads, k) == HEAD_BIG)
        for w_off in ((1.0,) if pl["big"] else (0.0, 1.0)):
            for op in ("head_rmsnorm_fwd", "head_rmsnorm_bwd"):
                add("head", f"{op[5:]}-r{rows}-h{heads}-d{k * W}-w{w_off:g}", op, pl, rows=rows, heads=heads, d=k * W, w_off=w_off)
    # RoPE: d / 2 off EPC (d = 8 in fp32, d = 8 and 24 in bf16), a pitch off EPC, a base off the grid: the scalar kernels
    rope = [(dd, dict()) for dd in ROPE_D] + [(8, dict()), (24, dict()), (64, dict(pad=3)), (64, dict(off=True))]
    for dd, pl in rope:
        tag = f"d{dd}{'-pad' + str(pl['pad']) if pl.get('pad') else ''}{'-off' if pl.get('off') else ''}"
        kw = dict(rows=ROPE_ROWS, nh=ROPE_NH, d=dd, seq=ROPE_SEQ)
        add("rope", f"rope_fwd-{tag}", "rope_fwd", pl, **kw)
        for er, el in ROPE_STABS:
            add("rope", f"rope_bwd-{tag}-{er:g}-{el:g}", "rope_bwd", pl, eps_rope=er, eps_lin=el, **kw)
        if (dd // 2) % W == 0 and not pl:
            add("rope", f"gqa_reduce_rope-{tag}", "gqa_reduce_rope", pl, rows=ROPE_ROWS, nh=2, rep=4, d=dd, seq=ROPE_SEQ)
    big = past_cap("rope", dtype)
    add("rope", "rope_fwd-big", "rope_fwd", dict(big=True), **big)
    add("rope", "rope_bwd-big", "rope_bwd", dict(big=True), eps_rope=1e-8, eps_lin=1e-8, **big)
    add("rope", "gqa_reduce_rope-big", "gqa_reduce_rope", dict(big=True), rep=2, **big)
    # the gated rule: split (two tensors), il (one interleaved tensor), cp
    for form in ("split", "il"):
        shapes = [(M, I, dict()) for I in GATED_I for M in GATED_M] + [(5, 96, dict(pad=3)), (5, 96, dict(off=True))] + ([(5, 25, dict())] if form == "split" else [])
        for M, I, pl in shapes:
            tag = f"{form}-M{M}-I{I}{'-pad' if pl.get('pad') else ''}{'-off' if pl.get('off') else ''}"
            for act in ACTS:
                add("gated", f"gated_fwd-{tag}-{act}", "gated_fwd", dict(form=form, **pl), M=M, I=I, act=act)
                for eg, el in STABS:
                    add("gated", f"gated_bwd-{tag}-{act}-{eg:g}-{el:g}", "gated_bwd", dict(form=form, **pl), M=M, I=I, act=act, eps_g=eg, eps_lin=el)
                if form == "il" and not pl:
                    add("gated", f"gated_cp-{tag}-{act}", "gated_cp", dict(form="il"), M=M, I=I, act=act)
    big = past_cap("gated", dtype)
    for form in ("split", "il"):
        add("gated", f"gated_fwd-{form}-big", "gated_fwd", dict(form=form, big=True), act="silu", **big)
        add("gated", f"gated_bwd-{form}-big", "gated_bwd", dict(form=form, big=True), act="silu", eps_g=1e-10, eps_lin=0.0, **big)
    add("gated", "gated_cp-il-big", "gated_cp", dict(form="il", big=True), act="gelu_tanh", **big)
    for n, off in ((1, False), (37, False), (4099, False), (4099, True)):
        add("add2", f"add2-n{n}{'-off' if off else ''}", "add2", dict(off=off), n=n, eps=1e-8)
    add("add2", "add2-big", "add2", dict(big=True), eps=1e-8, **past_cap("add2", dtype))
    for k in SANDWICH_K + (SANDWICH_NO,):
        for M, w_off in ((3, 1.0), (130, 0.0)) if k in (8, 300) else ((3, 1.0),):
            add("sandwich", f"sandwich_fwd-k{k}-M{M}-w{w_off:g}", "sandwich_fwd", M=M, H=k * W, w_off=w_off)
            for gres in (True, False):
                add("sandwich", f"sandwich_bwd-k{k}-M{M}-w{w_off:g}-{'res' if gres else 'nores'}", "sandwich_bwd", M=M, H=k * W, w_off=w_off, gres=gres)
    add("sandwich", "sandwich_bwd-big", "sandwich_bwd", dict(big=True), w_off=1.0, gres=True, **past_cap("sandwich_bwd", dtype))
    for dd, nq, nk in QK_CASES:
        for op in ("qk_norm_rope", "qkv_bwd_pack"):
            for w_off in (0.0, 1.0):
                add("qk", f"{op}-d{dd}-{nq}-{nk}-w{w_off:g}", op, dict(pad=2 * W), rows=QK_ROWS, nq=nq, nk=nk, d=dd, seq=QK_SEQ, w_off=w_off)
    for op in ("qk_norm_rope", "qkv_bwd_pack"):
        add("qk", f"{op}-big", op, dict(big=True), w_off=1.0, **past_cap("qk", dtype))
    return out


FAMILIES = ("rownorm", "head", "rope", "gated", "add2", "sandwich", "qk")
