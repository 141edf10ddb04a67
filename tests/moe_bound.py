"""Element-wise rounding bounds for the routed-expert kernels of csrc/moe.hip / csrc/moe_gemm.hpp (the four grouped GEMMs, lrp_moe_combine,
lrp_moe_gw_reduce): per operation an fp64 reference on the ROUNDED inputs, next to it the magnitude of the same sum taken over absolute values,
and from the two a WORST-CASE bound on what the kernel's roundings can do to that element.  Plain torch, any device; used by
tests/test_moe_bound_cpu.py (is the bound sound, does it discriminate) and tests/test_moe_ops_gpu.py (the kernels against it).  Layout as
tests/attn_bound.py.

u is the largest relative error of ONE round-to-nearest store: 2^-8 for bf16 storage, f for fp32 storage.  f = 2^-24 is one fp32 operation.
Every bound has the form

    e + u (|ref| + e),        e = the fp32 error of the value before its store

(the store rounds the computed value, |ref| + e at most, not the reference: that is the only change to the forms `u |ref| + e` the work
started from, and it is second order).  No term carries a fitted constant: the factors are u, f, the contraction length, counts of roundings
and the Lipschitz constants derived below.

The rounding points, read out of the kernels (paths below lrp-explains-transformers_amd/):

  the K-term MFMA sum in fp32: (K + 8) f A, A the same sum over absolute values (K sequential fp32 additions, 8 f of head room for the second
  order of (1 + f)^K at K <= 2048)
      csrc/moe_gemm.hpp:245            acc = mma(fa, fb, acc), all four operations
  EP_STORE (down_fwd y, K = I; gate_up_dgrad gx_rows, K = 2 I): one store
      csrc/moe_gemm.hpp:260            from_f32<T>(acc)
  EP_COEF (gate_up_fwd): g, u are accumulators with E_g = (H + 8) f A_g, E_u = (H + 8) f A_u
      csrc/moe_gemm.hpp:278            bf16 storage: gated_coef<true, ACT> (csrc/common.hpp:205-212) on act_apply_t<true> (csrc/common.hpp:169, :172):
                                       y = g rcp(1 + exp(-w)), w = g (SiLU) or 2 k0 (g + k1 g^3) (tanh-GELU as x sigmoid(2 z)); m = y u;
                                       q = (y / 2) rcp(g + 1e-10); cg = u q; cu = y / 2
      csrc/moe_gemm.hpp:281-284        fp32 storage: act_apply (csrc/common.hpp:141, :144), IEEE divisions, tanhf
      csrc/moe_gemm.hpp:286-288        the three stores
  EP_DGRAD (down_dgrad): D is an accumulator with E_D = (H + 8) f A_D
      csrc/moe_gemm.hpp:305            hw = 0.5 w (exact)
      csrc/moe_gemm.hpp:313-315        gm = hw D, Agu = gm coef: 2 fp32 roundings, one store each
      csrc/moe_gemm.hpp:311, :325-328, :340 and csrc/moe.hip:131-132
                                       the routing-weight partial: I products m_j D_j and I - 1 additions (4 in the lane, 4 shuffles, the two
                                       column halves, the column tiles), then 0.5 (exact) and one store: (I + 8) f over the absolute sum
  combine
      csrc/moe.hip:112                 acc += w v: k products and k additions, (k + 2) f over sum_s |w| |rows|
      csrc/moe.hip:116                 one store (csrc/common.hpp:90 Vec16<bf16_t>::set)

ASSUMED, not measured: the hardware v_exp_f32 and v_rcp_f32 are accurate to 1 ulp = 2 f each (nothing in this project states it or can
evaluate the instructions off the device; tests/attn_bound.py assumes the same of v_exp_f32 / v_log_f32).  The fp32-storage tanh-GELU goes
through the math library's tanhf, taken at OpenCL's published bound of 5 ulp = 10 f.

The activation.  sigma is the logistic function, S(g) = act(g) / g: sigma(g) for SiLU, sigma(2 z(g)) with z = k0 (g + k1 g^3) for tanh-GELU
(0.5 (1 + tanh z) = sigma(2 z)); 0 < S < 1.
  L_ACT = sup |act'|.  SiLU: act' = sigma (1 + g (1 - sigma)), largest at g = 2.3994: 1.0998 <= 1.1.  tanh-GELU: act' = S + g S', largest at
      g = 1.4185: 1.1290 <= 1.13.
  L_S = sup |S'|.  SiLU: sigma' <= 1/4.  tanh-GELU: S' = sigma'(2 z) 2 k0 (1 + 3 k1 g^2); at g = 0 it is 2 k0 / 4 = 0.39894 (= the normal density
      at 0), and it falls off on both sides because sigma'(2 z) decays like exp(-2 |z|) against the quadratic factor: 0.39894 <= 0.4.
  (tests/test_moe_bound_cpu.py::test_lipschitz_constants evaluates all four on a grid in fp64.)
  Arithmetic of act at the kernel's own g, bf16 storage and fp32 SiLU.  The argument of the hardware exp2 is -w log2 e: the constant and the product
  are 2 roundings, a relative error 2 |w| f of t = exp(-w); tanh-GELU forms w = 2 k0 (g + k1 g^3) in 7 more (k1 and its three products: 4 f on
  k1 g^3; the sum: f; 2 k0 and its product: 2 f; all relative to |w| as |k1 g^3| <= |g + k1 g^3|): c_w = 2 (SiLU), 9 (tanh-GELU).  exp2: 2 f.  1 + t:
  f.  rcp: 2 f.  g times it: f.  The errors of t enter 1 / (1 + t) damped by t / (1 + t) <= 1:
      |da_arith| <= |act(g)| (c_w |w| + 6) f.
  fp32 tanh-GELU, 0.5 g (1 + tanh z): z carries 7 f |z|, |z| sech^2 z <= 0.448, tanhf 10 f, the sum 1 + tanh <= 2: f 2; so 1 + tanh is off by at
  most 16 f ABSOLUTELY (it cancels for z << 0), and |da_arith| <= 8 f |g| + f |act(g)|.
  Both are evaluated at |g| + E_g and |act| + L_ACT E_g, the largest the kernel's own g allows.

    da  = L_ACT E_g + da_arith                                               error of act(g) in the kernel
    m   : e = |u| da + (|a| + da) E_u + f (|m| + ...)                         one product
    cu  : e = da / 2                                                         the halving is exact
    cg  = 1/2 u s,  s = act(g) / (g + 1e-10):
          ds = L_S E_g + eps-term + da_arith / gmin + 4 f (|s| + ...)        (g + 1e-10: f, rcp: 2 f, the product: f)
          eps-term = 1e-10 (1 + f) / gmin + 1e-10 / (|g| - 1e-10),  gmin = |g| - E_g - 1e-10 (1 + f): S(g) g / (g + eps) = S(g) (1 - eps / (g + eps)),
          once for the reference's eps and once for the kernel's fl(1e-10) at its own g (this is the `2e-10 / (|g| - E_g)` of the starting form
          with its second order kept)
          e = 1/2 ((|u| + E_u) ds + |s| E_u) + f (|cg| + ...)                 the product u q
          HELD ONLY where |g| >= 2 E_g + 2^-16; elsewhere cg must be finite with |cg| <= |u|.  The share of elements left out is a condition
          on the inputs, capped at EXCLUDED_CAP per case and asserted.
    y, gx_rows : e = (K + 8) f A
    Agu : e = |1/2 w coef| E_D + 2 f (|ref| + |1/2 w coef| E_D)
    gw  : e = 1/2 sum_j |m_j| E_D[j] + (I + 8) f 1/2 sum_j |m_j| (|D_j| + E_D[j]);  a skipped slot is an exact 0
    combine : e = (k + 2) f sum_s |w| |rows|;  a token with no live slot is an exact 0

The CPU model stays within these forms on every case, so no term was added because a bound was exceeded."""
import functools
import math

import torch

from tests.attn_bound import ratio, rne, trunc      # noqa: F401  (re-exported: the tests take them from here)

U = 2.0 ** -8
F = 2.0 ** -24
EPS = 1e-10
K0, K1 = 0.7978845608028654, 0.044715
L_ACT = {"silu": 1.1, "gelu_tanh": 1.13}
L_S = {"silu": 0.25, "gelu_tanh": 0.4}
C_W = {"silu": 2.0, "gelu_tanh": 9.0}
G_FLOOR = 2.0 ** -16
EXCLUDED_CAP = 5e-3
BM = 128                  # rows of an M tile (MOE_BM)
ACTS = ("silu", "gelu_tanh")

CASES = {
    # rows per expert; `skips` slots carry an id outside [0, E)
    "edges": dict(E=8, k=2, T=260, H=256, I=384, counts=[0, 1, 127, 128, 129, 60, 70, 4], skips=1),
    "seams": dict(E=6, k=2, T=258, H=128, I=128, counts=[0, 257, 0, 256, 1, 0], skips=2),
    "fanout": dict(E=128, k=8, T=48, H=128, I=128, counts=None, skips=0),
    "wrap": dict(E=80, k=1, T=80, H=128, I=1024, counts=[1] * 80, skips=0),
    "none": dict(E=4, k=2, T=5, H=128, I=128, counts=[0] * 4, skips=10),
}
# (case, dtype, activation) of the CPU model's and the kernels' runs: every case in bf16 and fp32, both activations on `edges`
RUNS = [(n, dt, "silu") for n in CASES for dt in (torch.bfloat16, torch.float32)] + [("edges", dt, "gelu_tanh") for dt in (torch.bfloat16, torch.float32)]
RUN_IDS = [f"{n}-{'bf16' if dt == torch.bfloat16 else 'fp32'}-{a}" for n, dt, a in RUNS]


def unit(dtype):
    return U if dtype == torch.bfloat16 else F


def routing(name):
    """idx [T, k] int64 (CPU, seeded): the planted row counts; a token never meets an expert twice; where `skips` >= k whole tokens are skipped"""
    c = CASES[name]
    E, k, T = c["E"], c["k"], c["T"]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if c["counts"] is None:
        return torch.rand(T, E, generator=gen).topk(k, dim=1).indices
    dead = c["skips"] // k                                   # tokens whose every slot is skipped
    ids = [e for e, n in enumerate(c["counts"]) for _ in range(n)] + [E] * (c["skips"] - dead * k)
    Tl = T - dead
    assert len(ids) == Tl * k and max(c["counts"]) <= max(Tl, 0)
    idx = torch.cat([torch.tensor(ids, dtype=torch.int64).reshape(k, Tl).T, torch.full((dead, k), E, dtype=torch.int64)])
    idx = idx[torch.randperm(T, generator=gen)]
    skipped = idx == E
    turn = torch.cumsum(skipped.flatten().long(), 0).reshape(T, k) % 3
    return torch.where(skipped, torch.tensor([-1, E, E + 3])[turn], idx)      # a skipped slot's id: -1, E, E + 3 in turn


class Plan:
    """the plan rows from idx alone (as tests/test_moe_wgrad_gpu.py::_ref): a stable sort of the expert ids, skipped slots last"""

    def __init__(self, idx, E):
        self.T, self.k = idx.shape
        self.E, self.R = E, idx.numel()
        flat = idx.flatten()
        live = (flat >= 0) & (flat < E)
        key = torch.where(live, flat, torch.full_like(flat, E))
        self.order = torch.sort(key, stable=True).indices                 # plan row -> t k + s
        self.cnt = torch.bincount(key, minlength=E + 1)[:E]
        self.off = torch.cat([torch.zeros(1, dtype=torch.int64, device=idx.device), torch.cumsum(self.cnt, 0)])
        self.n = int(self.cnt.sum())
        self.src = self.order[:self.n]
        self.tok, self.slot = self.src // self.k, self.src % self.k
        self.expert = key[self.src]
        self.inv = torch.full((self.R,), -1, dtype=torch.int64, device=idx.device)
        self.inv[self.src] = torch.arange(self.n, device=idx.device)
        self.toff = torch.cat([torch.zeros(1, dtype=torch.int64, device=idx.device), torch.cumsum((self.cnt + BM - 1) // BM, 0)])
        self.live_tok = live.reshape(self.T, self.k).any(1)

    def groups(self):
        for e in range(self.E):
            a, b = int(self.off[e]), int(self.off[e + 1])
            if b > a:
                yield e, slice(a, b)


@functools.lru_cache(maxsize=None)
def plan_of(name):
    return Plan(routing(name), CASES[name]["E"])


def planted(name):
    """the rows the structural faults of the CPU test are planted on (`edges`): the last live row of expert 2's partial tile, and the first row
    of expert 4's second tile with the expert before it"""
    P = plan_of(name)
    return dict(p_last=int(P.off[2] + P.cnt[2] - 1), p_second=int(P.off[4] + BM), e_prev=3)


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """every operand of every op, seeded on the CPU and rounded to dtype.  Activation rows carry their token's power-of-two scale 2^-6 .. 2^2
    (the planted rows of `edges`: 2^-6); token z has x = 0; gate row j0 of expert e0 is all zero; every activation row that nothing may read
    is NaN (plan rows at and past off[E]; the x / G rows of a token whose every slot is skipped)"""
    c, P = CASES[name], plan_of(name)
    E, k, T, H, I, R = c["E"], c["k"], c["T"], c["H"], c["I"], P.R
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    scale = 2.0 ** torch.randint(-6, 3, (T,), generator=gen).double()
    d = dict(name=name, dtype=dtype, small=[], zero_tok=None, e0=None, j0=37)
    if name == "edges":
        pl = planted(name)
        d["small"] = sorted({int(P.tok[p]) for p in (pl["p_last"], pl["p_last"] - 1, pl["p_second"])})
        scale[d["small"]] = 2.0 ** -6
    scale = scale.float()
    rs = torch.ones(R)
    rs[:P.n] = scale[P.tok]
    nan = float("nan")

    def rows(cols, s=1.0):
        t = torch.randn(R, cols, generator=gen) * (s * rs)[:, None]
        t[P.n:] = nan
        return t

    x, G = torch.randn(T, H, generator=gen) * scale[:, None], torch.randn(T, H, generator=gen) * scale[:, None]
    if P.n:
        d["zero_tok"] = next(t for t in range(T) if bool(P.live_tok[t]) and t not in d["small"])
        x[d["zero_tok"]] = 0
        d["e0"] = int(P.cnt.argmax())
    x[~P.live_tok], G[~P.live_tok] = nan, nan
    Wgu = torch.randn(E, 2 * I, H, generator=gen) / H ** 0.5
    if d["e0"] is not None:
        Wgu[d["e0"], d["j0"]] = 0
    Wd = torch.randn(E, H, I, generator=gen) / I ** 0.5
    w = (torch.rand(T, k, generator=gen) + 0.1) / k
    d.update(x=x, G=G, Wgu=Wgu, Wd=Wd, w=w, m_in=rows(I), coef_in=rows(2 * I, 0.5), Agu_in=rows(2 * I), rows_in=rows(H))
    for key in ("x", "G", "Wgu", "Wd", "w", "m_in", "coef_in", "Agu_in", "rows_in"):
        d[key] = d[key].to(dtype)
    return d


# ---- fp64 references --------------------------------------------------------------------------------------------------------------------
def act64(g, act):
    if act == "silu":
        return g * torch.sigmoid(g)
    return 0.5 * g * (1.0 + torch.tanh(K0 * (g + K1 * g ** 3)))


def _grouped(P, A, W, trans):
    """per plan row p of expert e: A[p] W[e]^T (trans) or A[p] W[e] -> (sum, the same sum over absolute values); A [n, K] fp64 in plan rows"""
    N = W.shape[1] if trans else W.shape[2]
    out, mag = (torch.zeros(P.n, N, dtype=torch.float64, device=A.device) for _ in range(2))
    for e, r in P.groups():
        B = W[e].double().T if trans else W[e].double()
        out[r], mag[r] = A[r] @ B, A[r].abs() @ B.abs()
    return out, mag


def gate_up_fwd(P, x, Wgu, act):
    """-> dict(g, u, A_g, A_u, a, m, s, cg, cu) [n, I] fp64"""
    I = Wgu.shape[1] // 2
    gu, A = _grouped(P, x.double()[P.tok], Wgu, True)
    g, u = gu[:, :I], gu[:, I:]
    a = act64(g, act)
    s = a / (g + EPS)
    return dict(g=g, u=u, A_g=A[:, :I], A_u=A[:, I:], a=a, m=a * u, s=s, cg=0.5 * u * s, cu=0.5 * a)


def down_fwd(P, m, Wd):
    """-> (y, A_y) [n, H]"""
    return _grouped(P, m.double()[:P.n], Wd, True)


def down_dgrad(P, G, Wd, coef, m, w):
    """-> dict(D, A_D [n, I], hc [n, 2 I] = 1/2 w coef, Agu [n, 2 I], gw [T, k], and the two sums of the gw bound [n])"""
    D, A_D = _grouped(P, G.double()[P.tok], Wd, False)
    hc = 0.5 * w.double().flatten()[P.src][:, None] * coef.double()[:P.n]
    md = m.double()[:P.n]
    gw = torch.zeros(P.R, dtype=torch.float64, device=D.device)
    gw[P.src] = 0.5 * (md * D).sum(1)
    return dict(D=D, A_D=A_D, hc=hc, Agu=hc * torch.cat([D, D], 1), gw=gw.reshape(P.T, P.k), m_abs=md.abs())


def gate_up_dgrad(P, Agu, Wgu):
    """-> (gx_rows, A) [n, H]"""
    return _grouped(P, Agu.double()[:P.n], Wgu, False)


def combine(P, rows, w=None):
    """-> (out, sum_s |w| |rows|) [T, H]; a token's live slots in order"""
    rows = rows.double()
    out, mag = (torch.zeros(P.T, rows.shape[1], dtype=torch.float64, device=rows.device) for _ in range(2))
    wv = torch.ones(P.n, dtype=torch.float64, device=rows.device) if w is None else w.double().flatten()[P.src]
    out.index_add_(0, P.tok, rows[:P.n] * wv[:, None])
    mag.index_add_(0, P.tok, rows[:P.n].abs() * wv.abs()[:, None])
    return out, mag


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def _store(ref, e, u):
    return e + u * (ref.abs() + e)


def bound_mma(ref, A, K, u):
    return _store(ref, (K + 8) * F * A, u)


def act_arith(g_abs, a_abs, act, dtype):
    """|da_arith| at |g| = g_abs, |act| = a_abs (doc above)"""
    if act == "gelu_tanh" and dtype == torch.float32:
        return 8 * F * g_abs + F * a_abs
    w_abs = g_abs if act == "silu" else 2 * K0 * (g_abs + K1 * g_abs ** 3)
    return a_abs * (C_W[act] * w_abs + 6) * F


def bounds_gate_up_fwd(R, H, act, dtype, eps=EPS, E_g=None, E_u=None):
    """R: gate_up_fwd(...) -> dict(m, cu, cg: bounds; held: where the cg bound holds; E_g, E_u).  eps, E_g, E_u: the stabiliser of s and the errors
    of g, u where they are not this module's (tests/gemm_bound.py: the dense gate/up GEMM takes eps_g as an argument and scales its rows)"""
    u, EPS = unit(dtype), eps      # noqa: N806  (the forms below are written in the docstring's EPS)
    g, uu, a, s = R["g"].abs(), R["u"].abs(), R["a"].abs(), R["s"].abs()
    E_g = (H + 8) * F * R["A_g"] if E_g is None else E_g
    E_u = (H + 8) * F * R["A_u"] if E_u is None else E_u
    arith = act_arith(g + E_g, a + L_ACT[act] * E_g, act, dtype)
    da = L_ACT[act] * E_g + arith
    e_m = uu * da + (a + da) * E_u
    e_m = e_m + F * (R["m"].abs() + e_m)
    held = g >= 2 * E_g + G_FLOOR
    gmin = (g - E_g - EPS * (1 + F)).clamp_min(1e-300)
    ds = L_S[act] * E_g + EPS * (1 + F) / gmin + EPS / (g - EPS).clamp_min(1e-300) + arith / gmin
    ds = ds + 4 * F * (s + ds)
    e_cg = 0.5 * ((uu + E_u) * ds + s * E_u)
    e_cg = e_cg + F * (R["cg"].abs() + e_cg)
    return dict(m=_store(R["m"], e_m, u), cu=_store(R["cu"], 0.5 * da, u), cg=_store(R["cg"], e_cg, u), held=held, E_g=E_g, E_u=E_u)


def bounds_down_dgrad(R, H, I, dtype):
    u = unit(dtype)
    E_D = (H + 8) * F * R["A_D"]
    E2 = torch.cat([E_D, E_D], 1)
    e = R["hc"].abs() * E2
    e = e + 2 * F * (R["Agu"].abs() + e)
    e_row = 0.5 * (R["m_abs"] * E_D).sum(1) + (I + 8) * F * 0.5 * (R["m_abs"] * (R["D"].abs() + E_D)).sum(1)
    return dict(Agu=_store(R["Agu"], e, u), gw_rows=e_row)


def bound_gw(P, R, B, dtype):
    e = torch.zeros(P.R, dtype=torch.float64, device=B["gw_rows"].device)
    e[P.src] = B["gw_rows"]
    return _store(R["gw"], e.reshape(P.T, P.k), unit(dtype))


def bound_combine(ref, mag, k, dtype):
    return _store(ref, (k + 2) * F * mag, unit(dtype))


def check(name, x, ref, bound, zero=None, log=None, strict=True, where=None):
    """x, ref, bound fp64, same shape: finite; |x - ref| <= bound on every element (of `where`, a bool mask, when given); exact zeros where
    `zero` says so.  Prints the worst err / bound and its index, appends it to log[name].  strict = False (the planted faults): only returns it"""
    if strict:
        assert x.shape == ref.shape, (name, x.shape, ref.shape)
        assert bool(torch.isfinite(x).all()), f"{name}: not finite"
        if zero is not None and bool(zero.any()):
            assert bool((x[zero.expand_as(x)] == 0).all()), f"{name}: an empty sum is not an exact zero"
    x = torch.nan_to_num(x, nan=float("inf"))
    if where is not None:
        x, bound = torch.where(where, x, ref), torch.where(where, bound, torch.ones_like(bound))
    worst, at = ratio(x, ref, bound)
    if log is not None:
        log[name] = max(log.get(name, 0.0), worst)
    if strict:
        print(f"  {name}: worst err / bound = {worst:.3f} at {at}")
        assert worst <= 1.0, (name, worst, at)
    return worst


def zero_sets(d, P, I):
    """where gate_up_fwd's m, cg, cu are exact zeros [n, I]: the rows of the x = 0 token, column j0 of expert e0's rows"""
    z = torch.zeros(P.n, I, dtype=torch.bool)
    if d["zero_tok"] is not None:
        z[P.tok == d["zero_tok"]] = True
        z[P.expert == d["e0"], d["j0"]] = True
    return z


def evaluate(d, act, out, log=None, strict=True, only=None):
    """every op-level output of one case against its bound.  d: inputs(...) (CPU); out: dict of fp64 CPU tensors in plan rows ([R, .], the first
    off[E] are judged) under m, cg, cu, y, Agu, gw [T, k], gx_rows, out_w, out_1 [T, H] -- those present (and in `only`) are checked.
    -> {name: worst err / bound}; asserts with strict"""
    name, dtype = d["name"], d["dtype"]
    c, P = CASES[name], plan_of(name)
    H, I, k = c["H"], c["I"], c["k"]
    log = {} if log is None else log
    kw = dict(log=log, strict=strict)
    want = lambda n: n in out and (only is None or n in only)      # noqa: E731
    if any(want(n) for n in ("m", "cg", "cu")):
        R = gate_up_fwd(P, d["x"], d["Wgu"], act)
        B = bounds_gate_up_fwd(R, H, act, dtype)
        zero = zero_sets(d, P, I)
        for n in ("m", "cu"):
            if want(n):
                check(n, out[n][:P.n], R[n], B[n], zero=zero, **kw)
        if want("cg"):
            x, held = out["cg"][:P.n], B["held"] | zero
            left = float((~held).double().mean()) if held.numel() else 0.0
            check("cg", x, R["cg"], torch.where(zero, torch.zeros_like(B["cg"]), B["cg"]), zero=zero, where=held, **kw)
            if strict:
                print(f"  cg: {100 * left:.3f} % of the elements sit below the floor on |g|")
                assert left <= EXCLUDED_CAP, left
                assert bool((x[~held].abs() <= R["u"][~held].abs()).all()), "cg below the floor on |g|: |cg| > |u|"
    if want("y"):
        ref, A = down_fwd(P, d["m_in"], d["Wd"])
        check("y", out["y"][:P.n], ref, bound_mma(ref, A, I, unit(dtype)), **kw)
    if want("Agu") or want("gw"):
        R = down_dgrad(P, d["G"], d["Wd"], d["coef_in"], d["m_in"], d["w"])
        B = bounds_down_dgrad(R, H, I, dtype)
        if want("Agu"):
            check("Agu", out["Agu"][:P.n], R["Agu"], B["Agu"], **kw)
        if want("gw"):
            check("gw", out["gw"], R["gw"], bound_gw(P, R, B, dtype), zero=(P.inv < 0).reshape(P.T, P.k), **kw)
    if want("gx_rows"):
        ref, A = gate_up_dgrad(P, d["Agu_in"], d["Wgu"])
        check("gx_rows", out["gx_rows"][:P.n], ref, bound_mma(ref, A, 2 * I, unit(dtype)), **kw)
    for n, w in (("out_w", d["w"]), ("out_1", None)):
        if want(n):
            ref, mag = combine(P, d["rows_in"], w)
            check(n, out[n], ref, bound_combine(ref, mag, k, dtype), zero=~P.live_tok[:, None], **kw)
    return log


# ---- the torch model of the kernels' arithmetic -----------------------------------------------------------------------------------------
FAULTS = {          # name -> the outputs it touches
    "swap_gu_block": ("m", "cg", "cu"),                                  # the gate and up halves swapped in one 16-column block
    "cu_for_cg": ("cg",),                                                # cu stored where cg belongs
    "last_row": ("m", "cg", "cu", "y", "Agu", "gw", "gx_rows"),          # the last live row of a partial tile takes its neighbour's data
    "prev_weight": ("m", "cg", "cu", "y", "Agu", "gw", "gx_rows"),       # the first row of an expert's second tile: the previous expert's weight
    "other_slot_w": ("Agu", "out_w"),                                    # the routing weight of the other slot
    "drop_gw_tile": ("gw",),                                             # one column tile's gw partial dropped
    "drop_last_k": ("m", "cg", "cu", "y", "Agu", "gw", "gx_rows"),       # the last K stage dropped
    "trunc": ("y", "gx_rows", "m", "cu"),                                # truncation at the single-rounding stores (bf16)
}
STRUCTURAL = tuple(n for n in FAULTS if n != "trunc")
CHAIN_TOUCH = {"swap_gu_block": ("out", "gx"), "cu_for_cg": ("gx",), "last_row": ("out", "gx", "gw"), "prev_weight": ("out", "gx", "gw"),
               "other_slot_w": ("out", "gx"), "drop_gw_tile": ("gw",), "drop_last_k": ("out", "gx", "gw"), "trunc": ("out", "gx")}


def _mm(P, A, W, trans, fault, pl, itemsize):
    """the grouped GEMM in fp32 (A [n, K] in plan rows), with the A-side and weight-side faults"""
    A = A.clone()
    if fault == "last_row":
        A[pl["p_last"]] = A[pl["p_last"] - 1]
    if fault == "drop_last_k":
        A[:, -(128 // itemsize):] = 0
    N = W.shape[1] if trans else W.shape[2]
    out = torch.zeros(P.n, N)
    B = lambda e: W[e].float().T if trans else W[e].float()      # noqa: E731
    for e, r in P.groups():
        out[r] = A[r] @ B(e)
    if fault == "prev_weight":
        p = pl["p_second"]
        out[p] = A[p] @ B(pl["e_prev"])
    return out


def _full(P, t):
    """[n, cols] -> [R, cols] with NaN rows past off[E] (what a kernel leaves of a NaN-filled buffer)"""
    out = torch.full((P.R, t.shape[1]), float("nan"))
    out[:P.n] = t
    return out


def model_gate_up_fwd(P, x, Wgu, act, dtype, rnd, fault=None, pl=None):
    """-> coef [R, 2 I], m [R, I] fp32 (rounded through rnd)"""
    I = Wgu.shape[1] // 2
    gu = _mm(P, x.float()[P.tok], Wgu, True, fault, pl, dtype.itemsize)
    g, u = gu[:, :I].clone(), gu[:, I:].clone()
    if fault == "swap_gu_block":
        j = slice(48, 64)
        g[:, j], u[:, j] = gu[:, I:][:, j], gu[:, :I][:, j]
    one, eps = torch.tensor(1.0), torch.tensor(1e-10, dtype=torch.float32)
    den = g + eps
    if dtype == torch.bfloat16:
        w = g if act == "silu" else (2.0 * K0) * (g + K1 * g * g * g)
        y = g * (one / (one + torch.exp(-w)))
        q = (0.5 * y) * (one / den)
        cg = torch.where(den == 0, torch.zeros_like(q), u * q)
    else:
        y = g / (one + torch.exp(-g)) if act == "silu" else 0.5 * g * (one + torch.tanh(K0 * (g + K1 * g * g * g)))
        cg = torch.where(den == 0, torch.zeros_like(y), 0.5 * u * (y / den))
    m, cu = y * u, 0.5 * y
    if fault == "cu_for_cg":
        cg = cu
    rr = rnd if dtype == torch.bfloat16 else (lambda t: t)
    st = trunc if (fault == "trunc" and dtype == torch.bfloat16) else rr
    return _full(P, torch.cat([rr(cg), st(cu)], 1)), _full(P, st(m))


def model_down_fwd(P, m, Wd, dtype, rnd, fault=None, pl=None):
    y = _mm(P, m.float()[:P.n], Wd, True, fault, pl, dtype.itemsize)
    st = trunc if fault == "trunc" else rnd
    return _full(P, st(y) if dtype == torch.bfloat16 else y)


def model_down_dgrad(P, G, Wd, coef, m, w, dtype, rnd, fault=None, pl=None):
    """-> Agu [R, 2 I], gw [T, k]"""
    I = Wd.shape[2]
    D = _mm(P, G.float()[P.tok], Wd, False, fault, pl, dtype.itemsize)
    wf = w.float()
    if fault == "other_slot_w":
        wf = wf.roll(1, 1)
    gm = (0.5 * wf.flatten()[P.src])[:, None] * D
    Agu = torch.cat([gm, gm], 1) * coef.float()[:P.n]
    prod = m.float()[:P.n] * D
    if fault == "drop_gw_tile":
        prod[:, BM:2 * BM] = 0
    part = prod.reshape(P.n, I // BM, BM).sum(2).sum(1)
    gw = torch.zeros(P.R)
    gw[P.src] = 0.5 * part
    rr = rnd if dtype == torch.bfloat16 else (lambda t: t)
    return _full(P, rr(Agu)), rr(gw).reshape(P.T, P.k)


def model_gate_up_dgrad(P, Agu, Wgu, dtype, rnd, fault=None, pl=None):
    gx = _mm(P, Agu.float()[:P.n], Wgu, False, fault, pl, dtype.itemsize)
    st = trunc if fault == "trunc" else rnd
    return _full(P, st(gx) if dtype == torch.bfloat16 else gx)


def model_combine(P, rows, w, dtype, rnd, fault=None):
    rows = rows.float()
    acc = torch.zeros(P.T, rows.shape[1])
    inv = P.inv.reshape(P.T, P.k)
    wf = None if w is None else w.float()
    if wf is not None and fault == "other_slot_w":
        wf = wf.roll(1, 1)
    for s in range(P.k):
        p = inv[:, s]
        live = p >= 0
        v = rows[p.clamp_min(0)]
        term = v if wf is None else wf[:, s, None] * v
        acc = acc + torch.where(live[:, None], term, torch.zeros_like(term))
    return rnd(acc) if dtype == torch.bfloat16 else acc


def model_ops(d, act, rnd=rne, fault=None):
    """every op of one case on its own (synthetic) inputs -> fp64 outputs under the keys of evaluate"""
    P, dtype = plan_of(d["name"]), d["dtype"]
    pl = planted(d["name"]) if fault in ("last_row", "prev_weight") else None
    coef, m = model_gate_up_fwd(P, d["x"], d["Wgu"], act, dtype, rnd, fault, pl)
    I = m.shape[1]
    Agu, gw = model_down_dgrad(P, d["G"], d["Wd"], d["coef_in"], d["m_in"], d["w"], dtype, rnd, fault, pl)
    out = dict(m=m, cg=coef[:, :I], cu=coef[:, I:], y=model_down_fwd(P, d["m_in"], d["Wd"], dtype, rnd, fault, pl), Agu=Agu, gw=gw,
               gx_rows=model_gate_up_dgrad(P, d["Agu_in"], d["Wgu"], dtype, rnd, fault, pl),
               out_w=model_combine(P, d["rows_in"], d["w"], dtype, rnd, fault), out_1=model_combine(P, d["rows_in"], None, dtype, rnd))
    return {n: t.double() for n, t in out.items()}


def model_chain(d, act, rnd=rne, fault=None):
    """the MoEExpertsFn chain (lxt_amd/efficient/moe.py) -> fp64 out [T, H], gx [T, H], gw [T, k]"""
    P, dtype = plan_of(d["name"]), d["dtype"]
    pl = planted(d["name"]) if fault in ("last_row", "prev_weight") else None
    coef, m = model_gate_up_fwd(P, d["x"], d["Wgu"], act, dtype, rnd, fault, pl)
    y = model_down_fwd(P, m, d["Wd"], dtype, rnd, fault, pl)
    out = model_combine(P, y, d["w"], dtype, rnd, fault)
    Agu, gw = model_down_dgrad(P, d["G"], d["Wd"], coef, m, d["w"], dtype, rnd, fault, pl)
    gx = model_combine(P, model_gate_up_dgrad(P, Agu, d["Wgu"], dtype, rnd, fault, pl), None, dtype, rnd)
    return dict(out=out.double(), gx=gx.double(), gw=gw.double())


def chain_ref(d, act):
    """the same chain in fp64 on the rounded inputs (tests/test_moe_gpu.py::ref_experts, walked by plan rows)"""
    P = plan_of(d["name"])
    R = gate_up_fwd(P, d["x"], d["Wgu"], act)
    y, _ = down_fwd(P, R["m"], d["Wd"])
    out, _ = combine(P, y, d["w"])
    B = down_dgrad(P, d["G"], d["Wd"], torch.cat([R["cg"], R["cu"]], 1), R["m"], d["w"])
    gx, _ = combine(P, gate_up_dgrad(P, B["Agu"], d["Wgu"])[0])
    return dict(out=out, gx=gx, gw=B["gw"])


def todays_bars(x, ref, dtype):
    """would tests/test_moe_gpu.py::test_experts_function_against_fp64 pass this chain output?  nmax <= 2e-2 and cos >= 0.999 in bf16, nmax <= 1e-5
    in fp32 (NaN rows of skipped tokens in neither) -> (passes, nmax, cos)"""
    ok = torch.isfinite(ref)
    a, b = x[ok].double(), ref[ok].double()
    if not bool(torch.isfinite(a).all()):
        return False, math.inf, 0.0
    nm = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    cs = float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))
    return (nm <= 2e-2 and cs >= 0.999) if dtype == torch.bfloat16 else nm <= 1e-5, nm, cs
