"""The fp64 references of tests/rowops_ref.py checked on the CPU, so that a failure of tests/test_rowops_gpu.py that survives this file is a
kernel's, not a reference's.

Each closed form written from include/lrp_hip.h is compared with autograd or an F.* call in fp64 on small random inputs (normalised max error
<= 1e-12: both sides are fp64, the slack is summation order), with the reference-made fp32 goldens of tests/golden/rules.npz (<= 1e-5: the
goldens are fp32 results, the bar the kernel tests hold against the same arrays), and evaluated on the planted special inputs of the GPU tests,
where it has to be finite wherever the header defines the result.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import rowops_ref as R
from tests.util import nmax, load, t

EXACT = 1e-12
GOLD = 1e-5
DTYPES = [torch.float32, torch.bfloat16]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("with_w", [True, False])
def test_layernorm_bwd_is_the_vjp_with_detached_std(with_w):
    M, H, eps = 5, 37, 1e-6
    x, Gy = rnd(M, H, seed=1, scale=1.5) + 0.7, rnd(M, H, seed=2)
    w = rnd(H, seed=3).abs() + 0.5 if with_w else None
    b = rnd(H, seed=4)
    xg = x.clone().requires_grad_()
    mu = xg.mean(-1, keepdim=True)
    std = ((xg - mu) ** 2).mean(-1, keepdim=True).add(eps).sqrt().detach()
    y = (xg - mu) / std
    y = (y * w if with_w else y) + b
    ref = torch.autograd.grad(y, xg, Gy, retain_graph=True)[0]
    assert nmax(R.layernorm_bwd(Gy, None, w, x, eps, 0.0), ref) < EXACT
    # the stabilised form is the same VJP of the modified gradient Gy (*) y/(y + eps_y)
    ys = y.detach()
    ref_s = torch.autograd.grad(y, xg, Gy * ys / (ys + 1e-6))[0]
    assert nmax(R.layernorm_bwd(Gy, ys, w, x, eps, 1e-6), ref_s) < EXACT


def test_layernorm_refs_against_golden():
    fx = load("rules.npz")
    x, w, b, g = (t(fx[k]) for k in ("ln_x", "ln_w", "ln_b", "ln_g"))
    y = R.layernorm_fwd(x, w, b, 1e-12)
    assert nmax(y, fx["ln_y"]) < GOLD
    Gx = R.layernorm_bwd(g, t(fx["ln_y"]), w, x, 1e-12, 1e-6)
    assert nmax(Gx * x.double(), fx["ln_Rin"]) < GOLD
    mean, rstd = R.layernorm_stats(x, 1e-12)
    assert nmax(((x.double() - mean[..., None]) * rstd[..., None]) * w.double() + b.double(), y) < EXACT


@pytest.mark.parametrize("with_w", [True, False])
def test_layernorm_bwd_plain_matches_the_header_formula(with_w):
    """the autograd reference against the closed form of include/lrp_hip.h: Gx = rstd (u - mean(u) - xh mean(u (*) xh))"""
    M, H, eps = 4, 101, 1e-6
    x, Gy = rnd(M, H, seed=5, scale=1.5) + 0.7, rnd(M, H, seed=6)
    w = rnd(H, seed=7).abs() + 0.5 if with_w else None
    mean, rstd = R.layernorm_stats(x, eps)
    u = Gy * w if with_w else Gy
    xh = (x - mean[:, None]) * rstd[:, None]
    closed = rstd[:, None] * (u - u.mean(-1, keepdim=True) - xh * (u * xh).mean(-1, keepdim=True))
    assert nmax(R.layernorm_bwd_plain(Gy, x, w, eps), closed) < EXACT


# ---------------------------------------------------------------------------------------------------------------------------- activations
def test_act_refs_against_golden():
    fx = load("rules.npz")
    x, G = t(fx["act_x"]), t(fx["act_G"])
    for act, key in (("silu", "silu"), ("gelu_tanh", "gelut")):
        assert nmax(R.act_fwd(x, act), fx[f"act_{key}_y"]) < GOLD
        assert nmax(R.act_bwd(G, x, act, 1e-10), fx[f"act_{key}_Gin"]) < GOLD


@pytest.mark.parametrize("act", R.ACTS)
def test_act_closed_forms(act):
    """F.* and its autograd against the textbook formulas, and act_bwd in fp64 (no storage rounding to speak of) against Gy act(x)/(x + eps)"""
    x, Gy = rnd(300, seed=8, scale=3.0), rnd(300, seed=9)
    k0, k1 = 0.7978845608028654, 0.044715
    sg = torch.sigmoid(x)
    th = torch.tanh(k0 * (x + k1 * x ** 3))
    cdf, pdf = 0.5 * (1 + torch.erf(x / 2 ** 0.5)), torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5
    y, dy = {"silu": (x * sg, sg * (1 + x * (1 - sg))),
             "gelu_tanh": (0.5 * x * (1 + th), 0.5 * (1 + th) + 0.5 * x * (1 - th * th) * k0 * (1 + 3 * k1 * x * x)),
             "gelu": (x * cdf, cdf + x * pdf),
             "tanh": (torch.tanh(x), 1 - torch.tanh(x) ** 2)}[act]
    assert nmax(R.act_fwd(x, act), y) < EXACT
    assert nmax(R.act_grad(Gy, x, act), Gy * dy) < EXACT
    assert nmax(R.act_bwd(Gy, x, act, 1e-10), Gy * y / (x + 1e-10)) < EXACT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", R.ACTS)
def test_act_refs_on_the_planted_specials(act, dtype):
    x = torch.tensor(R.SPECIALS).to(dtype)
    Gy = rnd(len(R.SPECIALS), seed=10).to(dtype)
    assert x[0] == 0 and torch.isfinite(R.act_fwd(x, act)).all() and torch.isfinite(R.act_grad(Gy, x, act)).all()
    for eps_g in (1e-10, 0.0):
        Gx = R.act_bwd(Gy, x, act, eps_g)
        assert torch.isfinite(Gx).all()
        assert float(Gx[0]) == 0.0                     # x = 0: act(0) = 0 over eps_g, and exactly 0 by definition where x + eps_g == 0
    # the stored-precision rounding of act(x) is in: the fp64 ratio differs from the rounded one by at most one unit of the storage type
    # (1e-30: values below the storage type's normal range, gelu(-20) = -5e-88 for one, round to zero)
    y64 = R.act_fwd(x, act)
    Gx = R.act_bwd(Gy, x, act, 1e-10)
    plain = Gy.double() * y64 / (x.double() + 1e-10)
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    assert bool(((Gx - plain).abs() <= ulp * plain.abs() + 1e-30).all())
    assert not torch.equal(Gx, plain)


# -------------------------------------------------------------------------------------------------------------------------------- softmax
def test_softmax_rule_against_golden():
    fx = load("rules.npz")
    xs, gs = t(fx["sm_x"]), t(fx["sm_g"])
    assert torch.isneginf(xs).any()
    p = R.softmax_fwd(xs, 1.0)
    assert nmax(p, fx["sm_p"]) < GOLD
    Rx = R.softmax_rule_bwd(xs, p, p * gs.double(), 1.0)
    assert torch.isfinite(Rx).all() and nmax(Rx, fx["sm_Rx"]) < GOLD


@pytest.mark.parametrize("inv_temp", [1.0, 0.37, 128 ** -0.5])
def test_softmax_rule_is_input_times_gradient(inv_temp):
    """Rx = x (*) d/dx sum(G (*) softmax(x/T)) with G = Rp / p (lxt/explicit/functional.py:293-322)"""
    x, Rp = rnd(4, 65, seed=11, scale=3.0), rnd(4, 65, seed=12)
    xg = x.clone().requires_grad_()
    p = torch.softmax(xg * inv_temp, -1)
    gx = torch.autograd.grad(p, xg, Rp / p.detach())[0]
    assert nmax(R.softmax_rule_bwd(x, p.detach(), Rp, inv_temp), x * gx) < EXACT


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_refs_on_masked_rows(dtype):
    x = (rnd(3, 65, seed=13, scale=3.0)).to(dtype)
    x[:, 3::7] = float("-inf")
    x[0, 1:] = float("-inf")
    Rp = rnd(3, 65, seed=14).to(dtype)
    p = R.softmax_fwd(x, 0.37)
    masked = torch.isneginf(x)
    assert torch.isfinite(p).all() and bool((p[masked] == 0).all()) and float(p[0, 0]) == 1.0
    assert nmax(p.sum(-1), torch.ones(3)) < EXACT
    Rx = R.softmax_rule_bwd(x, p, Rp, 0.37)
    assert torch.isfinite(Rx).all() and bool((Rx[masked] == 0).all())


# ------------------------------------------------------------------------------------------------------------- element-wise and read-outs
def test_eps_scale_modes():
    g, z = rnd(50, seed=15), rnd(50, seed=16)
    zg = z.clone().requires_grad_()
    # mode 0 is the gradient of log|c z + eps| scaled by g z: g z/(c z + eps); written out independently
    assert nmax(R.eps_scale(g, z, 2.0, 1e-3), g * z * torch.autograd.grad((2.0 * zg + 1e-3).abs().log().sum(), zg)[0] / 2.0) < EXACT
    assert torch.equal(R.eps_scale(g, z, 1.0, 0.0), g) and torch.equal(R.eps_scale(g, z, 0.5, 0.0), 2 * g)
    assert nmax(R.eps_scale(g, z, 2.0, 1e-3, relevance=True) * (2.0 * z + 1e-3), g) < EXACT
    # conservation of the add2 rule: Ra + Rb = R (a + b)/(a + b + eps)
    a, b = rnd(50, seed=17), rnd(50, seed=18)
    Ra, Rb = R.add2_rule_bwd(a, b, g, 1e-6)
    assert nmax(Ra + Rb, g * (a + b) / (a + b + 1e-6)) < EXACT and nmax(Ra * b, Rb * a) < EXACT
    assert torch.equal(R.mul(a, b), a * b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_bcast_is_a_broadcast_add(dtype):
    B, S, H = 3, 4, 10
    x, y = rnd(B * S, H, seed=19).to(dtype), rnd(S, H, seed=20).to(dtype)
    assert torch.equal(R.add_bcast(x, y), (x.reshape(B, S, H) + y).reshape(B * S, H))
    assert torch.equal(R.add_bcast(x, y[:1]), x + y[0]) and torch.equal(R.add_bcast(x, x), x + x)


@pytest.mark.parametrize("w_offset,eps_lin", [(0.0, 0.0), (1.0, 1e-8), (1.0, 0.0)])
def test_readout_and_head_seed(w_offset, eps_lin):
    e, G = rnd(9, 101, seed=21), rnd(9, 101, seed=22)
    assert nmax(R.readout(e, G), torch.einsum("mh,mh->m", e, G)) < EXACT
    # head seed: z/(z + eps) times the gradient of the chosen logit through the final norm with its rstd detached
    B, V, H = 3, 50, 101
    W, wn, rstd, h = rnd(V, H, seed=23), rnd(H, seed=24), rnd(B, seed=25).abs() + 0.5, rnd(B, H, seed=26)
    idx = torch.tensor([5, V - 1, 0], dtype=torch.int32)
    hg = h.clone().requires_grad_()
    logits = (hg * rstd[:, None] * (wn + w_offset)) @ W.T
    z = logits[torch.arange(B), idx.long()]
    gh = torch.autograd.grad(z.sum(), hg)[0]
    zfac = (z / (z + eps_lin)).detach() if eps_lin else 1.0
    out = R.head_seed(W, logits.detach(), idx, wn, rstd, w_offset, eps_lin)
    assert nmax(out, gh * (zfac[:, None] if eps_lin else 1.0)) < EXACT
