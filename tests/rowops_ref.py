"""fp64 restatements of the row and element-wise operations of csrc/rowops.hip and csrc/eltwise.hip, written from include/lrp_hip.h and the
reference's formulas (lxt/efficient/patches.py, lxt/explicit/functional.py), not from the kernels.

Every function takes the STORED tensors (fp32 or bf16, on any device), converts them to fp64 and returns fp64.  Where the header says a kernel
rounds an intermediate to the storage type, the reference does the same with `.to(dtype).double()` (act_bwd: act(x) in storage precision
before the ratio).  Where PyTorch supplies an independent statement of the operation (F.layer_norm, F.silu / F.gelu / torch.tanh and their
autograd, torch.softmax) that is used instead of a hand-written formula; tests/test_rowops_ref_cpu.py checks the remaining closed forms
against autograd on the CPU.
"""
import torch
import torch.nn.functional as F

ACTS = ("silu", "gelu_tanh", "gelu", "tanh")

# planted inputs of the activation tests: zero, the linear range, and the tails where exp overflows / tanh saturates in fp32.
# +-1e-3 is not a bf16 number: callers round the list to the storage type before use.
SPECIALS = (0.0, 1e-3, -1e-3, 0.5, -0.5, 8.0, -8.0, 20.0, -20.0, 90.0, -90.0)


def d(x):
    return None if x is None else x.double()


def act64(x64, act):
    if act == "silu":
        return F.silu(x64)
    if act == "gelu_tanh":
        return F.gelu(x64, approximate="tanh")
    if act == "gelu":
        return F.gelu(x64)
    if act == "tanh":
        return torch.tanh(x64)
    raise ValueError(act)


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_stats(x, eps):
    """-> (mean [M], rstd [M]) of the stored x, biased variance"""
    x64 = d(x)
    mean = x64.mean(-1)
    var = ((x64 - mean[..., None]) ** 2).mean(-1)
    return mean, (var + eps).rsqrt()


def layernorm_fwd(x, w, b, eps):
    return F.layer_norm(d(x), (x.shape[-1],), d(w), d(b), eps)


def layernorm_bwd(Gy, y, w, x, eps, eps_y):
    """identity rule with the std detached: u = Gy (*) y/(y + eps_y) (*) w * rstd, Gx = u - mean_row(u); eps_y == 0: no stabiliser (y unused)"""
    _, rstd = layernorm_stats(x, eps)
    u = d(Gy) * rstd[..., None]
    if eps_y != 0.0:
        y64 = d(y)
        u = u * (y64 / (y64 + eps_y))
    if w is not None:
        u = u * d(w)
    return u - u.mean(-1, keepdim=True)


def layernorm_bwd_plain(Gy, x, w, eps):
    """full VJP (mean and 1/std differentiated): autograd through F.layer_norm"""
    x64 = d(x).clone().requires_grad_()
    y = F.layer_norm(x64, (x.shape[-1],), d(w), None, eps)
    return torch.autograd.grad(y, x64, d(Gy))[0]


# ---------------------------------------------------------------------------------------------------------------------------- activations
def act_fwd(x, act):
    return act64(d(x), act)


def act_grad(Gy, x, act):
    x64 = d(x).clone().requires_grad_()
    return torch.autograd.grad(act64(x64, act), x64, d(Gy))[0]


def act_bwd(Gy, x, act, eps_g):
    """Gy * T(act(x)) / (x + eps_g), T = rounding to the storage type; exactly 0 where x + eps_g == 0"""
    x64 = d(x)
    y = act64(x64, act).to(x.dtype).double()
    den = x64 + eps_g
    zero = den == 0
    return torch.where(zero, torch.zeros_like(den), d(Gy) * y / torch.where(zero, torch.ones_like(den), den))


# -------------------------------------------------------------------------------------------------------------------------------- softmax
def softmax_fwd(x, inv_temp):
    return torch.softmax(d(x) * inv_temp, -1)


def softmax_rule_bwd(x, p, Rp, inv_temp):
    """Rx = (x/T) (*) (Rp - p * sum(Rp)), -inf entries of x -> 0"""
    xs = d(x) * inv_temp
    xs = torch.where(torch.isneginf(xs), torch.zeros_like(xs), xs)
    Rp64 = d(Rp)
    return xs * (Rp64 - d(p) * Rp64.sum(-1, keepdim=True))


# --------------------------------------------------------------------------------------------------------------------------- element-wise
def eps_scale(g, z, c, eps, relevance=False):
    """mode 0: g (*) z/(c z + eps), eps == 0 -> g/c;  mode 1 (relevance): g / (c z + eps)"""
    g64, z64 = d(g), d(z)
    if relevance:
        return g64 / (c * z64 + eps)
    if eps == 0.0:
        return g64 / c
    return g64 * (z64 / (c * z64 + eps))


def mul(a, b):
    return d(a) * d(b)


def add2_rule_bwd(a, b, R, eps):
    s = d(R) / (d(a) + d(b) + eps)
    return s * d(a), s * d(b)


def add_bcast(x, y):
    """x [M, H] + y [period, H] repeated down the rows, in the STORAGE type: one exact fp32 add and one round-to-nearest-even (the only
    reference here that is not fp64: the kernel has to match it bit for bit)"""
    M, H = x.shape
    rows = torch.arange(M, device=x.device) % y.shape[0]
    return (x.float() + y.float()[rows]).to(x.dtype)


# ------------------------------------------------------------------------------------------------------------------------------ read-outs
def readout(emb, G):
    return (d(emb) * d(G)).sum(-1)


def head_seed(W_lm, logits, idx, w_norm, rstd_last, w_offset, eps_lin):
    """Gh_last[b, :] = z/(z + eps_lin) * W_lm[idx[b], :] (*) (w_norm + w_offset) * rstd[b], z = logits[b, idx[b]]; eps_lin == 0: factor 1"""
    i = idx.long()
    z = d(logits)[torch.arange(len(i), device=i.device), i]
    zfac = z / (z + eps_lin) if eps_lin != 0.0 else torch.ones_like(z)
    return (zfac * d(rstd_last))[:, None] * d(W_lm)[i] * (d(w_norm) + w_offset)
