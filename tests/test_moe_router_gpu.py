"""GPU: the router kernels of csrc/moe_router.hip (ops.moe_router_fwd / moe_router_bwd / moe_expert_relevance) against fp64 torch
restatements of HF's Qwen3MoeTopKRouter.forward and its autograd, computed on the rounded inputs: expert choice, routing weights, the dense
logit gradient, tie rows, and the per-expert relevance read-out (fp64 scatter, bit-repeatability, prompt independence)."""
import pytest
import torch

from tests.util import nmax

pytestmark = pytest.mark.gpu

TS = (1, 63, 64, 130)
EK = ((8, 2), (60, 4), (128, 8), (1024, 16), (4, 4))
MARGIN = 1e-4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")


def make_logits(T, E, k, dtype, seed):
    """seeded logits whose k + 1 largest entries per row are spaced: the chosen experts get 2 + 0.4 j + U(0, 0.1) at random places, the rest
    stay below 1.05, so after the rounding to `dtype` every gap between neighbours among the k + 1 largest PROBABILITIES is >= 1e-4
    (asserted in the test, on the CPU)"""
    g = torch.Generator().manual_seed(seed)
    x = (0.3 * torch.randn(T, E, generator=g)).clamp(-1.05, 1.05)
    pick = torch.rand(T, E, generator=g).argsort(1)[:, :k]
    x.scatter_(1, pick, 2.0 + 0.4 * torch.arange(k, dtype=torch.float32)[None] + 0.1 * torch.rand(T, k, generator=g))
    return x.to(dtype)


def ref_router(logits, k, norm, gw):
    """fp64: HF's forward (softmax, topk, renorm) and autograd's gradient of sum(w G_w) at the logits"""
    x = logits.double().cpu().requires_grad_()
    p = torch.softmax(x, -1)
    top, idx = torch.topk(p, k, dim=-1)
    w = top / top.sum(-1, keepdim=True) if norm else top
    (w * gw.double().cpu()).sum().backward()
    return p.detach(), idx, w.detach(), x.grad


def pitched(t, fill=float("nan")):
    """the same values in storage with a row pitch > E on the 16-byte grid"""
    T, E = t.shape
    ld = (E + 8 + 7) // 8 * 8
    buf = torch.full((T, ld), fill, dtype=t.dtype, device=t.device)
    buf[:, :E] = t
    return buf[:, :E], buf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("norm", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("E,k", EK)
def test_router_forward_and_backward_against_fp64(E, k, norm, dtype):
    _need_gpu()
    import lxt_amd.ops as ops
    for T in TS:
        logits = make_logits(T, E, k, dtype, seed=1000 * E + T)
        gw = torch.randn(T, k, generator=torch.Generator().manual_seed(T + k)).to(dtype)
        p, r_idx, r_w, r_gl = ref_router(logits, k, norm, gw)
        srt = p.sort(-1, descending=True).values[:, : min(k + 1, E)]
        assert float((srt[:, :-1] - srt[:, 1:]).min()) >= MARGIN          # includes the k-th / (k+1)-th gap
        x, _ = pitched(logits.cuda())
        idx, w, lse = ops.moe_router_fwd(x, k, norm)
        assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), r_idx)
        assert nmax(lse, torch.logsumexp(logits.double(), -1)) <= 1e-6
        out, buf = pitched(torch.zeros(T, E, dtype=dtype, device="cuda"))
        gl = ops.moe_router_bwd(x, lse, idx, w, gw.cuda(), norm, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(buf[:, E:]).all()                              # nothing written past the E columns
        assert torch.equal(gl, ops.moe_router_bwd(x.contiguous(), lse, idx, w, gw.cuda(), norm))
        rowmax = r_gl.abs().amax(1, keepdim=True)
        if dtype == torch.float32:
            assert nmax(w, r_w) <= 1e-6
            assert nmax(gl, r_gl) <= 1e-5
        else:
            assert bool(((w.double().cpu() - r_w).abs() <= 2.0 ** -8 * r_w.abs()).all())
            assert bool(((gl.double().cpu() - r_gl).abs() <= (2.0 ** -8 + 1e-5) * rowmax).all())
        if norm:
            unsel = torch.ones(T, E, dtype=torch.bool).scatter_(1, r_idx, False)
            assert bool((gl.cpu()[unsel] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("norm", [True, False], ids=["renorm", "plain"])
def test_router_tie_rows(norm, dtype):
    """an all-equal row (HF's zero-initialised router) picks experts 0 .. k-1 with equal weights; a tie exactly at the k-th place goes to
    the lower index"""
    _need_gpu()
    import lxt_amd.ops as ops
    E, k = 128, 8
    x = torch.zeros(2, E, dtype=dtype)
    x[1, 70:70 + k - 1] = 3.0          # k - 1 clear winners ...
    x[1, [5, 100, 101]] = 1.0          # ... and three candidates for the last place
    idx, w, _ = ops.moe_router_fwd(x.cuda(), k, norm)
    idx, w = idx.cpu(), w.float().cpu()
    assert idx[0].tolist() == list(range(k)) and bool((w[0] == w[0, 0]).all())
    assert w[0, 0] == (1.0 / k if norm else 1.0 / E)
    assert idx[1].tolist() == list(range(70, 70 + k - 1)) + [5]
    assert bool((w[1, : k - 1] == w[1, 0]).all()) and w[1, k - 1] < w[1, 0]


def ref_expert_relevance(idx, w, gw, B, S, E):
    out = torch.zeros(B, E, dtype=torch.float64)
    prod = (w.double() * gw.double()).cpu().view(B, -1)
    ix = idx.cpu().view(B, -1)
    for b in range(B):
        live = (ix[b] >= 0) & (ix[b] < E)
        out[b].index_add_(0, ix[b][live], prod[b][live])
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S,E,k", [(1, 8, 2), (70, 8, 2), (70, 130, 16)])          # (70 x 16 slots: more than one staged chunk; 130: three expert blocks)
def test_expert_relevance(S, E, k, dtype):
    _need_gpu()
    import lxt_amd.ops as ops
    B, g = 3, torch.Generator().manual_seed(S + E)
    idx = torch.randint(0, E, (B * S, k), generator=g)
    idx[idx == 5] = 6                                                      # an expert nobody selects
    idx[torch.rand(B * S, k, generator=g) < 0.1] = -1                      # skipped slots
    idx[0, 0] = -1
    w, gw = torch.rand(B * S, k, generator=g).to(dtype), torch.randn(B * S, k, generator=g).to(dtype)
    ref = ref_expert_relevance(idx, w, gw, B, S, E)
    a = ops.moe_expert_relevance(idx.cuda(), w.cuda(), gw.cuda(), B, S, E)
    b = ops.moe_expert_relevance(idx.cuda(), w.cuda(), gw.cuda(), B, S, E)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    assert nmax(a, ref) <= 1e-6
    assert bool((a[:, 5] == 0).all())
    # prompt 1 keeps its row to the bit when the other prompts change
    idx2, w2, gw2 = idx.clone().view(B, S, k), w.clone().view(B, S, k), gw.clone().view(B, S, k)
    for other in (0, 2):
        idx2[other] = torch.randint(0, E, (S, k), generator=g)
        w2[other], gw2[other] = w2[other] * 0.5, -gw2[other]
    c = ops.moe_expert_relevance(idx2.view(B * S, k).cuda(), w2.view(B * S, k).cuda(), gw2.view(B * S, k).cuda(), B, S, E)
    assert torch.equal(a[1], c[1]) and not torch.equal(a[0], c[0])
