"""GPU: the routed-expert kernels of csrc/moe.hip through lxt_amd.efficient.moe.MoEExpertsFn -- routing plan, forward, G_x and G_w against an
fp64 restatement of the reference's experts_forward (lxt/efficient/models/qwen3_moe.py:14-44) written out here, bit-determinism, row
independence, and the Qwen3-MoE drop-in at model level (tests/moe_worker.py, one process per case) against fixtures from the reference."""
import os
import subprocess
import sys

import pytest
import torch

from tests.util import nmax

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")


def ref_experts(x, idx, w, Wgu, Wd, G, act="silu"):
    """fp64 closed form: per expert a gather, gate/up, m = act(g) u, y = m Wd^T; out += w y.  Backward with the two 1/2 rules and the
    identity rule on act: G_y = 1/2 w G, G_m = G_y Wd, G_g = 1/2 G_m u act(g) / (g + 1e-10), G_u = 1/2 G_m act(g); G_w = 1/2 y . G"""
    x, w, Wgu, Wd, G = (a.double() for a in (x, w, Wgu, Wd, G))
    T, H = x.shape
    E, I = Wd.shape[0], Wd.shape[2]
    f = torch.nn.functional.silu if act == "silu" else (lambda z: torch.nn.functional.gelu(z, approximate="tanh"))
    out, gx, gw = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(w)
    for e in range(E):
        t, s = torch.where(idx == e)
        if t.numel() == 0:
            continue
        gu = x[t] @ Wgu[e].T
        g, u = gu[:, :I], gu[:, I:]
        a = f(g)
        y = (a * u) @ Wd[e].T
        out.index_add_(0, t, y * w[t, s, None])
        Gm = (0.5 * w[t, s, None] * G[t]) @ Wd[e]
        gx.index_add_(0, t, torch.cat([0.5 * Gm * u * a / (g + 1e-10), 0.5 * Gm * a], 1) @ Wgu[e])
        gw[t, s] = 0.5 * (y * G[t]).sum(1)
    return out, gx, gw


def make(T, k, E, H, I, dtype, seed=0, skew=None, skip=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T, H, device="cuda", generator=g)
    if skew is None:
        idx = torch.rand(T, E, device="cuda", generator=g).argsort(1)[:, :k]          # distinct experts per token
    else:
        hot = torch.tensor(skew, device="cuda")
        idx = torch.stack([hot[torch.randperm(len(skew), device="cuda", generator=g)[:k]] if torch.rand(1, device="cuda", generator=g) < 0.9
                           else torch.randperm(E, device="cuda", generator=g)[:k] for _ in range(T)])
    if skip:
        idx = torch.where(torch.rand(T, k, device="cuda", generator=g) < skip, torch.full_like(idx, E), idx)
    w = torch.rand(T, k, device="cuda", generator=g) / k
    Wgu = torch.randn(E, 2 * I, H, device="cuda", generator=g) / H ** 0.5
    Wd = torch.randn(E, H, I, device="cuda", generator=g) / I ** 0.5
    G = torch.randn(T, H, device="cuda", generator=g)
    return [a.to(dtype) for a in (x, w, Wgu, Wd, G)], idx


def run(x, idx, w, Wgu, Wd, G, act="silu"):
    from lxt_amd.efficient.moe import MoEExpertsFn
    x = x.clone().requires_grad_()
    w = w.clone().requires_grad_()
    out = MoEExpertsFn.apply(x, idx, w, Wgu, Wd, act)
    out.backward(G)
    torch.cuda.synchronize()
    return out.detach(), x.grad, w.grad


def cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


def test_plan_is_a_stable_sort_of_the_expert_ids():
    _need_gpu()
    import lxt_amd.ops as ops
    for T, k, E, skip in ((2048, 8, 128, 0.0), (777, 3, 5, 0.2), (1, 1, 4, 0.0), (300, 2, 16, 1.0)):
        idx = torch.randint(0, E, (T, k), device="cuda", generator=torch.Generator(device="cuda").manual_seed(T))
        if skip:
            idx = torch.where(torch.rand(T, k, device="cuda") < skip, torch.full_like(idx, E), idx)
        plan = ops.MoePlan(idx, E)
        cnt, off, perm, inv = (v.long().cpu() for v in plan.views())
        flat = idx.flatten().cpu()
        live = flat < E
        assert cnt.tolist() == torch.bincount(flat[live], minlength=E).tolist()
        assert off.tolist() == [0] + torch.cumsum(cnt, 0).tolist()
        order = torch.sort(torch.where(live, flat, E), stable=True).indices[:int(live.sum())]
        assert perm[:int(live.sum())].tolist() == order.tolist()
        want_inv = torch.full((T * k,), -1, dtype=torch.long)
        want_inv[order] = torch.arange(order.numel())
        assert inv.tolist() == want_inv.tolist()


CASES = [  # T, k, E, H, I, skew, skip
    pytest.param(512, 8, 128, 2048, 768, None, 0.0, id="30b_a3b_T512"),
    pytest.param(2048, 8, 128, 2048, 768, None, 0.0, id="30b_a3b_T2048"),
    pytest.param(600, 2, 16, 256, 384, [0, 5, 9], 0.0, id="skew_empty_experts"),
    pytest.param(1, 1, 8, 256, 128, None, 0.0, id="T1_k1"),
    pytest.param(40, 2, 8, 128, 256, None, 0.3, id="skipped_slots"),
]


# the fp32 parity path runs every case but the T = 2048 one (its fp32 GEMM is the correctness-first MFMA form; T = 512 covers those dims)
PARAMS = [pytest.param(*c.values, dt, id=f"{c.id}-{n}") for c in CASES for dt, n in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"))
          if not (dt == torch.float32 and c.values[0] == 2048)]


@pytest.mark.parametrize("T,k,E,H,I,skew,skip,dtype", PARAMS)
def test_experts_function_against_fp64(T, k, E, H, I, skew, skip, dtype):
    _need_gpu()
    (x, w, Wgu, Wd, G), idx = make(T, k, E, H, I, dtype, seed=T + E, skew=skew, skip=skip)
    out, gx, gw = run(x, idx, w, Wgu, Wd, G)
    r_out, r_gx, r_gw = ref_experts(x, idx, w, Wgu, Wd, G)
    errs = [nmax(out, r_out), nmax(gx, r_gx), nmax(gw, r_gw)]
    if dtype == torch.float32:
        assert max(errs) <= 1e-5, errs
    else:
        coss = [cos(out, r_out), cos(gx, r_gx), cos(gw, r_gw)]
        assert max(errs) <= 2e-2 and min(coss) >= 0.999, (errs, coss)
    if skip:
        assert (gw[idx == E] == 0).all()


def test_gelu_tanh_experts():
    _need_gpu()
    (x, w, Wgu, Wd, G), idx = make(200, 4, 8, 256, 256, torch.float32, seed=5)
    out, gx, gw = run(x, idx, w, Wgu, Wd, G, act="gelu_tanh")
    r = ref_experts(x, idx, w, Wgu, Wd, G, act="gelu_tanh")
    assert max(nmax(out, r[0]), nmax(gx, r[1]), nmax(gw, r[2])) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_deterministic_and_row_independent(dtype):
    """two runs are bit-identical; a token's output and gradients do not change by a bit when other tokens are appended or prepended -- what
    keeps prompts batch-invariant.  Appended tokens (the first 300 of 700 kept) change every expert's row count and so every expert's first
    plan row p0, but the plan is a stable sort: a kept token keeps its row index inside its expert, and with it its M tile and its MFMA row.
    Dropping the LEADING tokens (the last 300 kept) moves the kept rows inside their experts as well.  Planted moves by 1 / 127 / 128 rows,
    op by op: tests/test_moe_ops_gpu.py::test_rows_do_not_depend_on_their_position"""
    _need_gpu()
    (x, w, Wgu, Wd, G), idx = make(700, 8, 64, 512, 256, dtype, seed=3)
    a = run(x, idx, w, Wgu, Wd, G)
    b = run(x, idx, w, Wgu, Wd, G)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    n = 300
    c = run(x[:n], idx[:n], w[:n], Wgu, Wd, G[:n])
    assert all(torch.equal(u[:n], v) for u, v in zip(a, c))
    d = run(x[-n:], idx[-n:], w[-n:], Wgu, Wd, G[-n:])
    assert all(torch.equal(u[-n:], v) for u, v in zip(a, d))
    rank = lambda i: (i.flatten()[:, None] == i.flatten()[None, :]).tril(-1).sum(1)      # noqa: E731  (a slot's row index inside its expert)
    assert bool((rank(idx)[-n * idx.shape[1]:] != rank(idx[-n:])).any())


@pytest.mark.parametrize("case", ["tiny", "fanout", "padded"])
def test_qwen3_moe_drop_in_against_the_reference(case):
    """monkey_patch(modeling_qwen3_moe) + the quickstart protocol, eager and sdpa, fp32 against the reference's fp32 and fp64 relevance, bf16
    against its fp32 (fresh process per case: the patches are process-global)"""
    _need_gpu()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "moe_worker.py"), case], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
