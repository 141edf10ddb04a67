"""GPU: lrp_span_seed (include/lrp_hip_span.h), the head seed of an answer-span explanation, against an fp64 computation in the test.
The yardstick is torch's own fp32 CPU log_softmax / softmax (and the torch composition one-hot - softmax, scaled) on the SAME rows, measured
here against the same fp64 values; the kernel may be 4 x as far (another summation order).  A case stacks its R in {1, 3, 17} calls (21 rows),
so that both errors are maxima over the same 21 rows, not a single draw.  Logits spread over +-80: without the max subtraction exp overflows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RS = (1, 3, 17)
# row pitches per V: the row's own length, and padded ones on and off the 16-byte grid (V = 4099: 4100 serves fp32 vectors only, 4104 bf16 too)
PITCHES = {1: (1, 4), 7: (7, 8), 1000: (1000, 1003), 4099: (4099, 4100, 4104)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from lxt_amd import ops
    return ops


def rows(R, V, ld, seed):
    """-> logits [R, V] fp32 as a view of [R, ld] (CPU), idx (first row 0, last row V - 1), w (a 0 and a negative one among them), rstd"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.rand(R, ld, generator=g) * 160.0 - 80.0
    idx = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    idx[0], idx[-1] = 0, V - 1
    w = torch.randn(R, generator=g)
    w[R // 2] = 0.0
    if R > 1:
        w[-1] = -1.75
    return buf[:, :V], idx, w, torch.rand(R, generator=g) + 0.5


def reference(l, idx, w):
    """fp64 values, and what torch's fp32 CPU kernels give for the same rows"""
    i = idx.long()[:, None]
    hot = torch.zeros(l.shape, dtype=torch.float64).scatter_(1, i, 1.0)
    r64 = dict(logprob=torch.log_softmax(l.double(), -1).gather(1, i)[:, 0], seed=w.double()[:, None] * (hot - torch.softmax(l.double(), -1)))
    t32 = dict(logprob=torch.log_softmax(l, -1).gather(1, i)[:, 0], seed=w[:, None] * (hot.float() - torch.softmax(l, -1)))
    return r64, t32


def run(ops, l, idx, w, rstd, ld, objective, seed_dtype):
    R, V = l.shape
    dl = torch.empty(R, ld, device="cuda").copy_(torch.nn.functional.pad(l, (0, ld - V)))[:, :V]
    sd = None
    if objective == "logprob":
        sd = torch.full((R, ld), float("nan"), device="cuda", dtype=seed_dtype)[:, :V]
    return ops.span_seed(dl, idx.cuda(), w.cuda(), rstd.cuda(), objective, seed=sd), dl


@pytest.mark.parametrize("seed_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", sorted(PITCHES))
def test_span_seed_vs_fp64(ops, V, seed_dtype):
    for ld in PITCHES[V]:
        got, want, tor = {"logprob": [], "seed": []}, {"logprob": [], "seed": []}, {"logprob": [], "seed": []}
        for R in RS:
            l, idx, w, rstd = rows(R, V, ld, 1000 * V + R)
            r64, t32 = reference(l, idx, w)
            (logit, logprob, rs, seed), dl = run(ops, l, idx, w, rstd, ld, "logprob", seed_dtype)
            assert torch.equal(logit.cpu(), l.gather(1, idx.long()[:, None])[:, 0])                  # the stored value, bitwise
            assert torch.equal(rs.cpu(), w * rstd) and seed.dtype == seed_dtype
            assert not seed[R // 2].any() and float(rs[R // 2]) == 0.0                               # a zero-weight row: exactly 0
            again = ops.span_seed(dl, idx.cuda(), w.cuda(), rstd.cuda(), "logprob", seed_dtype=seed_dtype)
            assert all(torch.equal(x, y) for x, y in zip(again, (logit, logprob, rs, seed)))         # bitwise repeatable
            # the logit objective: the same logit / logprob / rs bits, no dense seed
            lo = ops.span_seed(dl, idx.cuda(), w.cuda(), rstd.cuda(), "logit")
            assert lo[3] is None and all(torch.equal(x, y) for x, y in zip(lo[:3], (logit, logprob, rs)))
            for k, v in (("logprob", logprob), ("seed", seed)):
                got[k].append(v.double().cpu())
                want[k].append(r64[k])
                tor[k].append(t32[k].double())
        err = lambda a, b: float(max((x - y).abs().max() for x, y in zip(a, b)))      # noqa: E731
        e_lp, t_lp = err(got["logprob"], want["logprob"]), err(tor["logprob"], want["logprob"])
        t_sd = err(tor["seed"], want["seed"])
        print(f"[span_seed V={V} ld={ld} seed {seed_dtype}] max abs err vs fp64 over {sum(RS)} rows: logprob {e_lp:.2e} (torch fp32 {t_lp:.2e})", end="")
        assert e_lp <= 4 * t_lp
        if seed_dtype == torch.float32:
            e_sd = err(got["seed"], want["seed"])
            e_sum, t_sum = (max(float(x.sum(1).abs().max()) for x in s) for s in (got["seed"], tor["seed"]))
            print(f"  seed {e_sd:.2e} (torch {t_sd:.2e})  |row sum| {e_sum:.2e} (torch {t_sum:.2e})")
            assert e_sd <= 4 * t_sd and e_sum <= 4 * t_sum
        else:          # the same bound plus the one rounding to bf16: 2^-8 relative
            over = max(float(((x - y).abs() - 2.0 ** -8 * y.abs()).max()) for x, y in zip(got["seed"], want["seed"]))
            print(f"  bf16 seed: max (|err| - 2^-8 |seed|) {over:.2e} (torch fp32 err {t_sd:.2e})")
            assert over <= 4 * t_sd


@pytest.mark.parametrize("seed_dtype", [torch.float32, torch.bfloat16])
def test_span_seed_at_the_llama3_vocabulary(ops, seed_dtype):
    """V = 128256, R = 4: the 1024-thread form, several vector passes per thread"""
    R, V = 4, 128256
    l, idx, w, rstd = rows(R, V, V, 7)
    r64, t32 = reference(l, idx, w)
    (logit, logprob, rs, seed), dl = run(ops, l, idx, w, rstd, V, "logprob", seed_dtype)
    assert torch.equal(logit.cpu(), l.gather(1, idx.long()[:, None])[:, 0]) and torch.equal(rs.cpu(), w * rstd)
    assert not seed[R // 2].any()
    e_lp, t_lp = (float((x.double().cpu() - r64["logprob"]).abs().max()) for x in (logprob, t32["logprob"]))
    e_sd, t_sd = (float((x.double().cpu() - r64["seed"]).abs().max()) for x in (seed, t32["seed"]))
    e_sum, t_sum = (float(x.double().cpu().sum(1).abs().max()) for x in (seed, t32["seed"]))
    print(f"[span_seed V={V} R={R} seed {seed_dtype}] logprob {e_lp:.2e} (torch {t_lp:.2e})  seed {e_sd:.2e} (torch {t_sd:.2e})  "
          f"|row sum| {e_sum:.2e} (torch {t_sum:.2e})")
    assert e_lp <= 4 * t_lp
    if seed_dtype == torch.float32:
        assert e_sd <= 4 * t_sd and e_sum <= 4 * t_sum
    else:
        assert float(((seed.double().cpu() - r64["seed"]).abs() - 2.0 ** -8 * r64["seed"].abs()).max()) <= 4 * t_sd
    again = ops.span_seed(dl, idx.cuda(), w.cuda(), rstd.cuda(), "logprob", seed_dtype=seed_dtype)
    assert all(torch.equal(x, y) for x, y in zip(again, (logit, logprob, rs, seed)))


def test_span_seed_arguments(ops):
    l = torch.zeros(2, 8, device="cuda")
    idx = torch.zeros(2, device="cuda", dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.span_seed(l, idx, objective="prob")
    with pytest.raises(TypeError):
        ops.span_seed(l, idx.long())
    with pytest.raises(RuntimeError):
        ops.span_seed(l.cpu(), idx)
    with pytest.raises(ValueError):
        ops.span_seed(l, idx, objective="logprob", seed=torch.empty(2, 7, device="cuda"))
    logit, logprob, rs, seed = ops.span_seed(l, idx)                     # no weights, no rstd: w = 1, no rs
    assert rs is None and seed is None and not logit.any() and torch.allclose(logprob, torch.full_like(logprob, -2.0794415))
    empty = ops.span_seed(l[:0], idx[:0], objective="logprob")           # R = 0: nothing launched
    assert empty[0].numel() == 0 and empty[3].shape == (0, 8)
