"""Worker (one process per model family -- the patches are class-level and process-global, like the reference's): a HF model whose
parameters ALL require grad under lxt_amd.efficient.monkey_patch on the GPU in fp32; every parameter gradient the fixture holds
(tests/golden/param_grads_<family>[_top].npz, the real reference in fp64) is compared at the project's fp32 bar."""
import importlib
import os
import sys
import warnings

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")
from tests.golden.hf_models import wsum  # noqa: E402
from tests.golden.make_golden_param_grads import build, explain  # noqa: E402
from tests.util import GOLDEN, load, t, nmax  # noqa: E402

BAR = 1e-4


def main(family):
    fx = load(f"param_grads_{family}.npz")
    ref = {k[2:]: v for k, v in fx.items() if k.startswith("g:")}
    if os.path.exists(os.path.join(GOLDEN, f"param_grads_{family}_top.npz")):
        ref.update({k[2:]: v for k, v in load(f"param_grads_{family}_top.npz").items() if k.startswith("g:")})
    from lxt_amd.efficient import monkey_patch
    monkey_patch(importlib.import_module(f"transformers.models.{family}.modeling_{family}"))
    model = build(family)
    assert abs(wsum(model) - float(fx["wsum"])) < 1e-6 * float(fx["wsum"]), "weights did not reproduce"
    model = model.cuda()
    assert all(p.requires_grad for p in model.parameters())
    idx, logit = explain(model, t(fx["ids"])[0].cuda())
    ok = idx == int(fx["idx"]) and abs(logit - float(fx["logit"])) < 1e-4
    print(f"[{family}] idx {idx} (fixture {int(fx['idx'])}) logit {logit:.6f} (fixture {float(fx['logit']):.6f})")
    named = dict(model.named_parameters())
    missing = [n for n, p in named.items() if p.grad is None]
    print(f"[{family}] parameters without a gradient: {missing}")
    ok = ok and not missing
    worst = 0.0
    for n, g in ref.items():
        p = named[n]
        same = p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device and tuple(g.shape) == tuple(p.shape)
        err = nmax(p.grad, g) if same else float("inf")
        if err > BAR or not same:
            print(f"[{family}] {n} {tuple(p.shape)}: normalised max {err:.2e} layout ok {same}")
        worst = max(worst, err)
    for n in fx["zero"].tolist():        # zero in exact arithmetic (a key bias under softmax): at most rounding noise of its query sibling's scale
        sib = ref[n.replace("key", "query")]
        err = float(named[n].grad.abs().max()) / float(abs(sib).max())
        print(f"[{family}] {n}: exactly zero in the reference; max |grad| / max |its query sibling's| {err:.2e}")
        worst = max(worst, err)
    print(f"[{family}] {len(ref)} parameter gradients compared")
    print(f"WORST {worst:.3e}")
    return 0 if ok and worst <= BAR else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
