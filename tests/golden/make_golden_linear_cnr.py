#!/usr/bin/env python3
"""Linear eps-rule fixture whose bits do not depend on the host CPU: linear_eps_cnr.npz.
The lin_*_Rin outputs of rules.npz carry the rounding of the capture host's MKL kernels (another x86 CPU takes another code path and
differs in the last bits).  Here the reference runs under MKL's conditional numerical reproducibility mode (MKL_CBWR=COMPATIBLE, one
thread), which gives the same bits on every x86 CPU; tests/test_oracle_golden.py runs the oracle under the same mode.  Inputs: the
lin_* inputs of rules.npz.  Run with the reference importable:
    PYTHONPATH=<reference checkout> python tests/golden/make_golden_linear_cnr.py
"""
import os
import sys

os.environ.update(MKL_CBWR="COMPATIBLE", MKL_NUM_THREADS="1", OMP_NUM_THREADS="1")     # before torch loads MKL
from functools import partial  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import lxt.explicit.functional as lf          # noqa: E402  (the reference)
import lxt.explicit.rules as lrules           # noqa: E402
from oracle import rules as orules            # noqa: E402  (ours)

if __name__ == "__main__":
    torch.set_num_threads(1)
    z0 = np.load(os.path.join(HERE, "rules.npz"))
    out = {}
    for tag in ("c1", "toy", "mid"):
        x, W, b, gg = (torch.from_numpy(z0[f"lin_{tag}_{k}"]) for k in "xWbg")
        for eps_tag, eps in (("f", 1e-6), ("r", 1e-8)):
            xr = x.clone().requires_grad_()
            if eps_tag == "f":
                z = lf.linear_epsilon(xr, W, b, eps)
            else:
                z = lrules.EpsilonRule(partial(F.linear, weight=W, bias=b), eps)(xr)
            R_in, = torch.autograd.grad(z, xr, z.detach() * gg)
            _, R_o = orules.linear_epsilon(x, W, b, F.linear(x, W, b) * gg, eps)
            assert torch.equal(R_o, R_in), ("linear", tag, eps_tag)
            out[f"lin_{tag}_{eps_tag}_Rin"] = R_in.numpy()
    np.savez_compressed(os.path.join(HERE, "linear_eps_cnr.npz"), **out)
    print("wrote linear_eps_cnr.npz: " + ", ".join(f"{k}{v.shape}" for k, v in out.items()))
