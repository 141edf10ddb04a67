#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): span_gemma3.npz = answer-span explanations of
`lxt.efficient.monkey_patch(modeling_gemma3)` on the CPU in fp64 with eager attention -- the protocol, the cases a - d, the stored keys and
the linearity assertion of make_golden_span.py (whose explain / run_case / model_cases / all_fp64 run here unchanged), at S = 48.

Model: make_golden_generate_gemma3.build() -- hf_models.build_gemma3() (three sliding layers with a window of 32, one global) with seeded
non-trivial (1 + w) norm weights; a checksum of the weights is stored.  With S = 48 the explained positions (0, 17, 47; 42 .. 46; 20, 33)
lie on both sides of the window: rows 0 and 17 see every earlier key, rows from 32 on have lost their first keys in the sliding layers.
The whole pass is fp64: besides all_fp64(), HF's Gemma3RMSNorm.forward casts its input `.float()` whatever the model's dtype (the
reference patches `_norm` only); for this run an fp64 input and the fp64 weight keep their dtype there.  The rules are untouched."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

ISEED = 34


def norm_fp64(modeling_gemma3):
    def forward(self, x):
        if x.dtype != torch.float64:
            return self._norm(x.float()).mul(1.0 + self.weight.float()).type_as(x)
        return self._norm(x) * (1.0 + self.weight)

    modeling_gemma3.Gemma3RMSNorm.forward = forward


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from tests.golden import make_golden_span as gs
    gs.all_fp64()
    from lxt.efficient import monkey_patch
    from transformers.models.gemma3 import modeling_gemma3
    from tests.golden.hf_models import wsum
    from tests.golden.make_golden_generate_gemma3 import build
    monkey_patch(modeling_gemma3)
    norm_fp64(modeling_gemma3)
    ws = wsum(build())
    model = build().double()
    cfg = model.config
    np.savez_compressed(os.path.join(HERE, "span_gemma3.npz"), S=gs.S, wsum=ws, iseed=ISEED, window=int(cfg.sliding_window),
                        protocol=np.array(gs.PROTOCOL), **gs.model_cases("gemma3", model, cfg.vocab_size, ISEED, False))


if __name__ == "__main__":
    main(*sys.argv[1:2])
