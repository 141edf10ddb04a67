"""Worker of tests/test_cp_engine_gpu.py::test_engine_vs_dropin (one fresh process: class-level patches are process-global and never
un-patched): the three fixture models under lxt_amd.efficient.monkey_patch with the CP-LRP maps, fp32 on the device, each prompt of the
fixture's batch alone and un-padded, against LlamaLRP / QwenLRP(rule="cp") on the same model and against the fixture.  Prints WORST."""
import importlib
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from tests.util import load, nmax, t  # noqa: E402


def main():
    from lxt_amd.efficient import monkey_patch
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden.make_golden_generate import build
    worst = 0.0
    for name, fam, cls in (("llama", "llama", LlamaLRP), ("qwen2", "qwen2", QwenLRP), ("qwen3", "qwen3", QwenLRP)):
        fx = load(f"cp_{name}.npz")
        monkey_patch(importlib.import_module(f"transformers.models.{fam}.modeling_{fam}"),
                     importlib.import_module(f"lxt_amd.efficient.models.{fam}").cp_LRP)
        model = build(name)
        for p in model.parameters():
            p.requires_grad_(False)
        ids, lengths, S = t(fx["ids"]), fx["lengths"].tolist(), fx["ids"].shape[1]
        eng = cls.from_hf(model, dtype=torch.float32, rule="cp", max_seq=S)
        out = eng.explain(ids, lengths=lengths)
        model = model.cuda()
        for b, n in enumerate(lengths):
            e = model.get_input_embeddings()(ids[b: b + 1, S - n:].cuda()).requires_grad_()
            last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
            idx = int(last.argmax())
            assert idx == int(fx["idx"][b]) == int(out["idx"][b]), (idx, int(fx["idx"][b]))
            last[idx].backward()
            R = (e * e.grad)[0].sum(-1)
            e_eng, e_fx = nmax(out["R_tok"][b, S - n:], R), nmax(R, fx["R_tok"][b, S - n:])
            print(f"[cp {name} prompt {b} length {n}] engine vs drop-in {e_eng:.2e} | drop-in vs reference fp64 {e_fx:.2e}")
            worst = max(worst, e_eng, e_fx)
    print(f"WORST {worst:.3e}")
    return 0 if worst <= 1e-4 else 1


if __name__ == "__main__":
    sys.exit(main())
