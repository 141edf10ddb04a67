#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): mxfp4_llama.npz = the reference's explanation of a seeded Llama whose
seven Linear weights per layer were replaced by their MXFP4 quantise-dequantise images -- what a weight-only quantised model computes:
"dequantise, then the usual Linear and its LRP backward on the dequantised matrix" (ref examples/quantized_llama.py, there through
bitsandbytes).  `lxt.efficient.monkey_patch(modeling_llama)` (ref lxt/efficient/models/llama.py:9-14), CPU, eager attention, fp64; the arg-max
logit of the last position seeded with 1, R_tok = (e * e.grad).sum(-1).

The format is restated here in numpy, independently of the kernels and of the tests' torch restatement (include/lrp_hip_mxfp4.h states it in
full): blocks of 32 along the columns, scale byte E = floor(log2 amax) - 2 + 127 clamped to [0, 254] (0 for an all-zero block), codes = the
nearest of 0, 0.5, 1, 1.5, 2, 3, 4, 6 to |w| / 2^(E - 127), ties to the even code, sign in bit 3 (never on magnitude 0), two codes per byte,
low nibble first.

Frozen: ids [S], idx, logit, R_tok [S] fp64, and the codes / scales of layer 0's down projection (`wd_codes` [H, I / 2], `wd_scales`
[H, I / 32]: the engine stores that matrix as HF holds it).  Weights: oracle.llama.random_weights(cfg, seed=wseed), pinned by wsum.

Asserted before anything is written: the reference run in fp32 on the same weights is within 1e-5 (normalised max) of its fp64 run and picks
the same logit -- the 1e-4 bar of the fp32 engine test then has tenfold room on the reference's own rounding.  4-bit weights on a random-init
model can be badly conditioned for the eps = 0 rules; a seed that does not give that is replaced and the one used is recorded (wseed, iseed)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

CFG = dict(hidden=256, inter=512, n_layers=4, n_heads=8, n_kv=2, head_dim=32, vocab=512, rope_theta=500000.0, rms_eps=1e-5)
S, WSEED, ISEED = 64, 2, 12
LINEARS = ("wq", "wk", "wv", "wo", "wg", "wu", "wd")
MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
MAX_BYTES = 1 << 20              # of one .npz: the size limit of a committed file
FP32_BAR = 1e-5


def mx_quantize(w):
    """w [rows, cols] float32 -> (codes uint8 [rows, cols / 2], scales uint8 [rows, cols / 32])"""
    rows, cols = w.shape
    x = w.astype(np.float64).reshape(rows, cols // 32, 32)
    amax = np.abs(x).max(-1)
    _, e = np.frexp(amax)                                       # amax = m 2^e with m in [0.5, 1): floor(log2 amax) = e - 1
    E = np.where(amax == 0, 0, np.clip(e - 1 - 2 + 127, 0, 254)).astype(np.int64)
    a = np.abs(x) / np.ldexp(1.0, E - 127)[..., None]
    mid = (MAGS[1:] + MAGS[:-1]) / 2                            # 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5
    up = np.array([False, True, False, True, False, True, False])      # a tie goes to the even code: up where the code above is even
    c = ((a[..., None] > mid) | ((a[..., None] == mid) & up)).sum(-1)
    c = (c | (((x < 0) & (c > 0)) << 3)).reshape(rows, cols // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).astype(np.uint8), E.astype(np.uint8)


def mx_dequant(codes, scales):
    """-> float64 [rows, cols], every value exact"""
    rows = codes.shape[0]
    c = np.stack((codes & 15, codes >> 4), -1).reshape(rows, -1, 32).astype(np.int64)
    v = np.where(c >> 3 == 1, -1.0, 1.0) * MAGS[c & 7] * np.ldexp(1.0, scales.astype(np.int64) - 127)[..., None]
    return v.reshape(rows, -1)


def wsum(W):
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    return tot


def explain(model, ids):
    e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
    last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
    idx = int(last.argmax())
    last[idx].backward()
    return idx, float(last[idx]), (e * e.grad)[0].sum(-1).detach().double()


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from transformers.models.llama import modeling_llama
    from oracle import llama as ol
    from tests.golden.hf_models import build_llama_from_weights
    monkey_patch(modeling_llama)
    W = ol.random_weights(CFG, seed=WSEED)
    total = wsum(W)                                              # (of the ORIGINAL weights: what the engine under test is given)
    Wq = dict(W, layers=[dict(L) for L in W["layers"]])
    kept = None
    for li, L in enumerate(Wq["layers"]):
        for k in LINEARS:
            codes, scales = mx_quantize(L[k].numpy())
            img = mx_dequant(codes, scales)
            c2, s2 = mx_quantize(img.astype(np.float32))
            assert np.array_equal(c2, codes) and np.array_equal(s2, scales), "quantise(dequant(q)) != q"
            assert np.array_equal(img.astype(np.float32).astype(np.float64), img)
            L[k] = torch.from_numpy(img.astype(np.float32))
            if (li, k) == (0, "wd"):
                kept = codes, scales
    ids = torch.randint(0, CFG["vocab"], (S,), generator=torch.Generator().manual_seed(ISEED))
    idx, logit, R = explain(build_llama_from_weights(CFG, Wq, attn="eager", dtype=torch.float64), ids)
    idx32, _, R32 = explain(build_llama_from_weights(CFG, Wq, attn="eager", dtype=torch.float32), ids)
    gap = float((R32 - R).abs().max() / R.abs().max())
    print(f"idx {idx} logit {logit:+.6f}  sum R_tok {float(R.sum()):+.6f}  reference fp32 vs fp64: idx {idx32}, normalised max {gap:.2e}")
    assert idx32 == idx and gap <= FP32_BAR, "badly conditioned instance: choose another seed"
    path = os.path.join(HERE, "mxfp4_llama.npz")
    np.savez_compressed(path, cfg_keys=np.array(list(CFG.keys())), cfg_vals=np.array([float(v) for v in CFG.values()]), S=S, wseed=WSEED,
                        iseed=ISEED, wsum=total, ids=ids.numpy(), idx=idx, logit=logit, R_tok=R.numpy(), ref_fp32_gap=gap,
                        wd_codes=kept[0], wd_scales=kept[1],
                        protocol=np.array("lxt.efficient.monkey_patch(modeling_llama), fp64, CPU, eager attention, on the MXFP4 "
                                          "quantise-dequantise images of the seven Linear weights of every layer; arg-max logit of the last "
                                          "position seeded 1"))
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    main(*sys.argv[1:2])
