"""CPU: MXFP4 weight storage (lrp_mxfp4_quantize / lrp_mxfp4_dequant, LlamaLRP(weight_format="mxfp4")) -- the C ABI is declared and exported and
rejects bad calls before any launch, the engine refuses bad requests without a device, the byte accounting of the quantised layout, and the
fixture of the real reference (tests/golden/make_golden_mxfp4.py).  mx_quantize / mx_dequant below restate the format of
include/lrp_hip_mxfp4.h in torch; the GPU tests (tests/test_mxfp4_gpu.py) compare the kernels against them bit for bit, so they are checked on
their own here."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests.util import load

MAGS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
MIDS = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=torch.float64)
TIE_UP = torch.tensor([False, True, False, True, False, True, False])      # a tie goes to the code with m = 0: up where the code above is even
TIES = ((0.25, 0), (0.75, 1), (1.25, 1), (1.75, 2), (2.5, 2), (3.5, 4), (5.0, 4))      # value / X -> the magnitude it rounds to


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def mx_quantize(w):
    """w [rows, cols] float32 / bfloat16 (cols % 32 == 0) -> (codes uint8 [rows, cols / 2], scales uint8 [rows, cols / 32]), on the CPU"""
    rows, cols = w.shape
    x = w.detach().cpu().double().reshape(rows, cols // 32, 32)
    amax = x.abs().amax(-1)
    _, e = torch.frexp(amax)                                        # amax = m 2^e, m in [0.5, 1): floor(log2 amax) = e - 1
    E = torch.where(amax == 0, 0, (e.long() - 1 - 2 + 127).clamp(0, 254))
    a = (x.abs() * torch.ldexp(torch.ones((), dtype=torch.float64), 127 - E)[..., None])[..., None]      # |w| / X: exact
    c = ((a > MIDS) | ((a == MIDS) & TIE_UP)).sum(-1)
    c = (c | (((x < 0) & (c > 0)).long() << 3)).reshape(rows, cols // 2, 2)          # the sign, never on magnitude 0
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8), E.to(torch.uint8)


def mx_dequant(codes, scales, dtype):
    """-> [rows, cols] in dtype on the CPU, every value exact; E = 255 -> NaN"""
    rows = codes.shape[0]
    cb, E = codes.cpu().long(), scales.cpu().long()
    c = torch.stack((cb & 15, cb >> 4), -1).reshape(rows, -1, 32)
    X = torch.ldexp(torch.ones((), dtype=torch.float64), E - 127).masked_fill(E == 255, float("nan"))
    v = torch.where(c >> 3 == 1, -1.0, 1.0).double() * MAGS[c & 7] * X[..., None]
    return v.reshape(rows, -1).to(dtype)


def test_restatement_decodes_every_code_and_scale():
    for E in (0, 1, 2, 100, 127, 130, 252, 253, 254):
        codes = (torch.arange(16) | (torch.arange(16) << 4)).to(torch.uint8).repeat(1, 1)          # every code, in both nibbles
        scales = torch.tensor([[E]], dtype=torch.uint8)
        v = mx_dequant(codes, scales, torch.float64)
        X = 2.0 ** (E - 127)
        want = torch.cat((MAGS, -MAGS)).repeat_interleave(2) * X
        assert torch.equal(v[0], want), E
        if 8 <= E <= 252:          # out of the subnormal range, and where 6 X is finite (the quantiser's E <= 252), both types hold every value
            for dt in (torch.float32, torch.bfloat16):
                assert torch.equal(mx_dequant(codes, scales, dt)[0].double(), want), (E, dt)
    assert mx_dequant(torch.zeros(1, 16, dtype=torch.uint8), torch.tensor([[255]], dtype=torch.uint8), torch.float32).isnan().all()


def test_restatement_rounding_saturation_zero_and_sign():
    for k in (-20, 0, 7):
        X = 2.0 ** k
        blk = torch.zeros(1, 32, dtype=torch.float32)
        blk[0, 0] = 6.0 * X                                       # amax in [4, 8) X: the scale is X
        for i, (v, _) in enumerate(TIES):
            blk[0, 1 + i], blk[0, 9 + i] = v * X, -v * X
        blk[0, 20], blk[0, 21], blk[0, 22] = -0.0, -0.1 * X, 0.26 * X
        codes, scales = mx_quantize(blk)
        assert int(scales[0, 0]) == k + 127
        mag = mx_dequant(codes, scales, torch.float64)[0] / X
        for i, (v, to) in enumerate(TIES):
            assert float(mag[1 + i]) == to and float(mag[9 + i]) == -to, (v, to)
        c = torch.stack((codes & 15, codes >> 4), -1).reshape(-1)
        assert int(c[20]) == 0 and int(c[21]) == 0 and int(c[1]) == 0 and int(c[9]) == 0          # magnitude 0 never carries a sign
        assert float(mag[22]) == 0.5
    # values in (6, 8) X saturate to 6: an amax one bf16 ulp below a power of two keeps the scale of the binade below
    sat = torch.zeros(1, 32, dtype=torch.bfloat16)
    sat[0, 3] = torch.tensor(8.0 - 2.0 ** -5, dtype=torch.bfloat16)          # 7.96875 = 8 (1 - 2^-8)
    sat[0, 4], sat[0, 5] = -7.0, 6.5
    codes, scales = mx_quantize(sat)
    assert int(scales[0, 0]) == 127 and mx_dequant(codes, scales, torch.float32)[0, 3:6].tolist() == [6.0, -6.0, 6.0]
    # an exact power of two is 4 X; an all-zero block is E = 0 and codes 0
    p2 = torch.zeros(2, 32)
    p2[0, 7] = 2.0 ** -9
    codes, scales = mx_quantize(p2)
    assert scales.view(-1).tolist() == [127 - 9 - 2, 0] and int(codes[0, 3]) == 6 << 4 and not codes[1].any()
    # the clamp: a block below 2^-125 keeps E = 0
    tiny = torch.full((1, 32), 2.0 ** -126)
    assert int(mx_quantize(tiny)[1][0, 0]) == 0 and float(mx_dequant(*mx_quantize(tiny), torch.float32)[0, 0]) == 2.0 ** -126


def test_restatement_round_trip_is_the_identity_on_codes():
    g = torch.Generator().manual_seed(5)
    for dt in (torch.float32, torch.bfloat16):
        w = (torch.randn(24, 256, generator=g) * torch.exp2(torch.randint(-30, 31, (24, 8, 1), generator=g).float()).expand(24, 8, 32)
             .reshape(24, 256)).to(dt)
        w[3, 32:64] = 0
        codes, scales = mx_quantize(w)
        c2, s2 = mx_quantize(mx_dequant(codes, scales, dt))
        assert torch.equal(c2, codes) and torch.equal(s2, scales)
        top = torch.stack((codes & 7, (codes >> 4) & 7), -1).reshape(24, 8, 32).amax(-1)          # a non-zero block's largest code is 4 or 6
        assert set(top.view(-1).tolist()) <= {0, 6, 7} and int(top[3, 1]) == 0


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_counted():
    import lxt_amd._lib as L
    sig = ("int", ["void*", "void*", "void*", "int", "int", "int64_t", "int64_t", "int64_t", "int", "void*"])
    assert L.DECLS["lrp_mxfp4_quantize"] == sig and L.DECLS["lrp_mxfp4_dequant"] == sig
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "lrp_mxfp4_quantize") and hasattr(raw, "lrp_mxfp4_dequant")
    main = open(L.HEADER_PATH).read()
    assert '#include "lrp_hip_mxfp4.h"' in main
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert len(re.findall(r"\b(?:int64_t|int|const char\*)\s+lrp_\w+\s*\([^)]*\)\s*;", own)) == 89 and L.lib.lrp_version() == 8
    from lxt_amd import ops
    assert callable(ops.mxfp4_quantize) and callable(ops.mxfp4_dequant)


@pytest.mark.parametrize("fn", ["lrp_mxfp4_quantize", "lrp_mxfp4_dequant"])
def test_argument_validation_without_gpu(fn):
    import lxt_amd._lib as L
    A = 1 << 12                                   # an aligned fake device address: every call below is rejected before a launch
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    # a [48, 256] bf16 matrix (pitch 264), codes [48, 128] (pitch 144), scales [48, 8]
    if fn == "lrp_mxfp4_quantize":
        ok = dict(w=A, codes=A, scales=A, rows=48, cols=256, ldw=264, ldc=144, lds=8, dtype=L.BF16, stream=None)
    else:
        ok = dict(codes=A, scales=A, w=A, rows=48, cols=256, ldc=144, lds=8, ldw=264, dtype=L.BF16, stream=None)
    call = lambda **kw: getattr(L.lib, fn)(*{**ok, **kw}.values())      # noqa: E731
    for kw in (dict(w=None), dict(codes=None), dict(scales=None), dict(dtype=2), dict(dtype=-1)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(rows=0), dict(rows=-3), dict(cols=0), dict(cols=16), dict(cols=240), dict(cols=272, ldw=272), dict(ldw=248), dict(ldc=112),
               dict(lds=4), dict(rows=1 << 30, cols=64, ldw=64, ldc=32, lds=4)):
        assert call(**kw) == ESHAPE, kw
    for kw in (dict(w=A + 8), dict(w=A + 2), dict(codes=A + 8), dict(scales=A + 2), dict(scales=A + 1), dict(ldw=260), dict(ldc=136), dict(lds=10),
               dict(dtype=L.F32, w=A + 4), dict(dtype=L.F32, ldw=258)):
        assert call(**kw) == EALIGN, kw
    # what is fine: a scale row on the 4-byte grid only, an fp32 pitch of a multiple of 4 elements (a launch without a device fails: -4)
    for kw in (dict(scales=A + 4), dict(dtype=L.F32, ldw=260), dict(rows=1, cols=32, ldw=32, ldc=16, lds=4)):
        assert call(**kw) not in (EINVAL, EALIGN, ESHAPE), kw


def test_binding_rejects_cpu_tensors_and_wrong_shapes():
    from lxt_amd import ops
    w = torch.zeros(4, 64, dtype=torch.bfloat16)
    codes, scales = torch.zeros(4, 32, dtype=torch.uint8), torch.zeros(4, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.mxfp4_quantize(w)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.mxfp4_dequant(codes, scales, w)
    meta = lambda *s, dt=torch.uint8: torch.empty(*s, dtype=dt, device="meta")      # noqa: E731  (is_cuda is False: refused like a CPU tensor)
    with pytest.raises(RuntimeError):
        ops.mxfp4_quantize(meta(4, 64, dt=torch.bfloat16))


# ---- the engine's request checks and byte accounting -----------------------------------------------------------------------------------------
CFG_8B = dict(hidden=4096, inter=14336, n_layers=32, n_heads=32, n_kv=8, head_dim=128, vocab=128256, rope_theta=500000.0, rms_eps=1e-5)


def test_weight_format_refused_without_a_device():
    from lxt_amd import engine as E
    from lxt_amd.engine_qwen import QwenLRP
    ok = dict(hidden=64, inter=128, n_layers=1, n_heads=2, n_kv=1, head_dim=32, vocab=32, rope_theta=1e4, rms_eps=1e-5)
    assert E.weight_format_request(None, ok) is None and E.weight_format_request("mxfp4", ok) == "mxfp4"
    assert E.weight_format_request(None, dict(ok, hidden=50)) is None          # (no constraint without a format)
    for cls in (E.LlamaLRP, QwenLRP):
        for bad in ("nf4", "fp4", "MXFP4", "", 4, True):
            with pytest.raises(ValueError, match="weight_format must be"):
                cls(ok, dict(layers=[]), weight_format=bad)
        # a K off the 32 grid: hidden (q/k/v, gate/up), n_heads * head_dim (o), inter (down)
        for cfg, what in ((dict(ok, hidden=80), "hidden"), (dict(ok, n_heads=3, head_dim=16, n_kv=1), "n_heads"), (dict(ok, inter=144), "inter")):
            with pytest.raises(ValueError, match=what):
                cls(cfg, dict(layers=[]), weight_format="mxfp4")
        stub = cls.__new__(cls)          # (the check is the first thing the constructor does: nothing of the object exists yet)
        with pytest.raises(ValueError, match="weight_format must be"):
            stub.__init__(ok, dict(layers=[]), weight_format="int4")
        assert not hasattr(stub, "flat")


def test_other_drivers_do_not_take_the_keyword():
    import inspect
    from lxt_amd.engine_bert import BertLRP
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_gemma3_mm import Gemma3MMLRP
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    for cls in (BertLRP, Gemma3LRP, Gemma3MMLRP, Qwen3MoeLRP):
        assert "weight_format" not in inspect.signature(cls.__init__).parameters, cls


def test_quantised_layout_bytes_8b():
    from lxt_amd import engine as E
    bf = torch.bfloat16
    top, layer = E.LlamaLRP.flat_layout(CFG_8B, bf)
    rest, lin, q = E.quant_layout(layer)
    assert tuple(lin) == E.MX_MATRICES and set(rest) == {"ln1", "ln2"} and len(q) == 8
    nL = CFG_8B["n_layers"]
    flat_q, _, qlayers = E.pack_flat({}, q, nL, torch.uint8, "meta", align=128)
    exact = nL * sum(N * K // 2 + N * K // 32 for (N, K), _ in lin.values())
    assert exact == nL * 218103808 * 17 // 32                            # 4.25 bits per element of the 218.1 M per layer
    assert flat_q.dtype == torch.uint8 and exact <= flat_q.numel() <= exact + 127 * 8 * nL
    for Q, (name, ((N, K), _)) in ((Q, it) for Q in (qlayers[0], qlayers[-1]) for it in lin.items()):
        c, s = Q[name + "_c"], Q[name + "_s"]
        assert tuple(c.shape) == (N, K // 2) and tuple(s.shape) == (N, K // 32) and c.stride(0) % 16 == 0 and s.stride(0) % 4 == 0
        assert c.storage_offset() % 128 == 0 and s.storage_offset() % 128 == 0          # every view starts 128-byte aligned
    # against the bf16 layout: the Linears shrink to <= 0.27 of their bytes, everything else stays in `flat`
    full = E.pack_flat(top, layer, nL, bf, "meta")[0].numel() * 2
    kept = E.pack_flat(top, rest, nL, bf, "meta")[0].numel() * 2
    assert flat_q.numel() <= 0.27 * (full - kept)
    scratch = E.pack_flat({}, lin, 1, bf, "meta")[0].numel() * 2
    assert abs(scratch - (full - kept) / nL) <= 4 * 128 and 2 * 218103808 <= scratch < 1.03 * 2 * 218103808          # (436 MB of elements, the pitch padding on top)
    # a K / 32 that is no multiple of 4: the scale rows keep a pitch on the 4-byte grid
    small = dict(CFG_8B, hidden=96, inter=160, n_heads=3, n_kv=1, head_dim=32, vocab=64, n_layers=2)
    _, _, q = E.quant_layout(E.LlamaLRP.flat_layout(small, bf)[1])
    assert q["wqkv_s"] == ((160, 3), 4) and q["wd_s"] == ((96, 5), 8) and q["wqkv_c"] == ((160, 48), None)
    # the default layout is untouched by the new parameter
    assert E.pack_flat(top, layer, nL, bf, "meta", align=64)[0].numel() * 2 == full


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_identities():
    from oracle import llama as ol
    fx = load("mxfp4_llama.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    S = int(fx["S"])
    assert fx["ids"].shape == (S,) and fx["R_tok"].shape == (S,) and fx["R_tok"].dtype == np.float64 and np.isfinite(fx["R_tok"]).all()
    assert np.abs(fx["R_tok"]).max() > 0 and 0 <= int(fx["idx"]) < cfg["vocab"] and "quantise-dequantise" in str(fx["protocol"])
    assert float(fx["ref_fp32_gap"]) <= 1e-5                     # the reference's own fp32 rounding on this instance: tenfold under the 1e-4 bar
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    assert abs(tot - float(fx["wsum"])) <= 1e-9 * abs(tot)
    # the generator's numpy restatement and the torch one above agree on the stored matrix, byte for byte
    H, I = cfg["hidden"], cfg["inter"]
    assert fx["wd_codes"].shape == (H, I // 2) and fx["wd_scales"].shape == (H, I // 32) and fx["wd_codes"].dtype == np.uint8
    codes, scales = mx_quantize(W["layers"][0]["wd"])
    assert np.array_equal(codes.numpy(), fx["wd_codes"]) and np.array_equal(scales.numpy(), fx["wd_scales"])
    c2, s2 = mx_quantize(mx_dequant(codes, scales, torch.float32))
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
