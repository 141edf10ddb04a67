"""CPU: the MXFP4 expert weights of Qwen3MoeLRP (include/lrp_hip_moe_mxfp4.h, csrc/moe_mxfp4.hip) -- the four _q entry points are declared,
exported and reject bad calls before any launch, the wrappers refuse host tensors, the engine refuses an unknown format without a device, and
the COMPILED quantised grouped GEMMs keep the properties tests/test_moe_isa_cpu.py pins for the unquantised ones (no spills, the full MFMA
count in the K loop, the next stage's loads in flight under the MFMAs).  Numerics: tests/test_moe_mxfp4_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "lrp-explains-transformers_amd", "csrc", "moe_mxfp4.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

I64, VP, IP, FP = "int64_t", "void*", "int*", "float*"
SIGS = {
    "lrp_moe_gate_up_fwd_q": [VP, VP, VP, IP, VP, VP, "int", "int", "int", "int", "int", I64, I64, I64, "int", "int", VP],
    "lrp_moe_down_fwd_q": [VP, VP, VP, IP, VP, "int", "int", "int", "int", "int", I64, I64, "int", VP],
    "lrp_moe_down_dgrad_q": [VP, VP, VP, VP, VP, VP, IP, VP, FP, "int", "int", "int", "int", "int", I64, I64, I64, I64, "int", VP],
    "lrp_moe_gate_up_dgrad_q": [VP, VP, VP, IP, VP, "int", "int", "int", "int", "int", I64, I64, "int", VP],
}


def test_header_is_included_and_symbols_are_declared_and_exported():
    import lxt_amd._lib as L
    main = open(L.HEADER_PATH).read()
    assert '#include "lrp_hip_moe_mxfp4.h"' in main
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in SIGS.items():
        assert L.DECLS[name] == ("int", args), name
        assert hasattr(raw, name), name
        # the argument list of the unquantised sibling with `W` replaced by `codes, scales`
        sib = L.DECLS[name[:-2]][1]
        assert [a for i, a in enumerate(args) if i != 2] == sib, name
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)          # lrp_hip.h's own prototype count and the ABI version do not move
    assert len(re.findall(r"\b(?:int64_t|int|const char\*)\s+lrp_\w+\s*\([^)]*\)\s*;", own)) == 89 and L.lib.lrp_version() == 8


A = 1 << 12          # an aligned fake device address: every call below is rejected before a launch
# T 8, k 2, E 4, H 256, I 128, bf16, pitches = widths
OK = {
    "lrp_moe_gate_up_fwd_q": dict(x=A, codes=A, scales=A, plan=A, coef=A, m=A, T=8, k=2, E=4, H=256, I=128, ldx=256, ldcoef=256, ldm=128, act=None,
                                  dtype=None, stream=None),
    "lrp_moe_down_fwd_q": dict(m=A, codes=A, scales=A, plan=A, y=A, T=8, k=2, E=4, H=256, I=128, ldm=128, ldy=256, dtype=None, stream=None),
    "lrp_moe_down_dgrad_q": dict(G=A, codes=A, scales=A, coef=A, m=A, w=A, plan=A, Agu=A, part=A, T=8, k=2, E=4, H=256, I=128, ldg=256, ldcoef=256,
                                 ldm=128, ldagu=256, dtype=None, stream=None),
    "lrp_moe_gate_up_dgrad_q": dict(Agu=A, codes=A, scales=A, plan=A, gx=A, T=8, k=2, E=4, H=256, I=128, ldagu=256, ldgx=256, dtype=None,
                                    stream=None),
}


@pytest.mark.parametrize("fn", sorted(OK))
def test_argument_validation_without_gpu(fn):
    import lxt_amd._lib as L
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    ok = dict(OK[fn], dtype=L.BF16)
    if "act" in ok:
        ok["act"] = L.ACT["silu"]
    call = lambda **kw: getattr(L.lib, fn)(*{**ok, **kw}.values())      # noqa: E731
    for kw in (dict(codes=None), dict(scales=None), dict(plan=None), dict(dtype=7)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(codes=A + 8), dict(codes=A + 1), dict(scales=A + 2), dict(scales=A + 1)):
        assert call(**kw) == EALIGN, kw
    for kw in (dict(H=192), dict(I=64), dict(E=2048)):
        assert call(**kw) == ESHAPE, kw
    # the shape is judged before the pointers (the siblings' order), and what is fine passes the checks: scales on the 4-byte grid only
    assert call(H=192, codes=None) == ESHAPE
    assert call(scales=A + 4) not in (EINVAL, EALIGN, ESHAPE)
    assert call(dtype=L.F32) not in (EINVAL, EALIGN, ESHAPE)


def test_wrappers_refuse_cpu_tensors():
    from lxt_amd import ops
    w = torch.zeros(2, 256, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.MoeQuantWeight(w)
    q = ops.MoeQuantWeight.from_bytes(torch.zeros(2, 256, 64, dtype=torch.uint8), torch.zeros(2, 256, 4, dtype=torch.uint8))
    assert q.shape == (2, 256, 128)
    x = torch.zeros(4, 128, dtype=torch.bfloat16)

    class Plan:          # (never reached: the operands are refused first)
        T, k, E, rows, buf = 4, 1, 2, 4, torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.moe_down_fwd(x, q, Plan)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.moe_gate_up_dgrad(torch.zeros(4, 256, dtype=torch.bfloat16), q, Plan)
    with pytest.raises(RuntimeError, match="device tensors"):
        q.dequant(torch.bfloat16)
    with pytest.raises(ValueError, match="uint8"):
        ops.MoeQuantWeight.from_bytes(torch.zeros(2, 256, 64), torch.zeros(2, 256, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="scales"):
        ops.MoeQuantWeight.from_bytes(torch.zeros(2, 256, 64, dtype=torch.uint8), torch.zeros(2, 256, 8, dtype=torch.uint8))


def test_format_request_refuses_unknown_formats_without_a_device():
    from lxt_amd import engine_qwen_moe as M
    assert M.expert_format_request(None) is None and M.expert_format_request("mxfp4") == "mxfp4"
    for bad in ("int4", "nf4", "MXFP4", "", 4, True):
        with pytest.raises(ValueError, match="weight_format must be"):
            M.expert_format_request(bad)
    stub = M.Qwen3MoeLRP.__new__(M.Qwen3MoeLRP)          # the check is the first thing the constructor does: nothing of the object exists yet
    with pytest.raises(ValueError, match="weight_format must be"):
        stub.__init__(dict(hidden=128), dict(layers=[]), weight_format="int4")
    assert not hasattr(stub, "flat") and not hasattr(stub, "flat_q")
    with pytest.raises(TypeError, match="weight_fmt"):          # the keyword rides in a checked dict: a misspelling is refused like any other
        stub.__init__(dict(hidden=128), dict(layers=[]), weight_fmt="mxfp4")


def test_expert_bytes_arithmetic():
    """the capacity figures the feature is built for: 17 / 32 bytes per expert parameter"""
    from lxt_amd import engine_qwen_moe as M
    assert M.expert_bytes(48, 128, 2048, 768, None, torch.bfloat16) == 48 * 128 * 3 * 2048 * 768 * 2
    q30 = M.expert_bytes(48, 128, 2048, 768, "mxfp4", torch.bfloat16)
    assert q30 == 48 * 128 * 3 * 2048 * 768 * 17 // 32 and abs(q30 / 1e9 - 15.4) < 0.05
    q235 = M.expert_bytes(94, 128, 4096, 1536, "mxfp4", torch.bfloat16)
    assert abs(q235 / 1e9 - 120.6) < 0.05 and q235 < 288e9 < M.expert_bytes(94, 128, 4096, 1536, None, torch.bfloat16)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_quantised_k_loop_keeps_prefetch_in_flight(tmp_path):
    out = str(tmp_path / "moe_mxfp4.s")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "--cuda-device-only", "-S", SRC, "-o", out], check=True, capture_output=True, timeout=900)
    txt = open(out).read()
    funcs = [f for f in re.split(r"\n(?=_Z\S+:)", txt) if re.match(r"_Z\S*moe_gemm_kernel\S*:", f)]
    assert len(funcs) == 10, len(funcs)        # (gate/up fwd x {SiLU, tanh-GELU}, down fwd, down dgrad, gate/up dgrad) x {bf16, fp32}
    for f in funcs:
        name = f.split(":", 1)[0]
        L = f.split("\n")
        assert not any("ScratchSize" in ln and not ln.strip().endswith(": 0") for ln in L), f"{name}: register spills"
        found = []          # the K loop = the depth-2 loop holding the MFMAs (the extent rule of tests/test_moe_isa_cpu.py)
        for h in [i for i, ln in enumerate(L) if "Loop Header: Depth=2" in ln]:
            hline = next(j for j in range(h, h - 3, -1) if re.match(r"\.LBB\d+_\d+:", L[j].strip()))
            hlab = re.match(r"\.(LBB\d+_\d+):", L[hline].strip()).group(1)
            labs = {hlab} | {re.match(r"\.(LBB\d+_\d+):", ln.strip()).group(1) for ln in L
                             if re.match(r"\.LBB\d+_\d+:", ln.strip()) and "Header=" + hlab[1:] + " " in ln}
            starts = [i for i, ln in enumerate(L) if any(ln.strip().startswith("." + lb + ":") for lb in labs)]
            ends = [i for i, ln in enumerate(L) if any(re.search(r"s_c?branch\S*\s+\." + lb + r"\s*$", ln.split(";")[0].rstrip()) for lb in labs)]
            region = range(min(starts), max(ends) + 1)
            code = {i: L[i].split(";")[0].strip() for i in region}
            if any(c.startswith("v_mfma") for c in code.values()):
                hend = next(i for i in range(hline + 1, len(L)) if re.match(r"(\.LBB\d+_\d+:|; %bb\.)", L[i].strip())
                            or re.match(r"s_c?branch", L[i].strip()))
                found.append((code, range(hline, hend)))
        assert len(found) == 1, (name, len(found))
        code, header = found[0]
        mfma = sum(c.startswith("v_mfma") for c in code.values())
        assert mfma == (32 if "DF16b" in name else 128), (name, mfma)
        assert any(c.startswith("global_load") for c in code.values()), name
        stray = [c for i, c in code.items() if c.startswith("s_waitcnt") and "vmcnt" in c and i not in header]
        assert not stray, f"{name}: vmcnt wait outside the loop header (the stage's decode and LDS stores): {stray}"
