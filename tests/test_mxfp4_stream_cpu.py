"""CPU: the weight-streaming Linear on MXFP4 codes (include/lrp_hip_mxfp4_stream.h, csrc/linear_stream_q.hip) -- the two entry points are
declared, exported and bound; lrp_linear_stream_q_ok is the plain kernel's answer plus the format's pitch rules; bad calls are rejected before
any launch; the wrappers refuse host tensors; and the COMPILED kernel keeps what the design rests on: no spills, the decode and the plain
kernel's MFMA count per K tile inside the K loop, and no vmcnt(0) drain anywhere before the last MFMA.  Numerics: tests/test_mxfp4_stream_gpu.py."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "lrp-explains-transformers_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

I64, VP = "int64_t", "void*"
SIGS = {
    "lrp_linear_stream_q_ok": ["int", "int", "int", I64, I64, I64],
    "lrp_linear_stream_fwd_q": [VP, VP, VP, VP, VP, "int", "int", "int", I64, I64, I64, I64, "int", "int", VP, VP, VP],
}


def test_header_is_included_and_symbols_are_declared_exported_and_bound():
    import lxt_amd._lib as L
    main = open(L.HEADER_PATH).read()
    assert '#include "lrp_hip_mxfp4_stream.h"' in main
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in SIGS.items():
        assert L.DECLS[name] == ("int", args), name
        assert hasattr(raw, name) and callable(getattr(L.lib, name)), name
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)          # lrp_hip.h's own prototype count and the ABI version do not move
    assert len(re.findall(r"\b(?:int64_t|int|const char\*)\s+lrp_\w+\s*\([^)]*\)\s*;", own)) == 89 and L.lib.lrp_version() == 8


def test_q_ok_is_the_plain_answer_plus_the_pitch_rules():
    import lxt_amd._lib as L
    ok, plain = L.lib.lrp_linear_stream_q_ok, L.lib.lrp_linear_stream_ok
    seen = set()
    for M in (0, 1, 16, 17, 128, 129):
        for N in (64, 1024, 1536, 4096, 6144, 12288, 12300, 14336, 28672, 65600, 131072):
            for K in (256, 512, 768, 1024, 1536, 4096, 14336, 16384):
                for ldx in (K, K + 8, K + 4, K - 8):
                    want = plain(M, N, K, ldx, K)
                    assert ok(M, N, K, ldx, K // 2, K // 32) == want, (M, N, K, ldx)
                    assert ok(M, N, K, ldx, K // 2 + 16, K // 32 + 4) == want, (M, N, K, ldx)       # pitches beyond the row are fine
                    seen.add(want)
    assert seen == {0, 1}
    M, N, K = 4, 6144, 4096
    assert ok(M, N, K, K, K // 2, K // 32) == 1
    assert ok(M, N, K, K, K // 2 + 8, K // 32) == 0           # ldc % 16
    assert ok(M, N, K, K, K // 2, K // 32 + 2) == 0           # ldsc % 4
    assert ok(M, N, K, K, K // 2 - 16, K // 32) == 0          # ldc < K / 2
    assert ok(M, N, K, K, K // 2, K // 32 - 4) == 0           # ldsc < K / 32
    # the split policy is the plain entry's own (one definition): what the bit identity of the split form rests on
    assert [L.lib.lrp_linear_stream_fwd_splits(1, n, k) for n, k in ((4096, 1536), (6144, 4096), (4096, 4096), (1536, 4096), (12288, 512))] == [3, 2, 4, 8, 1]


A = 1 << 12          # an aligned fake device address: every call below is rejected before a launch
OK = dict(x=A, codes=A, scales=A, bias=None, z=A, M=4, N=6144, K=4096, ldx=4096, ldc=2048, ldsc=128, ldz=6144, dtype=None, out_dtype=None, ws=None,
          tickets=None, stream=None)


def test_argument_validation_without_gpu():
    import lxt_amd._lib as L
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    ok = dict(OK, dtype=L.BF16, out_dtype=L.BF16)
    call = lambda **kw: L.lib.lrp_linear_stream_fwd_q(*{**ok, **kw}.values())      # noqa: E731
    for kw in (dict(x=None), dict(codes=None), dict(scales=None), dict(z=None), dict(dtype=7), dict(out_dtype=7), dict(M=-1)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(dtype=L.F32), dict(M=129), dict(K=768, ldx=768, ldc=384, ldsc=24), dict(K=256, ldx=256, ldc=128, ldsc=8), dict(ldc=2032),
               dict(ldsc=124), dict(ldx=4088), dict(N=1 << 19)):
        assert call(**kw) == ESHAPE, kw
    for kw in (dict(x=A + 8), dict(codes=A + 8), dict(codes=A + 1), dict(ldc=2056), dict(ldx=4100), dict(scales=A + 2), dict(scales=A + 1),
               dict(ldsc=130)):
        assert call(**kw) == EALIGN, kw
    # the split form (ws and tickets given, a narrow weight): z / ldz / ws alignment as in the plain entry
    split = dict(N=4096, ldz=4096, ws=A, tickets=A)
    assert call(**split, z=A + 8) == EALIGN and call(**{**split, "ldz": 4098}) == EALIGN and call(**{**split, "ws": A + 4}) == EALIGN
    # nothing to do is not an error, and is decided before shapes and alignment are judged
    assert call(M=0) == 0 and call(N=0) == 0 and call(M=0, codes=A + 1, K=768) == 0
    # scales on the 4-byte grid only
    assert call(scales=A + 4, M=129) == ESHAPE and call(scales=A + 4, x=A + 8) == EALIGN


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    from lxt_amd import ops
    x = torch.zeros(4, 4096, dtype=torch.bfloat16)
    codes, scales = torch.zeros(6144, 2048, dtype=torch.uint8), torch.zeros(6144, 128, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.linear_stream_q_ok(x, codes, scales)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.linear_stream_fwd_q(x, codes, scales)


def _functions(txt, pat):
    return {f.split(":", 1)[0]: f.split("\n") for f in re.split(r"\n(?=_Z\S+:)", txt) if re.match(pat, f)}


def _tiles_and_mfmas(lines):
    """(K tiles, MFMAs) of a stream kernel's code: a K tile has ONE s_barrier, and the barriers of the epilogue come after the last MFMA"""
    code = [ln.split(";")[0].strip() for ln in lines]
    last = max(i for i, c in enumerate(code) if c.startswith("v_mfma"))
    return sum(c == "s_barrier" for c in code[:last]), sum(c.startswith("v_mfma_f32_16x16x32_bf16") for c in code), last


def test_compiled_k_loop_decodes_keeps_the_mfma_count_and_never_drains(tmp_path):
    asm = {}
    for name in ("linear_stream_q", "linear_stream"):
        out = str(tmp_path / (name + ".s"))
        subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", out], check=True, capture_output=True, timeout=900)
        asm[name] = open(out).read()
    q = _functions(asm["linear_stream_q"], r"_Z\S*linear_stream_q_fwd_kernel\S*:")
    plain = _functions(asm["linear_stream"], r"_Z\S*linear_stream_fwd_kernel\S*:")
    assert len(q) == 6 and len(plain) == 6, (sorted(q), sorted(plain))          # {fp32, bf16 output} x MBMAX {2, 4, 8}
    inst = lambda name: re.search(r"kernelI(\w+?Li\d+)EE", name).group(1)      # noqa: E731
    plain = {inst(n): L for n, L in plain.items()}
    for name, L in q.items():
        assert not any("ScratchSize" in ln and not ln.strip().endswith(": 0") for ln in L), f"{name}: register spills"
        assert not any(re.match(r"\s*scratch_", ln) for ln in L), f"{name}: scratch access"
        tiles, mfma, last = _tiles_and_mfmas(L)
        ptiles, pmfma, _ = _tiles_and_mfmas(plain[inst(name)])
        mb = int(re.search(r"Li(\d+)EE", name).group(1))
        assert tiles and mfma == tiles * 2 * mb and pmfma == ptiles * 2 * mb, (name, tiles, mfma, ptiles, pmfma)
        # the steady state: the basic blocks the compiler marks as loop bodies
        blocks, cur, inloop = [], [], False
        for ln in L:
            if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", ln.strip()):
                if cur and inloop:
                    blocks.append(cur)
                cur, inloop = [], ("Loop Header" in ln or "in Loop:" in ln)
            cur.append(ln.split(";")[0].strip())
        loop = [c for b in blocks for c in b]
        assert sum(c.startswith("v_cvt_scalef32_pk_bf16_fp4") for c in loop) >= 8, name
        ltiles = sum(c == "s_barrier" for c in loop)
        assert ltiles and ltiles % 4 == 0 and sum(c.startswith("v_mfma_f32_16x16x32_bf16") for c in loop) == ltiles * 2 * mb, (name, ltiles)
        assert sum(c.startswith("v_cvt_scalef32_pk_bf16_fp4") for c in loop) == 8 * ltiles, name          # 2 code words per lane and tile
        assert sum(c.startswith("buffer_load_dwordx4") and "lds" not in c for c in loop) == ltiles // 2, name      # 2 code loads per 4-tile group
        # no drain: every vmcnt wait up to the last MFMA (prologue and loop alike) leaves loads in flight
        waits = [ln.split(";")[0].strip() for ln in L[:last] if "s_waitcnt" in ln and "vmcnt" in ln]
        assert waits and not any(re.search(r"vmcnt\(0\)", w) for w in waits), (name, waits)
