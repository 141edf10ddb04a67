"""CPU: properties of the COMPILED grouped MoE GEMMs (csrc/moe.hip) that no numerics test sees -- no register spills, and a K loop whose
global loads of the next stage stay in flight under the current stage's MFMAs (no compiler-placed vmcnt wait between the prefetch loads and
the MFMAs of the same iteration).  hipcc cross-compiles the device code to assembly here (no GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "lrp-explains-transformers_amd", "csrc", "moe.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
def test_moe_gemm_k_loop_keeps_prefetch_in_flight(tmp_path):
    out = str(tmp_path / "moe.s")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "--cuda-device-only", "-S", SRC, "-o", out], check=True, capture_output=True, timeout=900)
    txt = open(out).read()
    funcs = [f for f in re.split(r"\n(?=_Z\S+:)", txt) if re.match(r"_Z\S*moe_gemm_kernel\S*:", f)]
    assert len(funcs) == 10, len(funcs)        # (gate/up fwd x {SiLU, tanh-GELU}, down fwd, down dgrad, gate/up dgrad) x {bf16, fp32}
    for f in funcs:
        name = f.split(":", 1)[0]
        L = f.split("\n")
        assert not any("ScratchSize" in ln and not ln.strip().endswith(": 0") for ln in L), f"{name}: register spills"
        # the K loop = the depth-2 loop holding the MFMAs; the compiler lays it out as [MFMA block] [header: vmcnt wait, LDS stores,
        # barrier] [prefetch loads of the next stage] with the back edge falling through, so its extent is first loop block ... last branch
        # into one of its blocks
        found = []
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
        assert mfma == (32 if "DF16b" in name else 128), (name, mfma)       # 2 macro steps x 16 tiles (fp32: 4 MFMAs per macro step)
        assert any(c.startswith("global_load") for c in code.values()), name
        waits = [(i, c) for i, c in code.items() if c.startswith("s_waitcnt") and "vmcnt" in c]
        stray = [c for i, c in waits if i not in header]
        assert not stray, f"{name}: vmcnt wait outside the loop header (the stage's LDS stores): {stray}"
