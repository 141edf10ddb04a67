"""CPU: a property of the COMPILED token-contracting kernels (csrc/wgrad.hip, csrc/moe_wgrad.hip) that no numerics test sees.  Their LDS layout,
transposed fragment read and staging store are csrc/wgrad_tiles.hpp's, and the grouped kernel also calls its MFMA block and accumulator
walk: the seven bf16 kernels must keep their accumulators and fragments in registers (no scratch), and one pass of the token loop must be
exactly the 2 x (16 ds_read_b64_tr_b16 + 16 v_mfma_f32_16x16x32_bf16) of one staged 64-token tile -- nothing unrolled twice, nothing
hoisted out or duplicated by a helper that did not inline.  hipcc cross-compiles the device code to assembly here (no GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "lrp-explains-transformers_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the seven bf16 kernels by their template arguments as they stand in the mangled names (<RS, PLAIN> dense, <MODE, Q> grouped)
KERNELS = {"wgrad": ("wgrad_rel_bf16_kernel", ("ILb1ELb0EE", "ILb0ELb0EE", "ILb0ELb1EE")),
           "moe_wgrad": ("moe_wgrad_bf16_kernel", ("ILi0ELb0EE", "ILi1ELb0EE", "ILi0ELb1EE", "ILi1ELb1EE"))}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_bf16_token_loop_is_one_tile_of_mfmas_and_no_scratch(tmp_path, src):
    out = str(tmp_path / (src + ".s"))
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "--cuda-device-only", "-S", os.path.join(CSRC, src + ".hip"), "-o", out], check=True, capture_output=True, timeout=900)
    txt = open(out).read()
    kernel, instances = KERNELS[src]
    funcs = {f.split(":", 1)[0]: f for f in re.split(r"\n(?=_ZN\S+:)", txt) if re.match(r"_ZN\S*" + kernel + r"\S*:", f)}
    for inst in instances:
        name = next(n for n in funcs if kernel + inst in n)          # (StopIteration: the instantiation is gone)
        L = funcs[name].split("\n")
        scratch = [ln for ln in L if "ScratchSize" in ln]
        assert scratch and all(ln.strip().endswith(": 0") for ln in scratch), f"{name}: register spills"
        # the token loop: the kernel's one loop, from its header block to the last branch back to it
        hdr = next(i for i, ln in enumerate(L) if "Loop Header: Depth=1" in ln)
        label = re.match(r"(\.LBB\d+_\d+):", L[hdr].strip()).group(1)
        end = max(i for i, ln in enumerate(L) if re.search(r"s_c?branch\S*\s+" + re.escape(label) + r"\s*$", ln.split(";")[0].rstrip()))
        body = [ln.split(";")[0].strip() for ln in L[hdr:end + 1]]
        mfma = sum(b.startswith("v_mfma_f32_16x16x32_bf16") for b in body)
        reads = sum(b.startswith("ds_read_b64_tr_b16") for b in body)
        assert (mfma, reads) == (32, 32), (name, mfma, reads)
