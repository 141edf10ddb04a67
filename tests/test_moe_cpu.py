"""CPU: the Qwen3-MoE drop-in (lxt_amd.efficient.models.qwen3_moe) and the lrp_moe_* entries of the C ABI, without a GPU."""
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_PATCH = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import lxt_amd
from lxt_amd.efficient import monkey_patch
from transformers.models.qwen3_moe import modeling_qwen3_moe as M
monkey_patch(M)
assert M.Qwen3MoeExperts.forward.__module__ == "lxt_amd.efficient.moe", M.Qwen3MoeExperts.forward.__module__
cfg = M.Qwen3MoeConfig(hidden_size=128, moe_intermediate_size=128, num_experts=4, num_experts_per_tok=2, num_hidden_layers=1,
                       num_attention_heads=2, num_key_value_heads=1, head_dim=64, vocab_size=64)
ex = M.Qwen3MoeExperts(cfg)
try:
    ex(torch.zeros(3, 128), torch.zeros(3, 2, dtype=torch.long), torch.ones(3, 2))
except RuntimeError as e:
    assert "no CPU fallback" in str(e), e
else:
    raise AssertionError("a CPU instance ran")
print("ok")
"""


def test_monkey_patch_qwen3_moe_in_a_fresh_process():
    """the map patches nn.Linear process-wide: run it in a child process"""
    r = subprocess.run([sys.executable, "-c", _PATCH, ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


def test_qwen3_moe_in_the_default_map():
    from lxt_amd.efficient.models import DEFAULT_MAP, _FAMILIES
    from transformers.models.qwen3_moe import modeling_qwen3_moe as M
    assert "qwen3_moe" in _FAMILIES and M in DEFAULT_MAP
    assert M.Qwen3MoeExperts in DEFAULT_MAP[M] and M.Qwen3MoeMLP in DEFAULT_MAP[M] and M.Qwen3MoeRMSNorm in DEFAULT_MAP[M]
    assert list(DEFAULT_MAP[M])[-1] is M                            # the modeling module (attention) is patched last


def test_moe_entries_declared_exported_and_validated():
    import ctypes
    import lxt_amd._lib as L
    lib, BF16, F32 = L.lib, L.BF16, L.F32
    names = ["lrp_moe_plan_ints", "lrp_moe_plan", "lrp_moe_gate_up_fwd", "lrp_moe_down_fwd", "lrp_moe_combine", "lrp_moe_down_dgrad",
             "lrp_moe_gw_reduce", "lrp_moe_gate_up_dgrad"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert n in L.DECLS and hasattr(raw, n), n
    assert lib.lrp_version() == 8
    # plan size: cnt E + off E+1 + toff E+1 + perm R + inv R + ceil(R / 256) E
    assert lib.lrp_moe_plan_ints(2048, 8, 128) == 3 * 128 + 2 + 2 * 16384 + 64 * 128
    assert lib.lrp_moe_plan_ints(4, 2, 2048) == -3 and lib.lrp_moe_plan_ints(0, 2, 8) == -3
    # plan: null / misaligned
    assert lib.lrp_moe_plan(None, 256, 4, 2, 8, None) == -1
    assert lib.lrp_moe_plan(260, 256, 4, 2, 8, None) == -2          # int64 index tensor not 8-byte aligned
    # gate/up forward: null, shape (H, I multiples of 128), alignment of every operand and pitch, activation
    a = (256, 256, 512, 768, 1024)                                 # x, Wgu, plan, coef, m (16-byte aligned fake addresses)
    ok = dict(T=4, k=2, E=8, H=128, I=128, ldx=128, ldc=256, ldm=128, act=0, dt=BF16)

    def gu(x=a[0], w=a[1], pl=a[2], c=a[3], m=a[4], **kw):
        d = dict(ok, **kw)
        return lib.lrp_moe_gate_up_fwd(x, w, pl, c, m, d["T"], d["k"], d["E"], d["H"], d["I"], d["ldx"], d["ldc"], d["ldm"], d["act"],
                                       d["dt"], None)
    assert gu(x=None) == -1 and gu(pl=None) == -1 and gu(m=None) == -1
    assert gu(H=192, ldx=192) == -3 and gu(I=96, ldc=192, ldm=96) == -3
    assert gu(x=264) == -2 and gu(c=770) == -2 and gu(w=1032) == -2
    assert gu(ldx=132) == -2 and gu(ldx=100) == -3 and gu(act=2) == -1 and gu(dt=7) == -1
    # the other entries
    assert lib.lrp_moe_down_fwd(None, 256, 512, 768, 4, 2, 8, 128, 128, 128, 128, BF16, None) == -1
    assert lib.lrp_moe_down_fwd(256, 256, 512, 776, 4, 2, 8, 128, 128, 128, 128, BF16, None) == -2
    assert lib.lrp_moe_combine(256, None, 512, 8, 4, 2, 8, 128, 128, 128, BF16, None) == -2
    assert lib.lrp_moe_combine(256, None, None, 768, 4, 2, 8, 128, 128, 128, BF16, None) == -1
    assert lib.lrp_moe_down_dgrad(256, 256, 512, 768, None, 1024, 1280, 1536, 4, 2, 8, 128, 128, 128, 256, 128, 256, BF16, None) == -1
    assert lib.lrp_moe_down_dgrad(256, 256, 512, 768, 1025, 1024, 1280, 1536, 4, 2, 8, 128, 128, 128, 256, 128, 256, BF16, None) == -2
    assert lib.lrp_moe_down_dgrad(256, 256, 512, 768, 1024, 1024, 1288, 1536, 4, 2, 8, 128, 128, 128, 256, 128, 256, BF16, None) == -2
    assert lib.lrp_moe_gw_reduce(None, 256, 512, 4, 2, 8, 128, BF16, None) == -1
    assert lib.lrp_moe_gw_reduce(258, 256, 512, 4, 2, 8, 128, BF16, None) == -2
    assert lib.lrp_moe_gate_up_dgrad(256, 256, 512, 768, 4, 2, 8, 128, 128, 256, 120, BF16, None) == -3
    assert lib.lrp_moe_gate_up_dgrad(256, 256, None, 768, 4, 2, 8, 128, 128, 256, 128, BF16, None) == -1


def test_moe_function_refuses_what_it_does_not_serve():
    import pytest
    import torch
    from lxt_amd.efficient.moe import experts_forward

    class Fake:
        pass
    ex = Fake()
    ex.act_fn, ex.gate_up_proj, ex.down_proj = torch.nn.SiLU(), torch.zeros(4, 256, 128), torch.zeros(4, 128, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        experts_forward(ex, torch.zeros(3, 128), torch.zeros(3, 2, dtype=torch.long), torch.ones(3, 2))
    import lxt_amd.ops as ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.MoePlan(torch.zeros(3, 2, dtype=torch.long), 4)
