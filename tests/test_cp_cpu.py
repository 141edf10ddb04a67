"""CPU: the CP-LRP surface without a device.
  * lrp_attn_bwd_dv / lrp_attn_bwd_dv_ok / lrp_gated_cp_bwd_il are declared in include/lrp_hip_attn_cp.h, exported and bound; their argument
    checks return before any HIP call, so the library is driven with integers as pointers (16: aligned, 8: misaligned, 0: NULL);
  * the ops wrappers refuse mixed dtypes, non-fp32 statistics and CPU tensors;
  * the `rule` keyword and cp_request raise on a stub without a device; the drivers that do not serve rule= do not take it;
  * the three fixtures cp_{llama,qwen2,qwen3}.npz (the real reference, make_golden_cp.py) equal oracle/hf_efficient.py's
    patch_instance(model, "cp") restatement in fp64."""
import inspect

import numpy as np
import pytest
import torch

from tests.util import load, nmax

F32, BF16 = 0, 1
EINVAL, EALIGN, ESHAPE, OK = -1, -2, -3, 0
DV = "q k G G_t lse dv B S Hq Hkv d ldq ldk ldg ldt lddv scale q_begin row_lo row_hi dtype stream".split()
GATED = "Gm gu Agu M I ldgm ldgu ldagu act dtype stream".split()


@pytest.fixture(scope="module")
def L():
    import lxt_amd._lib as lib
    return lib


def dv_call(dt_, d_, **change):
    """a well-formed call (B 2, S 40, Hq 4, Hkv 2, dense pitches, ldt = 64, no row intervals) with `change` applied; never issued unchanged"""
    a = dict(q=16, k=16, G=16, G_t=16, lse=16, dv=16, B=2, S=40, Hq=4, Hkv=2, d=d_, ldq=4 * d_, ldk=2 * d_, ldg=4 * d_, ldt=64, lddv=2 * d_,
             scale=0.125, q_begin=0, row_lo=None, row_hi=None, dtype=dt_, stream=None)
    a.update(change)
    return [a[n] for n in DV]


def test_entries_declared_exported_bound(L):
    assert [t for t in L.DECLS["lrp_attn_bwd_dv"][1]] == ["void*"] * 4 + ["float*", "void*"] + ["int"] * 5 + ["int64_t"] * 5 + \
        ["float", "int", "int*", "int*", "int", "void*"]
    assert len(L.DECLS["lrp_gated_cp_bwd_il"][1]) == len(GATED) and L.DECLS["lrp_attn_bwd_dv_ok"][1] == ["int", "int"]
    for name in ("lrp_attn_bwd_dv", "lrp_attn_bwd_dv_ok", "lrp_gated_cp_bwd_il"):
        assert getattr(L.lib, name).argtypes is not None
    served = {(dt, d) for dt in (F32, BF16) for d in (8, 16, 32, 48, 64, 96, 128, 256) if L.lib.lrp_attn_bwd_dv_ok(dt, d)}
    assert served == {(F32, 16), (F32, 32), (F32, 64), (F32, 128), (BF16, 64), (BF16, 96), (BF16, 128)}
    import lxt_amd.ops as ops
    assert ops.attn_bwd_dv_ok(torch.bfloat16, 128) and not ops.attn_bwd_dv_ok(torch.bfloat16, 256) and not ops.attn_bwd_dv_ok(torch.float16, 128)


@pytest.mark.parametrize("dtype,d", [(F32, 16), (F32, 64), (F32, 128), (BF16, 64), (BF16, 96), (BF16, 128)])
def test_attn_bwd_dv_refuses_before_launch(L, dtype, d):
    f = L.lib.lrp_attn_bwd_dv
    need_t = bool(L.lib.lrp_attn_needs_transposed(dtype, d))
    for p in ("q", "k", "G", "lse", "dv"):
        assert f(*dv_call(dtype, d, **{p: 0})) == EINVAL, p
    for p in ("q", "k", "G", "dv"):
        assert f(*dv_call(dtype, d, **{p: 8})) == EALIGN, p
    assert f(*dv_call(dtype, d, ldq=4 * d + 1)) == EALIGN and f(*dv_call(dtype, d, ldk=2 * d + 1)) == EALIGN
    assert f(*dv_call(dtype, d, ldg=4 * d + 1)) == EALIGN and f(*dv_call(dtype, d, lddv=2 * d + 1)) == EALIGN
    if need_t:
        assert f(*dv_call(dtype, d, G_t=0)) == EINVAL and f(*dv_call(dtype, d, G_t=8)) == EALIGN
        assert f(*dv_call(dtype, d, ldt=32)) == EALIGN and f(*dv_call(dtype, d, ldt=65)) == EALIGN
    assert f(*dv_call(dtype, d, row_lo=16)) == EINVAL and f(*dv_call(dtype, d, row_hi=16)) == EINVAL
    for change in (dict(scale=0.0), dict(Hq=3), dict(q_begin=-1), dict(dtype=7), dict(B=-1), dict(Hkv=0)):
        assert f(*dv_call(dtype, d, **change)) == EINVAL, change
    assert f(*dv_call(dtype, d, B=65536)) == ESHAPE
    assert f(*dv_call(dtype, d, B=0)) == OK and f(*dv_call(dtype, d, S=0)) == OK


@pytest.mark.parametrize("dtype,d", [(F32, 8), (F32, 48), (F32, 96), (F32, 256), (BF16, 16), (BF16, 32), (BF16, 256)])
def test_attn_bwd_dv_unserved_head_dims(L, dtype, d):
    assert L.lib.lrp_attn_bwd_dv(*dv_call(dtype, d)) == (EINVAL if d < 16 else ESHAPE)


def test_attn_bwd_dv_interval_table_refusal(L):
    """the interval table lives in LDS behind the two stages: 2 x (2 x 16 KiB + 256) + 16 bytes per 32 rows <= 160 KiB"""
    big = 32 * ((160 * 1024 - 2 * (2 * 16384 + 256)) // 16 + 1)
    assert L.lib.lrp_attn_bwd_dv(*dv_call(BF16, 128, S=big, ldt=big, row_lo=16, row_hi=16)) == ESHAPE


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gated_cp_bwd_il_refuses_before_launch(L, dtype):
    f, epc = L.lib.lrp_gated_cp_bwd_il, 4 if dtype == F32 else 8
    base = dict(Gm=16, gu=16, Agu=16, M=3, I=64, ldgm=64, ldgu=128, ldagu=128, act=0, dtype=dtype, stream=None)
    call = lambda **c: f(*[dict(base, **c)[n] for n in GATED])          # noqa: E731
    for p in ("Gm", "gu", "Agu"):
        assert call(**{p: 0}) == EINVAL and call(**{p: 8}) == EALIGN
    for change in (dict(I=48), dict(act=4), dict(act=-1), dict(M=-1), dict(dtype=5)):
        assert call(**change) == EINVAL, change
    assert call(ldgm=32) == ESHAPE and call(ldgu=64) == ESHAPE and call(ldagu=120) == ESHAPE
    assert call(ldgm=64 + epc // 2) == EALIGN and call(ldgu=128 + 1) == EALIGN and call(ldagu=128 + epc - 1) == EALIGN
    assert call(M=0) == OK and call(I=0, ldgm=0, ldgu=0, ldagu=0) == OK


def test_ops_wrappers_check_their_operands():
    import lxt_amd.ops as ops
    q, k, G = torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(8, 64)
    lse, dv = torch.zeros(1, 1, 8), torch.zeros(8, 64)
    with pytest.raises(TypeError):
        ops.attn_bwd_dv(q, k.bfloat16(), G, lse, dv, 1, 8, 1, 1, 64, 0.125)
    with pytest.raises(TypeError):
        ops.attn_bwd_dv(q, k, G, lse.double(), dv, 1, 8, 1, 1, 64, 0.125)
    with pytest.raises(RuntimeError):
        ops.attn_bwd_dv(q, k, G, lse, dv, 1, 8, 1, 1, 64, 0.125)              # CPU tensors: no fallback
    Gm, gu = torch.zeros(2, 64), torch.zeros(2, 128)
    with pytest.raises(TypeError):
        ops.gated_cp_bwd_il(Gm, gu.bfloat16(), gu, "silu")
    with pytest.raises(RuntimeError):
        ops.gated_cp_bwd_il(Gm, gu, gu.clone(), "silu")


def test_rule_keyword_without_a_device():
    import lxt_amd.engine as E
    from lxt_amd.engine_cp import cp_request
    from lxt_amd.engine_bert import BertLRP
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_gemma3_mm import Gemma3MMLRP
    from lxt_amd.engine_qwen import QwenLRP
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    cfg = dict(hidden=128, inter=256, n_layers=1, n_heads=4, n_kv=2, head_dim=32, vocab=64, rope_theta=1e4, rms_eps=1e-5)
    for cls in (E.LlamaLRP, QwenLRP):
        assert inspect.signature(cls.__init__).parameters["rule"].default == "attnlrp"
        for kw in (dict(rule="lrp"), dict(rule="CP"), dict(rule=None), dict(rule="cp", mode="explicit")):
            with pytest.raises(ValueError):          # checked first: before the weights, before a device is looked at
                cls(cfg, {}, dtype=torch.float32, **kw)
        with pytest.raises(ValueError):
            cls(dict(cfg, head_dim=48), {}, dtype=torch.float32, rule="cp")
    for cls in (Gemma3LRP, Gemma3MMLRP, Qwen3MoeLRP, BertLRP):
        assert "rule" not in inspect.signature(cls.__init__).parameters and "rule" not in inspect.signature(cls.from_hf).parameters
    assert cp_request("attnlrp", "explicit", heads=("out",), attn_map="sum", weights=("o",)) == "attnlrp"
    assert cp_request("cp", "efficient", heads=None, attn_map=None, weights=()) == "cp"
    for kw in (dict(mode="explicit"), dict(heads=("out",)), dict(attn_map="sum"), dict(attn_map=[(0, 1)]), dict(weights=("qkv",)),
               dict(dtype=torch.bfloat16, head_dim=256), dict(dtype=torch.float32, head_dim=96)):
        with pytest.raises(ValueError):
            cp_request("cp", **kw)

    class Stub(E.LlamaLRP):          # no device, no weights: what set_rule / explain check before they touch either
        def __init__(self):
            self.cfg, self.dtype, self.mode, self.rule, self.layers = cfg, torch.float32, "efficient", "attnlrp", ()
            self._graphs = E.GraphCache(torch.device("cpu"))

    stub = Stub()
    stub._graphs.graphs["x"] = None
    stub.set_rule("cp")
    assert stub.rule == "cp" and not stub._graphs.graphs
    with pytest.raises(ValueError):
        stub.set_rule("explicit")
    with pytest.raises(ValueError):
        stub.set_mode("explicit")
    for kw in (dict(heads=("out",)), dict(attn_map="sum"), dict(weights=("o",))):
        with pytest.raises(ValueError):
            stub.explain(torch.zeros(1, 4, dtype=torch.long), **kw)

    class Other(Stub):
        def forward(self, *a, **k):
            return None

    with pytest.raises(ValueError):          # a driver with a forward of its own (Qwen3MoeLRP) inherits set_rule and refuses "cp"
        Other().set_rule("cp")


@pytest.mark.parametrize("name", ["llama", "qwen2", "qwen3"])
def test_fixtures_equal_the_oracle_restatement(name):
    from oracle import hf_efficient as oh
    from tests.golden.hf_models import wsum
    from tests.golden.make_golden_generate import build
    from tests.golden.make_golden_span import explain
    fx, model = load(f"cp_{name}.npz"), build(name)
    assert abs(wsum(model) - float(fx["wsum"])) <= 1e-9 * float(fx["wsum"])
    model = oh.patch_instance(model.double(), "cp")
    ids, lengths, S = torch.from_numpy(fx["ids"]), fx["lengths"].tolist(), fx["ids"].shape[1]
    assert float(fx["err32"]) < 1e-5
    for b, n in enumerate(lengths):
        r = explain(model, ids[b, S - n:], [n - 1], [None], [1.0], "logit")
        assert r["target"][0] == int(fx["idx"][b]) and abs(r["logit"][0] - float(fx["logit"][b])) <= 1e-10
        assert nmax(r["R_tok"], fx["R_tok"][b, S - n:]) <= 1e-9 and nmax(r["layer_R"], fx["layer_R"][:, b]) <= 1e-9
        assert not np.any(fx["R_tok"][b, : S - n])
    for objective in ("logit", "logprob"):
        g = lambda k: fx[f"span_{objective}/{k}"]          # noqa: E731
        r = explain(model, ids[0], g("positions")[0].tolist(), [None] * 4, g("weights")[0].tolist(), objective)
        assert r["target"] == g("target")[0].tolist()
        assert nmax(r["R_tok"], g("R_tok")[0]) <= 1e-9 and nmax(r["layer_R"], g("layer_R")[:, 0]) <= 1e-9
        assert nmax(np.asarray(r["logprob"]), g("logprob")[0]) <= 1e-9
