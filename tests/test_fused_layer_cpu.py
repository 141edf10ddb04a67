"""CPU: the fused dense Llama layer (lxt_amd.engine.fused_layer_ok / fused_layer_fwd / fused_layer_bwd, shared by LlamaLRP and the drop-in's
DecoderLayerFn) asks its eligibility questions about the row pitches its launches then get.  The predicates are host functions of the library;
the launches are recorded on meta tensors, nothing runs on a device."""
import torch

import lxt_amd.engine as E
import lxt_amd.ops as ops

# Llama-3-8B: Aqkv [M, 6144] bf16 is a 12-KiB row, on the 4-KiB grid -> +64 elements; m / Agu get pitch_pad, the large weights weight_pitch_pad
H, I, NQ, NK, D, M = 4096, 14336, 32, 8, 128, 8192
NQKV = (NQ + 2 * NK) * D


def _weights(pt):
    pitched = lambda rows, cols, pitch: torch.empty(rows, pitch, device="meta", dtype=torch.bfloat16)[:, :cols]     # noqa: E731
    return dict(wqkv=pitched(NQKV, H, pt["Wqkv"]), wo=pitched(H, NQ * D, NQ * D), wgu=pitched(2 * I, H, pt["Wgu"]), wd=pitched(H, I, pt["Wd"]))


def test_fused_layer_eligibility_asks_about_the_launched_pitches(monkeypatch):
    pt = E.fused_layout(H, I, NQ, NK, D, torch.bfloat16)
    assert pt["Aqkv"] == NQKV + 64 and pt["Agu"] > 2 * I and pt["m"] > I           # (the padded case: the drop-in once asked at nqkv / 2 I)
    W, meta = _weights(pt), (NQ, NK, D, 1e-5, "silu", D ** -0.5)
    asked = {}
    monkeypatch.setattr(ops, "norm_fused_ok", lambda M_, N, K, lda, ldb, nn, dt: asked.setdefault((N, K, nn), (lda, ldb)) is not None)
    monkeypatch.setattr(ops, "gated_coef_ok", lambda *a: asked.setdefault("coef", a) is not None)
    ok = E.fused_layer_ok(M, W, meta, torch.bfloat16, {})
    assert ok.coef and ok.norm and ok.prep and ok.full == (D in (64, 128) and ops.attn_dq_d_ok(torch.bfloat16, D))
    assert asked["coef"] == (M, I, H, H, pt["Wgu"], H, pt["Wd"], "silu", torch.bfloat16)

    # what the launches get: the forward / backward on recording stubs, buffers from a meta-device allocator
    got = {}

    def stub(name, ret):
        def f(*a, **kw):
            got.setdefault(name, []).append(a)
            return ret(*a)
        monkeypatch.setattr(ops, name, f)

    stub("attn_fwd", lambda *a: None)
    stub("gemm_res_ssq", lambda x, W_, res, out, *r: out)
    stub("rms_rstd", lambda ssq, M_, H_, eps, rstd: rstd)
    stub("gemm_gated_fwd_coef", lambda x, W_, coef, m, *r: (coef, m))
    stub("gemm_gated_bwd_coef", lambda A, W_, coef, Agu: Agu)
    stub("gemm_nn_rs_res", lambda s, W_, rs, res, out: out)
    stub("gemm_nn_rs", lambda s, W_, rs, out: out)
    for name in ("attn_bwd_dq_d", "attn_bwd_dkv", "gqa_reduce_rope", "gqa_reduce"):
        stub(name, lambda *a: None)
    alloc = lambda tag, rows, cols, pad, dt: torch.empty(rows, cols + pad, device="meta", dtype=dt)[:, :cols]     # noqa: E731
    new = lambda cols: torch.empty(M, cols, device="meta", dtype=torch.bfloat16)                                  # noqa: E731
    vec = torch.empty(M, device="meta", dtype=torch.float32)
    cos = torch.empty(2048, D, device="meta", dtype=torch.float32)
    st = E.fused_layer_fwd(new(H), vec, new(NQKV), new((NQ + NK) * D), W, cos, cos, M // 2048, 2048, meta, alloc)
    st.update(rstd1=vec, qkv=new(NQKV), qkr=new((NQ + NK) * D))
    E.fused_layer_bwd(new(H), st, W, cos, cos, M // 2048, 2048, meta, alloc)

    m = got["gemm_res_ssq"][1][0]                                     # h' = h1 + m Wd^T
    Agu, Aqkv = got["gemm_nn_rs_res"][0][0], got["gemm_nn_rs_res"][1][0]
    assert asked[(H, I, False)] == (m.stride(0), W["wd"].stride(0)) == (pt["m"], pt["Wd"])
    assert asked[(H, 2 * I, True)] == (Agu.stride(0), W["wgu"].stride(0)) == (pt["Agu"], pt["Wgu"])
    assert asked[(H, NQKV, True)] == (Aqkv.stride(0), W["wqkv"].stride(0)) == (pt["Aqkv"], pt["Wqkv"])
    assert asked[(NQ * D, H, True)] == (got["gemm_nn_rs"][0][0].stride(0), NQ * D)     # Gho = 1/2 (Aa Wo)
    assert got["attn_bwd_dq_d"][0][7].stride(0) == pt["Aqkv"]        # the dQ kernel stores into the same Aqkv
