"""CPU: the latent feature attribution read-out (lrp_colsum_dot, LlamaLRP.explain(latent=...)) -- its C ABI is declared and exported, rejects
bad calls before any launch, and the engine's request check refuses unknown names before a kernel of the model runs."""
import ctypes

import pytest
import torch


def test_colsum_dot_symbols_declared_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    assert decls["lrp_colsum_dot_ws"] == ("int64_t", ["int", "int", "int"])
    assert decls["lrp_colsum_dot"][0] == "int" and len(decls["lrp_colsum_dot"][1]) == 12
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "lrp_colsum_dot") and hasattr(raw, "lrp_colsum_dot_ws")
    assert L.lib.lrp_version() == 8


def test_colsum_dot_workspace_query():
    lib = __import__("lxt_amd._lib", fromlist=["lib"]).lib
    # fp32 partials of 64-row chunks of each prompt: B * ceil(S / 64) * N * 4 bytes; one chunk per prompt needs none
    assert lib.lrp_colsum_dot_ws(4, 2048, 14336) == 4 * 32 * 14336 * 4
    assert lib.lrp_colsum_dot_ws(5, 65, 7) == 5 * 2 * 7 * 4
    assert lib.lrp_colsum_dot_ws(4, 64, 4096) == 0 and lib.lrp_colsum_dot_ws(1, 1, 3) == 0
    assert lib.lrp_colsum_dot_ws(0, 64, 8) == -3 and lib.lrp_colsum_dot_ws(1, 0, 8) == -3 and lib.lrp_colsum_dot_ws(1, 8, 0) == -3


def test_colsum_dot_argument_validation_without_gpu():
    import lxt_amd._lib as L
    lib, BF16, F32 = L.lib, L.BF16, L.F32
    A = 1 << 12                                   # an aligned fake device address: every call below is rejected before a launch
    # (x, g, out, ws, M, N, B, S, ldx, ldg, dtype, stream)
    assert lib.lrp_colsum_dot(None, A, A, A, 256, 64, 2, 128, 64, 64, BF16, None) == -1          # null operand
    assert lib.lrp_colsum_dot(A, None, A, A, 256, 64, 2, 128, 64, 64, BF16, None) == -1
    assert lib.lrp_colsum_dot(A, A, None, A, 256, 64, 2, 128, 64, 64, BF16, None) == -1          # null output
    assert lib.lrp_colsum_dot(A, A, A, None, 256, 64, 2, 128, 64, 64, BF16, None) == -1          # null workspace where one is needed
    assert lib.lrp_colsum_dot(A, A, A, A, 256, 64, 2, 128, 64, 64, 7, None) == -1                # unknown dtype
    assert lib.lrp_colsum_dot(A, A, A, A, 255, 64, 2, 128, 64, 64, BF16, None) == -3             # S B != rows
    assert lib.lrp_colsum_dot(A, A, A, A, 0, 64, 0, 128, 64, 64, BF16, None) == -3               # B < 1
    assert lib.lrp_colsum_dot(A, A, A, A, 256, 0, 2, 128, 64, 64, BF16, None) == -3              # N < 1
    assert lib.lrp_colsum_dot(A, A, A, A, 256, 64, 2, 128, 56, 64, BF16, None) == -3             # pitch below the row width
    assert lib.lrp_colsum_dot(A + 2, A, A, A, 256, 64, 2, 128, 64, 64, BF16, None) == -2         # operand off the 16-byte grid
    assert lib.lrp_colsum_dot(A, A + 8, A, A, 256, 64, 2, 128, 64, 64, BF16, None) == -2
    assert lib.lrp_colsum_dot(A, A, A, A, 256, 60, 2, 128, 60, 64, BF16, None) == -2             # bf16 pitch not a multiple of 8
    assert lib.lrp_colsum_dot(A, A, A, A, 256, 62, 2, 128, 64, 66, F32, None) == -2              # fp32 pitch not a multiple of 4
    assert lib.lrp_colsum_dot(A, A, A + 2, A, 256, 64, 2, 128, 64, 64, F32, None) == -2          # output not 4-byte aligned
    # one chunk per prompt (S <= 64): no workspace needed, so a NULL one is no error -- the call then gets as far as the alignment check
    assert lib.lrp_colsum_dot(A, A, A, None, 128, 64, 2, 64, 60, 64, F32, None) == -3
    assert lib.lrp_colsum_dot(A + 4, A, A, None, 128, 64, 2, 64, 64, 64, F32, None) == -2


def test_colsum_dot_binding_rejects_cpu_tensors():
    from lxt_amd import ops
    x = torch.randn(8, 16)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.colsum_dot(x, x, 2, 4)
    with pytest.raises(ValueError):
        ops.colsum_dot(x, torch.randn(8, 8), 2, 4)


def test_latent_request_names():
    from lxt_amd.engine import latent_request, LATENT
    bf, f4 = torch.bfloat16, torch.float32
    assert latent_request(None, 4096, 14336, bf) == frozenset()
    assert latent_request([], 4096, 14336, bf) == frozenset()
    assert latent_request(("trace", "resid", "mlp"), 4096, 14336, bf) == frozenset(LATENT)
    assert latent_request("mlp", 4096, 14336, bf) == frozenset({"mlp"})           # one name as a string, not its letters
    assert latent_request({"trace", "trace"}, 4096, 14336, bf) == frozenset({"trace"})
    for bad in (["neurons"], ("trace", "R_mlp"), "heads", 3):
        with pytest.raises(ValueError):
            latent_request(bad, 4096, 14336, bf)
    # the column read-out reads rows of a multiple of 16 bytes: H for "resid", I for "mlp" ("trace" reads no columns)
    with pytest.raises(ValueError):
        latent_request(["resid"], 4100, 14336, bf)
    with pytest.raises(ValueError):
        latent_request(["mlp"], 4096, 14338, f4)
    assert latent_request(["trace"], 4100, 14338, bf) == frozenset({"trace"})
    assert latent_request(["mlp"], 4100, 14336, bf) == frozenset({"mlp"})


def test_explain_rejects_latent_before_anything_runs():
    """LlamaLRP.explain checks latent first: a stub without weights or a device raises the ValueError, not an error of a missing kernel input"""
    from lxt_amd.engine import LlamaLRP
    stub = LlamaLRP.__new__(LlamaLRP)
    stub.cfg, stub.dtype = dict(hidden=64, inter=128, vocab=32), torch.bfloat16
    with pytest.raises(ValueError, match="unknown read-out"):
        stub.explain(torch.zeros(1, 4, dtype=torch.long), latent=["attention_heads"])
