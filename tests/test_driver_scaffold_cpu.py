"""CPU: the scaffolding the fused drivers share (lxt_amd.engine): the flat weight layout of LlamaLRP and Gemma3LRP, pinned at released model
dimensions against the numbers their earlier hand-written packing code produced, and the explain() front end's conversions and refusals."""
import pytest
import torch

import lxt_amd.engine as E
import lxt_amd.engine_gemma3 as G

BF16 = torch.bfloat16


def _layout(top, layers):
    """{name: (storage offset, shape, stride)} of the model-wide views and of layer 0's"""
    d = lambda t: (t.storage_offset(), tuple(t.shape), t.stride())      # noqa: E731
    return {k: d(v) for k, v in top.items()}, {k: d(v) for k, v in layers[0].items()}


def test_llama_flat_layout_8b(monkeypatch):
    monkeypatch.setattr(E, "PITCH_PAD", True)
    cfg = dict(hidden=4096, inter=14336, n_layers=32, n_heads=32, n_kv=8, head_dim=128, vocab=128256)
    flat, top, layers = E.pack_flat(*E.LlamaLRP.flat_layout(cfg, BF16), 32, BF16, "meta")
    assert flat.numel() == 8181256192 and flat.dtype == BF16 and len(layers) == 32
    t, l0 = _layout(top, layers)
    assert t == {"embed": (0, (128256, 4096), (4096, 1)), "lm_head": (525336576, (128256, 4096), (4096, 1)), "norm": (1050673152, (4096,), (1,))}
    assert l0 == {"ln1": (1050677248, (4096,), (1,)), "ln2": (1050681344, (4096,), (1,)), "wqkv": (1050685440, (6144, 4096), (4224, 1)),
                  "wo": (1076637696, (4096, 4096), (4096, 1)), "wgu": (1093414912, (28672, 4096), (4224, 1)),
                  "wd": (1214525440, (4096, 14336), (14400, 1))}
    assert layers[31]["ln1"].storage_offset() == 7958425600 and layers[31]["wd"].storage_offset() == 8122273792


@pytest.mark.parametrize("tied", [True, False])
def test_gemma3_flat_layout_4b(monkeypatch, tied):
    monkeypatch.setattr(E, "PITCH_PAD", True)
    cfg = dict(hidden=2560, inter=10240, n_layers=34, n_heads=8, n_kv=4, head_dim=256, vocab=262208)
    flat, top, layers = E.pack_flat(*G.Gemma3LRP.flat_layout(cfg, BF16, tied), 34, BF16, "meta")
    o = 0 if tied else 671252480                                  # an untied LM head is stored after the embedding
    assert flat.numel() == 3974962688 + o and len(layers) == 34
    assert ("lm_head" in top) == (not tied)
    t, l0 = _layout(top, layers)
    assert t["embed"] == (0, (262208, 2560), (2560, 1)) and t.get("lm_head", t["embed"]) == (o, (262208, 2560), (2560, 1))
    assert t["norm"] == (671252480 + o, (2560,), (1,))
    assert l0 == {"ln_in": (671255040 + o, (2560,), (1,)), "ln_pa": (671257600 + o, (2560,), (1,)), "ln_pf": (671260160 + o, (2560,), (1,)),
                  "ln_pff": (671262720 + o, (2560,), (1,)), "qn": (671265280 + o, (256,), (1,)), "kn": (671265536 + o, (256,), (1,)),
                  "wqkv": (671265792 + o, (4096, 2560), (2560, 1)), "wo": (681751552 + o, (2560, 2048), (2048, 1)),
                  "wgu": (686994432 + o, (20480, 2560), (2688, 1)), "wd": (742044672 + o, (2560, 10240), (10304, 1))}
    assert layers[33]["ln_in"].storage_offset() == 3877794816 + o and layers[33]["wd"].storage_offset() == 3948584448 + o


def test_arena_accessors(monkeypatch):
    monkeypatch.setattr(E, "PITCH_PAD", True)
    ar = E.Arena(torch.device("cpu"), BF16)
    m = ar.wide("m", 8, 14336)                                    # a long-K operand: row pitch off the 4-KiB grid
    assert m.shape == (8, 14336) and m.stride(0) == 14400 and m.dtype == BF16
    x, x32 = ar.new("x", 3, 5), ar.f32("x", 3, 5)                 # one buffer per (tag, dtype)
    assert x.dtype == BF16 and x32.dtype == torch.float32 and x.data_ptr() != x32.data_ptr()
    x.fill_(1.0)
    z = ar.zeros("x", 3, 5)
    assert z.data_ptr() == x.data_ptr() and float(z.abs().sum()) == 0.0 and ar.gen == 0


def test_explain_front_end():
    cpu = torch.device("cpu")
    ids = torch.randint(0, 50, (3, 10))
    front = lambda **kw: E.explain_inputs(kw.pop("input_ids", ids), kw.pop("inputs_embeds", None), kw.pop("lengths", None),   # noqa: E731
                                          kw.pop("target", None), 50, 16, BF16, cpu, **kw)
    assert front() == (3, 10, None, None, None)

    # lengths: prompt b occupies the last lengths[b] columns; a row attends to the keys [S - lengths[b], i], a pad row to none
    lens = [10, 4, 1]
    B, S, emb, (lo, hi), idx = front(lengths=torch.tensor(lens))
    assert lo.dtype == hi.dtype == torch.int32 and lo.shape == hi.shape == (3, 10)
    for b, n in enumerate(lens):
        for i in range(S):
            assert (int(lo[b, i]), int(hi[b, i])) == (S - n, i + 1 if i >= S - n else 0)
    assert front(lengths=lens)[3][1].tolist() == hi.tolist()

    # target -> int32 indices; inputs_embeds -> [B S, H] in the model dtype
    _, _, _, _, idx = front(target=[0, 7, 49])
    assert idx.dtype == torch.int32 and idx.tolist() == [0, 7, 49]
    B, S, emb, _, _ = front(input_ids=None, inputs_embeds=torch.randn(3, 10, 8))
    assert (B, S) == (3, 10) and emb.shape == (30, 8) and emb.dtype == BF16

    for bad in (dict(lengths=[10, 0, 3]), dict(lengths=[11, 4, 1]), dict(target=[1, 2]), dict(target=[1, 2, 50]), dict(target=[-1, 2, 3]),
                dict(target=[1, 2, 3], seed=torch.zeros(3, 50)), dict(seed=torch.zeros(3, 49)), dict(input_ids=torch.zeros(3, 17, dtype=torch.long))):
        with pytest.raises(ValueError):
            front(**bad)
