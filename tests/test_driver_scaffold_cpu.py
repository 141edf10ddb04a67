"""CPU: the scaffolding the fused drivers share (lxt_amd.engine): the flat weight layout of LlamaLRP and Gemma3LRP, pinned at released model
dimensions against the numbers their earlier hand-written packing code produced, the explain() front end's conversions and refusals, and the
host side of the explain / generate pipeline behind both decoder drivers (read-out assembly, the map request's head dims, the KV-cache set-up)."""
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


# ---- the explain / generate pipeline the decoder drivers share

class _Sink:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("span", [False, True])
def test_readout_outputs_assembly(span):
    """B = 2, S = 3, L = 2 on integer-valued fp32 (every sum is exact): R_trace[l] sums to layer_R[l], index 0 is R_tok, and the head's
    boundary is non-zero at the last column only -- with a span at the span's columns only"""
    B, S, L = 2, 3, 2
    R_tok = torch.tensor([[1.0, -2.0, 4.0], [8.0, 16.0, -32.0]])
    mid = torch.tensor([3.0, 5.0, -7.0, 11.0, 13.0, 17.0])                    # the input of layer 1, per token [B S]
    if span:
        rows, rel_last = torch.tensor([0, 2, 4, 3]), torch.tensor([19.0, 23.0, -29.0, 31.0])      # slot order: prompt 0 -> columns 0, 2; prompt 1 -> 1, 0
        head = torch.tensor([[19.0, 0.0, 23.0], [31.0, -29.0, 0.0]])
    else:
        rows, rel_last = None, torch.tensor([19.0, 23.0])
        head = torch.tensor([[0.0, 0.0, 19.0], [0.0, 0.0, 23.0]])
    layer_R = [rel_last, mid, R_tok.reshape(-1).clone()]                       # from the top boundary down to the embedding
    lat = dict(R_resid=torch.ones(L + 1, B, 4))
    hs = _Sink(out=dict(out=torch.arange(24.0).view(L, B, 2, S), k=torch.ones(L, B, 2, S)))
    am = _Sink(total=torch.ones(L, B, S, S), per_head=torch.zeros(1, B, S, S), pairs=((1, 0),))
    cpu = torch.device("cpu")

    out = E.readout_outputs(dict(R_tok=R_tok), B, S, layer_R, lat, True, True, hs, am, cpu, rows)
    tr = out["R_trace"]
    assert tr.shape == (L + 1, B, S) and out["layer_R"].shape == (L + 1, B)
    for l in range(L + 1):
        assert torch.equal(tr[l].sum(-1), out["layer_R"][l]), l
    assert torch.equal(tr[0], R_tok) and torch.equal(tr[1], mid.view(B, S)) and torch.equal(tr[L], head)
    assert out["R_resid"] is lat["R_resid"]
    assert set(out) == {"R_tok", "layer_R", "R_trace", "R_resid", "R_head_out", "R_head_k", "R_head", "R_attn", "R_attn_heads", "attn_map_heads"}
    assert torch.equal(out["R_head"], hs.out["out"].sum(-1)) and out["attn_map_heads"] == [(1, 0)]
    assert out["R_attn"] is am.total and out["R_attn_heads"] is am.per_head

    # each key appears exactly when its sink has it; nothing asked for: the dict comes back as it went in
    only = E.readout_outputs(dict(R_tok=R_tok), B, S, layer_R, {}, True, False, _Sink(out=dict(q=hs.out["k"])), _Sink(total=None, per_head=None, pairs=()),
                             cpu, rows)
    assert set(only) == {"R_tok", "layer_R", "R_head_q"} and torch.equal(only["layer_R"], out["layer_R"])
    only = E.readout_outputs(dict(R_tok=R_tok), B, S, layer_R, {}, False, True, None, _Sink(total=am.total, per_head=None, pairs=()), cpu, rows)
    assert set(only) == {"R_tok", "R_trace", "R_attn"} and torch.equal(only["R_trace"], tr)
    assert set(E.readout_outputs(dict(R_tok=R_tok), B, S, None, {}, False, False, None, None, cpu, rows)) == {"R_tok"}


def test_attn_map_request_head_dims_of_the_callers_kernel():
    req = lambda d, dt=BF16, **kw: E.attn_map_request("sum", 2, 4, d, dt, "efficient", **kw)      # noqa: E731
    old = r"attn_map: no kernel for head dim 256 in torch\.bfloat16 \(bf16: 64 or 128; fp32: a multiple of 4 up to 256\)"
    with pytest.raises(ValueError, match=old):
        req(256)
    assert req(256, bf16_dims=(64, 128, 256)) == (True, ()) and req(64) == req(128) == (True, ())
    assert G.gemma_attn_map_request("sum", 2, 4, 256, BF16) == (True, ())
    for kw in ({}, dict(bf16_dims=(64, 128, 256))):
        for d in (96, 32, 512, None):
            with pytest.raises(ValueError, match="no kernel for head dim"):
                req(d, **kw)
        assert req(96, torch.float32, **kw) == (True, ())          # (fp32 does not look at bf16_dims)
        with pytest.raises(ValueError, match="no kernel"):
            req(260, torch.float32, **kw)
        with pytest.raises(ValueError, match="efficient placement"):
            E.attn_map_request("sum", 2, 4, 128, BF16, "explicit", **kw)
    with pytest.raises(ValueError, match="no kernel"):
        G.gemma_attn_map_request("sum", 2, 4, 96, BF16)


class _StubDriver:
    """what generate_cached reads of a driver, on the CPU: a forward that leaves known K / V rows, a recording decode step and graph cache"""

    def __init__(self, L, nq, nk, d, H, V):
        self.cfg, self.max_seq, self.dtype, self.device = dict(vocab=V, n_heads=nq, n_kv=nk, head_dim=d), 64, torch.float32, torch.device("cpu")
        self.layers, self._arena, self.H, self.steps, self.keys = [None] * L, E.Arena(self.device, self.dtype), H, [], []

    def embed(self, ids):
        return ids.to(self.dtype)[:, None].expand(-1, self.H) * 0.5

    def forward(self, emb, B, S, row_iv):
        c = self.cfg
        self.fwd = (emb, B, S, row_iv)
        mk = lambda li, w: torch.arange(B * S * w, dtype=self.dtype).view(B * S, w) + 1000 * li      # noqa: E731
        stash = [dict(k=mk(li, c["n_kv"] * c["head_dim"]), v=-mk(li, c["n_kv"] * c["head_dim"])) for li in range(len(self.layers))]
        return dict(stash=stash, logits=torch.zeros(B, c["vocab"]))

    def _decode_step(self, tok, pos, lo, kc, vc, ws):
        self.steps.append((tok, pos, lo, kc, vc, ws))
        return "logits", "idx"

    def _graphs(self, key, run, *inputs):
        self.keys.append(key)
        return run(*inputs)


@pytest.mark.parametrize("graph", [False, True])
def test_generate_cached_cache_shapes_and_step_inputs(monkeypatch, graph):
    """no device: the token loop is replaced by a recorder, the decode step and the graph cache are the stub's"""
    L, nq, nk, d, H, V, B, S, T = 3, 4, 2, 8, 16, 32, 2, 5, 3
    drv = _StubDriver(L, nq, nk, d, H, V)
    monkeypatch.setattr(E, "greedy_decode", lambda *a, **kw: (a, kw))
    ids, lens = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(0)), [5, 2]
    args = dict(input_ids=ids, max_new_tokens=T, lengths=lens, eos_token_id=7, pad_token_id=None, graph=graph, return_logits=True, inputs_embeds=None,
                force_tokens=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=None)
    run = lambda d_, **kw: E.generate_cached(d_, drv.embed, lambda st: (st["k"], st["v"]), lambda b, cap: ("decode", b, cap, "tail"),      # noqa: E731
                                             **dict(args, **kw))
    (logits, step, cols, ids_d, lens_h, n_new, eos, pad, forced, want_logits), kw = run(drv)
    emb, fB, fS, row_iv = drv.fwd
    assert (fB, fS) == (B, S) and torch.equal(emb, drv.embed(ids.reshape(-1))) and row_iv[0][:, 0].tolist() == [0, 3]
    assert torch.equal(ids_d, ids) and lens_h.tolist() == lens and (n_new, eos, pad, forced, want_logits) == (T, [7], 7, None, True)
    assert kw == dict(sampler=None) and logits.shape == (B, V)
    assert cols.dtype == torch.int32 and torch.equal(cols, torch.arange(S, S + T, dtype=torch.int32))
    tok, pos = torch.zeros(B, dtype=torch.long), cols[:1]
    assert step(tok, pos) == ("logits", "idx") and len(drv.steps) == 1
    s_tok, s_pos, lo, kc, vc, ws = drv.steps[0]
    assert s_tok is tok and s_pos is pos and drv.keys == ([("decode", B, S + T, "tail")] if graph else [])
    assert kc.shape == vc.shape == (L, B, S + T, nk * d) and kc.dtype == drv.dtype
    assert lo.dtype == torch.int32 and lo.tolist() == [S - n for n in lens]
    assert ws.dtype == torch.uint8 and ws.numel() == E.ops.attn_decode_ws(B, nq, d, S + T)
    fw = drv.forward(None, B, S, None)
    for li, st in enumerate(fw["stash"]):          # the prefill's rows, layer by layer; the T new columns are the decode step's to write
        assert torch.equal(kc[li, :, :S], st["k"].view(B, S, nk * d)) and torch.equal(vc[li, :, :S], st["v"].view(B, S, nk * d))
    # every refusal comes before the driver's device, arena or weights are looked at
    bare = type("Bare", (), dict(cfg=drv.cfg, max_seq=64))()
    for bad in (dict(max_new_tokens=0), dict(max_new_tokens=60), dict(lengths=[6, 1]), dict(eos_token_id=V), dict(inputs_embeds=torch.zeros(B, S, H)),
                dict(temperature=0.5), dict(do_sample=True)):
        with pytest.raises(ValueError):
            run(bare, **bad)
