"""No GPU: the element-wise bounds of tests/gemm_bound.py for the dense GEMM family.
  (a) soundness: a torch model of the kernels' arithmetic (fp32 maths in the kernels' K-tile / split / slab order, a round trip through bf16
      exactly where they store) is within every bound on every element of every case; the exact zeros and the cap on the share of cg / cu left out
      are asserted;
  (b) discrimination: each planted structural fault leaves the bound on every output it touches; next to it, whether the bars
      tests/test_kernels_gpu.py holds these kernels to (nmax, block maximum) would have let it through -- at least one fault planted on a block
      whose entries are 2^-6 of the output's maximum does pass them (asserted: the reason these tests exist);
  (c) the signed-bias statistic separates truncating stores from round-to-nearest;
  (d) the shapes of tests/test_gemm_bound_gpu.py reach what they claim: the host rules of csrc/gemm.hip, mirrored in gemm_bound and held
      against the library's own exported answers (no device is touched)."""
import pytest
import torch

from tests import gemm_bound as gb

BF16, F32 = torch.bfloat16, torch.float32
CUS = 4          # compute units of the model's persistent walk: a 3 x 3-tile problem then gives workgroup 0 the tiles 0, 4, 8


def _case(name):
    """the CPU cases: small shapes with the same structure as the device's (ragged tiles, several K tiles, K splits, row chunks of 256)"""
    blk = (16, 32)
    tab = gb.rope_tables(512)
    mk = gb.operands
    if name.startswith("nt-reg"):
        return "nt", mk(300, 280, 200, dtype=F32 if name.endswith("fp32") else BF16, seed=1, block=blk, with_bias=True)
    if name.startswith("nt-glds"):
        return "nt", mk(130, 70, 256, dtype=F32 if name.endswith("fp32") else BF16, seed=2, block=blk)
    if name == "nt-f32out":
        return "nt", mk(130, 70, 128, seed=3, block=blk, odt=F32, with_bias=True)
    if name == "nt-batched":
        return "nt", mk(70, 50, 96, seed=4, batch=3)
    if name in ("nt-walk", "nn-walk"):
        return name[:2], mk(600, 700, 192, nn=name[:2] == "nn", seed=5, block=(272, 300), cus=CUS)
    if name.startswith("skinny"):
        _, shape, nn, odt = name.split("-")
        N, K, plan = {"s11": (1022, 1408, (11, 2)), "k2560": (4090, 2560, (10, 4)), "one": (1001, 128, (1, 2))}[shape]
        return "skinny", mk(17, N, K, nn=nn == "nn", seed=6, plan=plan, odt=F32 if odt == "fp32" else BF16, with_bias=nn == "nn")
    if name in ("nt_rs", "nt_rs_bias"):
        return name, mk(512, 256, 128, seed=7, block=blk, chunk=256)
    if name in ("nn_rs", "nn_rs_res"):
        return name, mk(512, 256, 128, nn=True, seed=8, block=blk, chunk=256)
    if name == "res_ssq":
        return name, mk(300, 256, 192, seed=9, block=blk)
    if name in ("rope-192", "rope-512", "bias_rope"):
        seq = 512 if name == "rope-512" else 192
        return ("bias_rope" if name == "bias_rope" else "rope"), mk(512, 512, 128, seed=10, block=blk, chunk=256, seq=seq, rope_cols=256, cos=tab[0], sin=tab[1])
    if name.startswith("gated_fwd"):
        _, act, stab, rs = name.split("-")
        eps_g, eps_lin = gb.STABS[int(stab)]
        return "gated_fwd", mk(300, 256, 128, seed=11, block=blk, act=act, eps_g=eps_g, eps_lin=eps_lin, with_rs=rs == "rs")
    if name == "gated_bwd":
        d = mk(300, 128, 192, nn=True, seed=12, block=blk)
        gen = torch.Generator().manual_seed(12)
        d["coef"] = (0.5 * torch.randn(300, 256, generator=gen)).to(BF16)
        return name, d
    if name.startswith("smallm_fwd"):
        dt = F32 if name.endswith("fp32") else BF16
        return "smallm_fwd", mk(5, *gb.SMALLM_SHAPE, dtype=dt, seed=13, with_res=False, with_bias="bias" in name)
    if name.startswith("smallm_dgrad"):
        _, kind, dts = name.split("-")
        kw = {"plain": {}, "ratio": dict(eps=1e-6), "rel": dict(eps=1e-6, rel_in=True, rel_out=True)}[kind]
        return "smallm_dgrad", mk(5, gb.SMALLM_SHAPE[1], gb.SMALLM_SHAPE[0], nn=True, dtype=F32 if dts == "fp32" else BF16, seed=14, with_z=True, **kw)
    if name == "stream_fwd":
        return "skinny", mk(17, 256, 2048, seed=15, with_res=False, chain=512, adds=4, with_bias=True)
    if name.startswith("stream_dgrad-"):
        return "stream_dgrad", mk(17, 256, 2048, nn=True, seed=17, with_res=False, with_z=True, chain=128, adds=3 + 4, group=4, eps=1e-6,
                                  rel_in=name.endswith("rel"), odt=F32 if "fp32" in name else BF16)
    if name == "stream_dgrad":
        return "skinny", mk(17, 256, 2048, nn=True, seed=16, with_res=False, chain=128, adds=3 + 4, group=4)
    raise KeyError(name)


CASES = (["nt-reg-bf16", "nt-reg-fp32", "nt-glds-bf16", "nt-glds-fp32", "nt-f32out", "nt-batched", "nt-walk", "nn-walk"]
         + [f"skinny-{s}-{nn}-{o}" for s in ("s11", "k2560", "one") for nn in ("nt", "nn") for o in ("bf16", "fp32")]
         + ["nt_rs", "nt_rs_bias", "nn_rs", "nn_rs_res", "res_ssq", "rope-192", "rope-512", "bias_rope", "gated_bwd"]
         + [f"gated_fwd-{a}-{s}-{r}" for a in ("silu", "gelu_tanh") for s in (0, 1) for r in ("rs", "plain")]
         + ["smallm_fwd-bf16", "smallm_fwd-bias-bf16", "smallm_fwd-bias-fp32"] + [f"smallm_dgrad-{k}-{t}" for k in ("plain", "ratio", "rel") for t in ("bf16", "fp32")]
         + ["stream_fwd", "stream_dgrad", "stream_dgrad-z", "stream_dgrad-z-rel", "stream_dgrad-z-out-fp32"])
# where each fault is planted
PLANTS = {"drop_kstep": ("nt-reg-bf16", "nt-reg-fp32", "nt-glds-bf16", "nt-walk", "nn-walk"), "stale_first_ktile": ("nt-walk", "nn-walk"),
          "drop_seam": ("skinny-s11-nt-bf16", "skinny-s11-nn-fp32"), "dup_seam": ("skinny-s11-nt-bf16", "skinny-s11-nn-fp32"),
          "short_last": ("skinny-k2560-nt-bf16", "skinny-k2560-nn-fp32"), "sk_dead_rows": ("skinny-s11-nt-bf16", "skinny-s11-nn-bf16"),
          "reduce_tail": ("skinny-s11-nt-bf16", "skinny-s11-nt-fp32"), "rs_neighbour": ("nt_rs", "nn_rs_res", "rope-192"),
          "rs_chunk_local": ("nt_rs", "nn_rs_res"), "rope_chunk": ("rope-512",), "rope_pos_off1": ("rope-192",), "rope_sign": ("rope-192",),
          "bias_after_rot": ("bias_rope",), "double_round": ("res_ssq", "nn_rs_res"), "ssq_unrounded": ("res_ssq",),
          "cu_for_cg": ("gated_fwd-silu-0-plain", "gated_fwd-gelu_tanh-1-rs", "gated_bwd"), "swap_gu_block": ("gated_fwd-silu-0-plain", "gated_fwd-silu-1-rs")}
ON_SMALL_BLOCK = ("drop_kstep", "rs_neighbour")          # planted on the 2^-6-scaled rows alone


def _with_stored(form, d, out):
    if form == "res_ssq":
        d = dict(d, stored=out["out"])
    return d


@pytest.mark.parametrize("name", CASES)
def test_model_is_within_every_bound(name):
    form, d = _case(name)
    print(f"[{name}] the model against its bounds")
    for rnd in (gb.rne, gb.trunc):          # truncation is one rounding of at most 2 u: not sound for a bound of u (the bias statistic tells it)
        out = gb.model(form, d, rnd=rnd)
        if rnd is gb.trunc:
            if d["odt"] == F32 and form != "stream_dgrad":              # nothing is rounded to bf16: the two models agree bit for bit
                assert all(torch.equal(out[n], gb.model(form, d)[n]) for n in out)
            continue
        log = gb.evaluate(form, _with_stored(form, d, out), out)
        print(f"model {name}: worst err / bound per output: " + " ".join(f"{n} {r:.3f}" for n, r in log.items()))
        assert set(log) == set(out)
    for n, share in gb.excluded(form, d).items():
        assert share <= gb.EXCLUDED_CAP, (n, share)


def test_planted_faults_leave_the_bound():
    assert set(PLANTS) == set(gb.STRUCTURAL)
    passed_today = []
    print("fault @ case: err / bound per touched output | today's bars (nmax, worst block / max|ref|)")
    for fault, names in PLANTS.items():
        forms, touched = gb.FAULTS[fault]
        for name in names:
            form, d = _case(name)
            assert form in forms, (fault, name)
            out = gb.model(form, d, fault=fault)
            R = gb.references(form, _with_stored(form, d, gb.model(form, d)))
            hit = [n for n in touched if n in out]
            assert hit, (fault, name)
            ratios = {n: gb.evaluate(form, _with_stored(form, d, gb.model(form, d)), out, strict=False, only=(n,))[n] for n in hit}
            bars = {n: gb.todays_bars(out[n], R[n][0], form, d["odt"]) for n in hit if n != "ssq"}
            through = bool(bars) and all(b[0] for b in bars.values())
            print(f"  {fault:18s} @ {name:24s} " + " ".join(f"{n} {r:.3g}" for n, r in ratios.items()) + " | "
                  + " ".join(f"{n} {b[1]:.2e} {b[2]:.2e}" for n, b in bars.items()) + f" | today's bars: {'PASS (missed)' if through else 'caught'}")
            for n, r in ratios.items():
                assert r > 1.0, (fault, name, n, r)
            clean = gb.model(form, d)
            for n in hit:
                if n != "ssq":
                    assert gb.todays_bars(clean[n], R[n][0], form, d["odt"])[0], (name, n)
            if through and fault in ON_SMALL_BLOCK:
                passed_today.append((fault, name))
    assert passed_today, "no structural fault on a 2^-6-scaled block passes today's bars: the premise of these tests is gone"


def test_planted_block_is_small():
    """the rows the faults of ON_SMALL_BLOCK sit on: their outputs are about 2^-6 of the output's maximum"""
    for name in ("nt-reg-bf16", "nt-walk", "nt_rs"):
        form, d = _case(name)
        ref = gb.references(form, dict(d, with_bias=False))["out"][0]
        r0, c0 = d["block"]
        share = float(ref[r0:r0 + 16, c0:c0 + 16].abs().max() / ref.abs().max())
        assert 2.0 ** -9 < share < 2.0 ** -5, (name, share)
    # the walk case: workgroup 0's second tile is a full one, its first tile another
    turn, wg0 = gb.walk(3, 3, CUS)
    assert len(wg0) == 3 and len(set(wg0)) == 3 and sorted(turn.flatten().tolist()) == [0, 0, 0, 0, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("name", [n for n in CASES if not n.endswith("fp32") and n not in ("nt-f32out",)] + ["stream_dgrad-z-out-fp32"])
def test_bias_tells_truncation(name):
    form, d = _case(name)
    if not gb.bias_case(form, d):
        assert name == "stream_dgrad-z-rel"          # (the one form the statistic is not admitted on: gemm_bound.bias_case)
        return
    good, bad = gb.model(form, d), gb.model(form, d, rnd=gb.trunc)
    R = gb.references(form, d)
    for n in good:
        if n == "ssq":
            continue
        b_rne, b_trunc = gb.signed_bias(good[n], R[n][0]), gb.signed_bias(bad[n], R[n][0])
        print(f"  {name} {n}: bias rne {b_rne:+.3f} u, trunc {b_trunc:+.3f} u")
        assert b_trunc < -0.25 and abs(b_rne) <= 0.5 * abs(b_trunc), (name, n, b_rne, b_trunc)


def test_shapes_reach_what_they_claim():
    """the shape table of the GPU test at 256 compute units: the tile-size choice of launch_fast, lrp_gemm_skinny's split plan, the *_ok gates,
    pp_row_chunk -- the mirrors in gemm_bound, and the library's own answer where it exports one"""
    import lxt_amd._lib as L
    lib, cus = L.lib, 256
    for M, N, K, batch, f_bf16, f_fp32 in gb.NT_CASES:
        assert gb.nt_form(M, N, K, BF16, K + 64, K + 64, batch or 1) == f_bf16 and gb.nt_form(M, N, K, F32, K + 64, K + 64, batch or 1) == f_fp32
    assert gb.pp_row_chunk(2 ** 21) == 256 and gb.pp_row_chunk(640) == (2 ** 30 - 1) // 640 // 256 * 256 and gb.pp_row_chunk(2 ** 23) == 0
    for name, (M, N) in gb.pp_shapes(cus).items():
        tiles = gb.cdiv(M, 256) * gb.cdiv(N, 256)
        assert (190 <= tiles <= cus) if name == "one_round" else (cus < tiles < 2 * cus and M % 256 and N % 256), (name, tiles)
        for K in gb.PP_K:
            assert gb.nt_form(M, N, K, BF16, K + 8, K + 8) == "pp" and gb.pp_ok(M, N, K, K + 8, N + 8, 1) and M <= gb.pp_row_chunk(K + 8)
        turn, _ = gb.walk(gb.cdiv(M, 256), gb.cdiv(N, 256), cus)
        assert int(turn.max()) == (0 if name == "one_round" else 1) and int((turn == 0).sum()) == min(tiles, cus)
    assert [K // 64 for K in gb.PP_K] == [2, 3, 4, 5, 9]
    for name, (N, K, plan) in gb.SKINNY_SHAPES.items():
        assert N % 4 and gb.skinny_plan(256, N, K) == plan
        for M in gb.SKINNY_M:
            assert gb.skinny_splits(M, N, K) == lib.lrp_gemm_skinny_splits(M, N, K) and gb.skinny_plan(M, N, K) == plan
            assert gb.pp_ok(M, N, K, K + 8, K + 8, 0) and gb.pp_ok(M, N, K, K + 8, N + 10, 1)
    assert gb.skinny_plan(17, 4090, 2560, adjust=False) == (14, 3)          # 40 K tiles in splits of 3: the last one would hold 1
    assert gb.SKINNY_SHAPES["splits11"][2][0] == 8 + 2 + 1                   # the reduce kernel's 8-, 2- and 1-slab loops all run
    assert [M <= 240 for M in gb.SKINNY_M] == [True] * 5 + [False] * 2       # the SK instantiation and the plain one
    for name, s in gb.fused_shapes(cus).items():
        tiles = gb.cdiv(s["M"], 256) * (s["N"] // 256)
        assert (190 <= tiles <= cus) if name == "le" else tiles > cus, (name, tiles)
        assert s["M"] % 256 and s["rope_cols"] < s["N"] and any((p * s["seq"]) % 256 for p in range(1, s["Mr"] // s["seq"]))
        for K in gb.FUSED_K:
            M, Mr, N = s["M"], s["Mr"], s["N"]
            for nn, ldb in ((0, K + 8), (1, N + 8)):
                assert gb.norm_fused_ok(M, N, K, K + 8, ldb, nn) and lib.lrp_gemm_norm_fused_ok(M, N, K, K + 8, ldb, nn, L.BF16) == 1
            for wb, fn in ((False, lib.lrp_gemm_nt_rs_rope_ok), (True, lib.lrp_gemm_nt_rs_bias_rope_ok)):
                assert gb.rope_ok(Mr, N, K, K + 8, K + 8, N + 8, s["seq"], s["rope_cols"], wb)
                assert fn(Mr, N, K, K + 8, K + 8, N + 8, s["seq"], s["rope_cols"], 128, L.BF16) == 1
            assert gb.gated_fused_ok(M, N, K, N // 2, K + 8, K + 8, 0)
    for name, (M, I) in gb.gated_bwd_shapes(cus).items():
        tiles = gb.cdiv(M, 256) * (I // 256)
        assert (190 <= tiles <= cus) if name == "pair" else tiles > cus
        for K in gb.FUSED_K:
            assert gb.gated_fused_ok(M, I, K, I, K + 8, I + 8, 1) and gb.gated_fused_ok(M, 2 * I, K, I, K + 8, K + 8, 0)
            assert lib.lrp_gemm_gated_coef_ok(M, I, K, K + 8, K + 8, K + 8, I + 8, 0, L.BF16) == 1
    assert not gb.norm_fused_ok(2100, 5376, 128, 136, 136, 0)               # one tile column fewer than `le`: 189 tiles, refused
    # the streaming Linears: the smallest shapes their gates admit, with and without contraction splits
    for name, (N, K, splits) in gb.STREAM_FWD.items():
        for M in gb.STREAM_M:
            assert lib.lrp_linear_stream_ok(M, N, K, K + 8, K + 8) == 1 and lib.lrp_linear_stream_fwd_splits(M, N, K) == splits
            assert (lib.lrp_linear_stream_fwd_tickets(M, N, K) > 0) == (splits > 1)
    assert lib.lrp_linear_stream_ok(17, 12226 - 64, 512, 520, 520) == 0 and lib.lrp_linear_stream_ok(17, 3072 - 64, 2048, 2056, 2056) == 0
    N, Kout, splits = gb.STREAM_DGRAD
    for M in gb.STREAM_M:
        assert lib.lrp_linear_stream_dgrad_ok(M, N, Kout, N + 8, Kout + 8) == (1 if M <= 32 else 0)
        assert lib.lrp_linear_stream_dgrad_ws(M, N, Kout) == splits * M * Kout * 4 and lib.lrp_linear_stream_dgrad_tickets(M, N, Kout) == Kout // 64
    assert lib.lrp_linear_stream_dgrad_ok(17, N, Kout - 64, N + 8, Kout) == 0 and N <= 2560
    from lxt_amd import ops
    assert max(gb.SMALLM_M) <= ops.SMALLM_MAX and gb.SMALLM_SHAPE[0] % 16 and gb.SMALLM_SHAPE[1] % 512 and gb.SMALLM_SHAPE[0] < 32768


def test_gemm_nt_takes_the_output_type_from_out():
    """ops.gemm_nt: a given `out` decides the output type; an out_dtype that contradicts it is refused before any pointer is handed over (CPU
    tensors: a call that got past the check would raise RuntimeError instead)"""
    from lxt_amd import ops
    a, b = torch.zeros(4, 8, dtype=BF16), torch.zeros(4, 8, dtype=BF16)
    with pytest.raises(TypeError, match="gemm_nt: out is"):
        ops.gemm_nt(a, b, out=torch.zeros(4, 4, dtype=F32), out_dtype=BF16)
    with pytest.raises(RuntimeError):          # a well-formed fp32 `out` for bf16 operands goes on to the (absent) device
        ops.gemm_nt(a, b, out=torch.zeros(4, 4, dtype=F32))


def test_bias_is_not_admitted_on_the_relevance_form():
    """gemm_bound.bias_case: one row of the fused stabiliser's relevance form, the device case's operands.  One s carries half of the row's
    absolute sum, so its single round-to-nearest error shows as a `bias` of the whole row: the statistic cannot tell truncation there"""
    N, Kout, splits = gb.STREAM_DGRAD
    d = gb.operands(1, Kout, N, nn=True, seed=13, with_res=False, with_z=True, chain=N // (4 * splits), adds=3 + splits, group=4, eps=1e-6, rel_in=True)
    sv = gb._stream_s(d)[0].abs()
    assert float(sv.max() / sv.sum()) > 0.4 and not gb.bias_case("stream_dgrad", d)
    ref = gb.references("stream_dgrad", d)["out"][0]
    b_rne, b_trunc = (gb.signed_bias(gb.model("stream_dgrad", d, rnd=r)["out"], ref) for r in (gb.rne, gb.trunc))
    print(f"bias rne {b_rne:+.3f} u, trunc {b_trunc:+.3f} u")
    assert b_rne < -0.25          # (what test_bias_tells_truncation takes as the mark of truncation, from a round-to-nearest model)
    gb.evaluate("stream_dgrad", d, gb.model("stream_dgrad", d))          # (the bound itself holds)
