"""CPU: return codes of malformed attention calls.

Every argument check of lrp_attn_fwd / lrp_attn_bwd_dq / lrp_attn_bwd_dq_d / lrp_attn_bwd_dkv returns before any HIP call, so the
library can be driven with integers as pointers (16: aligned, 8: misaligned, 0: NULL).  Each row takes a well-formed base call -- which
is never issued itself -- and changes ONE thing; it is issued for F32 and BF16 and d in {16, 32, 48, 64, 96, 128, 256}.

The expected codes below are literals RECORDED from the library of the commit before the attention host path was moved onto one call
descriptor (AttnCall), and the test passes unchanged on that commit: it pins the text and the order of the entry checks, including
their small differences between the entries (which pointers are tested, % epc against % 4 against % 8).  One character per (dtype, d):
I = LRP_EINVAL, A = LRP_EALIGN, S = LRP_ESHAPE, K = LRP_OK (early return), '.' = the row is not issued because nothing refuses it
(the change is not checked for that dtype / d and the call would launch a kernel, for which a CPU run has no device)."""
import pytest

F32, BF16 = 0, 1
DS = (16, 32, 48, 64, 96, 128, 256)
CODE = {"I": -1, "A": -2, "S": -3, "K": 0}

ARGS = {
    "lrp_attn_fwd": "q k v v_t o lse B S Hq Hkv d ldq ldk ldv ldt ldo scale causal window q_begin row_lo row_hi dtype stream",
    "lrp_attn_bwd_dq": "q k v k_t Gho lse D dq B S Hq Hkv d ldq ldk ldv ldt ldgho lddq scale eps_mask eps_qk causal window q_begin "
                       "row_lo row_hi dtype stream",
    "lrp_attn_bwd_dq_d": "q k v Gho o lse D dq B S Hq Hkv d ldq ldk ldv ldgho ldo lddq scale causal window row_lo row_hi cos_t sin_t "
                         "dtype stream",
    "lrp_attn_bwd_dkv": "q k v q_t Gho Gho_t lse D dk_h dv_h B S Hq Hkv d ldq ldk ldv ldt ldgho lddk lddv scale eps_mask eps_qk causal "
                        "window q_begin row_lo row_hi dtype stream",
}
POINTERS = ("q", "k", "v", "v_t", "k_t", "q_t", "Gho", "Gho_t", "o", "lse", "D", "dq", "dk_h", "dv_h")
PITCHES = ("ldq", "ldk", "ldv", "ldt", "ldo", "ldgho", "lddq", "lddk", "lddv")


def base_call(fn, dtype, d):
    """a well-formed call: B 2, S 40, Hq 4, Hkv 2, dense pitches, ldt = 64, causal, no row intervals, no RoPE tables"""
    a = dict(B=2, S=40, Hq=4, Hkv=2, d=d, scale=0.125, eps_mask=0.0, eps_qk=0.0, causal=1, window=0, q_begin=0, row_lo=None, row_hi=None,
             cos_t=None, sin_t=None, dtype=dtype, stream=None, ldt=64, ldk=2 * d, ldv=2 * d)
    a.update({p: 16 for p in POINTERS})
    a.update({p: 4 * d for p in PITCHES if p not in a})
    return {n: a[n] for n in ARGS[fn].split()}


def mutations(fn):
    """(label, {argument: value}) -- each changes one thing of the base call (the row-interval / table pairs: one side given)"""
    names = ARGS[fn].split()
    out = [("null " + p, {p: 0}) for p in POINTERS if p in names]
    out += [("misaligned " + p, {p: 8}) for p in POINTERS if p in names]
    out += [(p + " + 1", {p: None}) for p in PITCHES if p in names]                 # value filled from the base
    if "ldt" in names:
        out.append(("ldt < S", {"ldt": 32}))
    out += [("row_lo only", {"row_lo": 16}), ("row_hi only", {"row_hi": 16})]
    if "cos_t" in names:
        out += [("cos_t only", {"cos_t": 16}), ("sin_t only", {"sin_t": 16}), ("cos_t with d = 96", {"cos_t": 16, "sin_t": 16, "d": 96})]
    out += [("scale 0", {"scale": 0.0}), ("Hq % Hkv", {"Hq": 3}), ("B = 65536", {"B": 65536}), ("d = 8", {"d": 8}),
            ("unknown dtype", {"dtype": 7}), ("B = 0", {"B": 0})]
    return out


def issue(lib, fn, label, change, dtype, d):
    a = base_call(fn, dtype, d)
    for k, v in change.items():
        a[k] = a[k] + 1 if v is None else v
    return getattr(lib, fn)(*a.values())


# one string per changed thing: F32 d = 16, 32, 48, 64, 96, 128, 256, then BF16 likewise
EXPECT = {
    "lrp_attn_fwd": {
        "null q":              "IIIIIII IIIIIII",
        "null k":              "IIIIIII IIIIIII",
        "null v":              "..S.S.. S.SIIII",
        "null v_t":            "IIIIIII III....",
        "null o":              "IIIIIII IIIIIII",
        "null lse":            "IIIIIII IIIIIII",
        "misaligned q":        "AAAAAAA AAAAAAA",
        "misaligned k":        "AAAAAAA AAAAAAA",
        "misaligned v":        "..S.S.. S.SAAAA",
        "misaligned v_t":      "AAAAAAA AAA....",
        "misaligned o":        "AAAAAAA AAAAAAA",
        "misaligned lse":      "..S.S.. S.S....",
        "ldq + 1":             "AAAAAAA AAAAAAA",
        "ldk + 1":             "AAAAAAA AAAAAAA",
        "ldv + 1":             "..S.S.. S.SAAAA",
        "ldt + 1":             "AAAAAAA AAA....",
        "ldo + 1":             "AAAAAAA AAAAAAA",
        "ldt < S":             "AAAAAAA AAA....",
        "row_lo only":         "IIIIIII IIIIIII",
        "row_hi only":         "IIIIIII IIIIIII",
        "scale 0":             "IIIIIII IIIIIII",
        "Hq % Hkv":            "IIIIIII IIIIIII",
        "B = 65536":           "SSSSSSS SSSSSSS",
        "d = 8":               "IIIIIII IIIIIII",
        "unknown dtype":       "IIIIIII IIIIIII",
        "B = 0":               "KKKKKKK KKKKKKK",
    },
    "lrp_attn_bwd_dq": {
        "null q":              "IIIIIII IIIIIII",
        "null k":              "IIIIIII IIIIIII",
        "null v":              "IIIIIII IIIIIII",
        "null k_t":            "IIIIIII III....",
        "null Gho":            "IIIIIII IIIIIII",
        "null lse":            "IIIIIII IIIIIII",
        "null D":              "IIIIIII IIIIIII",
        "null dq":             "IIIIIII IIIIIII",
        "misaligned q":        "AAAAAAA AAAAAAA",
        "misaligned k":        "AAAAAAA AAAAAAA",
        "misaligned v":        "AAAAAAA AAAAAAA",
        "misaligned k_t":      "AAAAAAA AAA....",
        "misaligned Gho":      "AAAAAAA AAAAAAA",
        "misaligned lse":      "..S.S.. S.S....",
        "misaligned D":        "..S.S.. S.S....",
        "misaligned dq":       "AAAAAAA AAAAAAA",
        "ldq + 1":             "AAAAAAA AAAAAAA",
        "ldk + 1":             "AAAAAAA AAAAAAA",
        "ldv + 1":             "AAAAAAA AAAAAAA",
        "ldt + 1":             "AAAAAAA AAA....",
        "ldgho + 1":           "AAAAAAA AAAAAAA",
        "lddq + 1":            "AAAAAAA AAAAAAA",
        "ldt < S":             "AAAAAAA AAA....",
        "row_lo only":         "IIIIIII IIIIIII",
        "row_hi only":         "IIIIIII IIIIIII",
        "scale 0":             "IIIIIII IIIIIII",
        "Hq % Hkv":            "IIIIIII IIIIIII",
        "B = 65536":           "SSSSSSS SSSSSSS",
        "d = 8":               "IIIIIII IIIIIII",
        "unknown dtype":       "IIIIIII IIIIIII",
        "B = 0":               "KKKKKKK KKKKKKK",
    },
    "lrp_attn_bwd_dq_d": {
        "null q":              "IIIIIII IIIIIII",
        "null k":              "IIIIIII IIIIIII",
        "null v":              "IIIIIII IIIIIII",
        "null Gho":            "IIIIIII IIIIIII",
        "null o":              "IIIIIII IIIIIII",
        "null lse":            "IIIIIII IIIIIII",
        "null D":              "IIIIIII IIIIIII",
        "null dq":             "IIIIIII IIIIIII",
        "misaligned q":        "SSSSSSS SSSAAAS",
        "misaligned k":        "SSSSSSS SSSAAAS",
        "misaligned v":        "SSSSSSS SSSAAAS",
        "misaligned Gho":      "SSSSSSS SSSAAAS",
        "misaligned o":        "SSSSSSS SSSAAAS",
        "misaligned lse":      "SSSSSSS SSS...S",
        "misaligned D":        "SSSSSSS SSS...S",
        "misaligned dq":       "SSSSSSS SSSAAAS",
        "ldq + 1":             "SSSSSSS SSSAAAS",
        "ldk + 1":             "SSSSSSS SSSAAAS",
        "ldv + 1":             "SSSSSSS SSSAAAS",
        "ldo + 1":             "SSSSSSS SSSAAAS",
        "ldgho + 1":           "SSSSSSS SSSAAAS",
        "lddq + 1":            "SSSSSSS SSSAAAS",
        "row_lo only":         "IIIIIII IIIIIII",
        "row_hi only":         "IIIIIII IIIIIII",
        "cos_t only":          "IIIIIII IIIIIII",
        "sin_t only":          "IIIIIII IIIIIII",
        "cos_t with d = 96":   "SSSSSSS SSSSSSS",
        "scale 0":             "IIIIIII IIIIIII",
        "Hq % Hkv":            "IIIIIII IIIIIII",
        "B = 65536":           "SSSSSSS SSSSSSS",
        "d = 8":               "IIIIIII IIIIIII",
        "unknown dtype":       "IIIIIII IIIIIII",
        "B = 0":               "SSSSSSS SSSKKKS",
    },
    "lrp_attn_bwd_dkv": {
        "null q":              "IIIIIII IIIIIII",
        "null k":              "IIIIIII IIIIIII",
        "null v":              "IIIIIII IIIIIII",
        "null q_t":            "IIIIIII III....",
        "null Gho":            "IIIIIII IIIIIII",
        "null Gho_t":          "IIIIIII III....",
        "null lse":            "IIIIIII IIIIIII",
        "null D":              "IIIIIII IIIIIII",
        "null dk_h":           "IIIIIII IIIIIII",
        "null dv_h":           "IIIIIII IIIIIII",
        "misaligned q":        "AAAAAAA AAAAAAA",
        "misaligned k":        "AAAAAAA AAAAAAA",
        "misaligned v":        "AAAAAAA AAAAAAA",
        "misaligned q_t":      "AAAAAAA AAA....",
        "misaligned Gho":      "AAAAAAA AAAAAAA",
        "misaligned Gho_t":    "AAAAAAA AAA....",
        "misaligned lse":      "..S.S.. S.S....",
        "misaligned D":        "..S.S.. S.S....",
        "misaligned dk_h":     "AAAAAAA AAAAAAA",
        "misaligned dv_h":     "AAAAAAA AAAAAAA",
        "ldq + 1":             "AAAAAAA AAAAAAA",
        "ldk + 1":             "AAAAAAA AAAAAAA",
        "ldv + 1":             "AAAAAAA AAAAAAA",
        "ldt + 1":             "AAAAAAA AAA....",
        "ldgho + 1":           "AAAAAAA AAAAAAA",
        "lddk + 1":            "AAAAAAA AAAAAAA",
        "lddv + 1":            "AAAAAAA AAAAAAA",
        "ldt < S":             "AAAAAAA AAA....",
        "row_lo only":         "IIIIIII IIIIIII",
        "row_hi only":         "IIIIIII IIIIIII",
        "scale 0":             "IIIIIII IIIIIII",
        "Hq % Hkv":            "IIIIIII IIIIIII",
        "B = 65536":           "SSSSSSS SSSSSSS",
        "d = 8":               "IIIIIII IIIIIII",
        "unknown dtype":       "IIIIIII IIIIIII",
        "B = 0":               "KKKKKKK KKKKKKK",
    },
}

# the dK / dV kernels of attention32.hip keep a per-32-row interval table in LDS beside their tiles: with row intervals the smallest S (a
# multiple of 32) the library refuses is 63520 for d = 128 and for d = 256 (2 * (2 * 16 KiB + 512) + 64 KiB + S / 32 * 16 > 160 KiB)
DKV_LDS_REFUSED_S = {128: 63520, 256: 63520}


@pytest.mark.parametrize("fn", sorted(ARGS))
def test_attention_entry_return_codes(fn):
    import lxt_amd._lib as L
    table, wrong, issued = EXPECT[fn], [], 0
    assert [m[0] for m in mutations(fn)] == list(table), "every changed thing has its row of recorded codes, in order"
    for label, change in mutations(fn):
        codes = table[label].split()
        assert len(codes) == 2 and all(len(c) == len(DS) for c in codes), label
        for dtype in (F32, BF16):
            for d, ch in zip(DS, codes[dtype]):
                if ch == ".":
                    continue
                rc = issue(L.lib, fn, label, change, dtype, d)
                issued += 1
                if rc != CODE[ch]:
                    wrong.append((label, "BF16" if dtype else "F32", d, rc, CODE[ch]))
    assert not wrong, f"{fn}: (row, dtype, d, returned, recorded) {wrong[:20]}"
    assert issued > 200


@pytest.mark.parametrize("d", sorted(DKV_LDS_REFUSED_S))
def test_attention_dkv_interval_table_refusal(d):
    import lxt_amd._lib as L
    a = base_call("lrp_attn_bwd_dkv", BF16, d)
    a.update(S=DKV_LDS_REFUSED_S[d], row_lo=16, row_hi=16)
    assert L.lib.lrp_attn_bwd_dkv(*a.values()) == -3
