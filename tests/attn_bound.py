"""Element-wise rounding bounds for the bf16 attention kernels (efficient placement: every stabiliser 0, sigma = scale / 2 as
tests/test_kernel_edges_gpu.py::_ref_bwd): an fp64 reference of every output, next to it the magnitude of the same sum taken over absolute
values, and from the two a WORST-CASE bound on what the kernel's roundings can do to that element.  Plain torch, any device; used by
tests/test_attn_bound_cpu.py (is the bound sound, does it discriminate) and tests/test_attn_bound_gpu.py (the kernels against it).

u = 2^-8 is the largest relative error of one round-to-nearest fp32 -> bf16 conversion, f = 2^-24 of one fp32 operation.  A bound is

    u x (the magnitude of what is rounded at each bf16 rounding point on the value's path)  +  one fp32 term.

No term carries a fitted constant: the factors are u, f, the head dim d and counts of roundings.

The bf16 rounding points, read out of the kernels (paths below lrp-explains-transformers_amd/):

  P -> bf16, the B operand of the P V / P^T Gho MFMAs (relative, so u A_o resp. u A_dv whatever the softmax's reference point is: the lazy
  running maximum of the d >= 64 forwards only moves the exponent)
      csrc/attention32_tiles.hpp:111   pack8: forward d in {64, 96, 128} (called at csrc/attention32.hip:158) and d = 256 (csrc/attention32.hip:895)
      csrc/attention_tiles.hpp:87      PackCols<bf16_t>::pack: d = 32 forward (csrc/attention.hip:695), d = 32 dK / dV (csrc/attention.hip:560)
      csrc/attention32.hip:598         dK / dV d in {64, 96, 128};  csrc/attention32.hip:1218  dK / dV d = 256 (pass 0)
      csrc/attention_cp.hip:252        the dV-only kernel
  dS = p (dP - D) -> bf16 (before the factor scale / 2, a power of two times scale in fp32: the rounding is relative, the magnitude is A_dq / A_dk)
      csrc/attention32_tiles.hpp:111   pack8: dQ and dQ-with-D d in {64, 96, 128} (csrc/attention32.hip:335), dQ d = 256 (csrc/attention32.hip:1038)
      csrc/attention_tiles.hpp:87      d = 32 dQ (csrc/attention.hip:838), d = 32 dK / dV (csrc/attention.hip:560)
      csrc/attention32.hip:599         dK / dV d in {64, 96, 128};  csrc/attention32.hip:1219  dK / dV d = 256 (pass 1)
  the store of the fp32 accumulator times its factor (1 / l, scale / 2 or 1) -> bf16
      csrc/attention32_tiles.hpp:235 and :247   store_rows<DH>: o, dq, dk_h, dv_h at d in {64, 96, 128, 256} (d = 256: csrc/attention32.hip:759), CP dv
      csrc/attention_tiles.hpp:124     store_rows<T, D>: o, dq, dk_h, dv_h at d = 32
  the GQA group sum: bf16 dk_h / dv_h summed in fp32, one store -> bf16
      csrc/common.hpp:90               Vec16<bf16_t>::set, called by gqa_reduce_kernel at csrc/attention.hip:928
  (The 4-wave kernels of csrc/attention.hip -- P at :145 and :390, dS at :290 and :390 with scale / 2 already inside, stores with factor 1 -- round at
  the same three places; at bf16 they serve only head-transposed operands off the 128-byte pitch grid, tests/test_kernel_edges_gpu.py::
  test_attention_narrow_transposed_pitch, and are not run by these cases.)
  No factor is folded into a bf16 MFMA operand: q, k, v and Gho go into the MFMAs as they are stored (csrc/rowops.hip:353 forms Gho = Go / 2, exact in
  bf16, and D from the rounded Gho); scale, log2 e, 1 / l and scale / 2 are all applied to fp32 values.

The fp32 term.  A score is a d-term fp32 MFMA sum, |error| <= d f scale sum_c |q_ic| |k_jc| <= d f A_s; the exponent's fma, the products with
scale log2 e and lse log2 e, the hardware exp2 and the reciprocal of l add single fp32 roundings of quantities bounded by A_s (resp. |lse|): 8 of them
are allowed for, E_s = (d + 8) f A_s.  The accuracy of the hardware exp2 / log2 (v_exp_f32, v_log_f32) is ASSUMED, not measured: 1 ulp = 2 f
each, which fits into the 8; nothing in this project states it or can evaluate the instruction off the device.  (tests/test_attn_bound_cpu.py::
test_exp2_of_the_model measures only the exp2 the CPU model itself uses, 1.18 f against fp64.)  A kernel that consumes lse inherits the forward's
lse error L as a relative error of p.  These are the forms the issue starts from; the model stays within them on every case, so nothing was
added to them because a bound was exceeded.  ONE term is added, by derivation: dP is a d-term fp32 sum and enters dS with an absolute error
(d + 8) f sum_c |Gho_ic| |v_jc|, which |dP| does not bound -- with one visible key p = 1, the reference dS is exactly 0 and that error is all
that is left of dq and dk.

    o          u (A_o + |o|)                                  + E_s A_o
    lse        E_s + 8 f (1 + |lse|)                          =: L
    D          (d + 8) f A_D
    dq         u (A_dq + |dq|)                                + sigma (P ((E_s + L) (|dP| + |D|) + (d + 8) f |Gho| |V|^T)) |K|
    dk_h       u (A_dk_h + |dk_h|)                            + sigma (P ((E_s + L) (|dP| + |D|) + (d + 8) f |Gho| |V|^T))^T |Q|
    dv_h       u (A_dv_h + |dv_h|)                            + ((E_s + L) P)^T |Gho|
    dk, dv     u (sum_h (A_h + |x_h|) + |x|)                  + the sum of the heads' fp32 terms                    (lrp_attn_bwd_dkv + lrp_gqa_reduce)
    CP dv      u (sum_h A_dv_h + |dv|)                        + sum_h ((E_s + 8 f (1 + |lse|)) P)^T |G|             (lrp_attn_bwd_dv: one store)

P is the normalised softmax under `vis` for everything but the CP dv, whose header defines P = exp(scale q.k - lse) on the lse it is handed."""
import torch

U = 2.0 ** -8
F = 2.0 ** -24

D_ALL = (32, 64, 96, 128, 256)
HEADS = ((2, 2), (8, 2))
S_ALL = (1, 33, 129, 257, 300)
B = 2
CP_DV_D = (64, 96, 128)          # the bf16 head dims of lrp_attn_bwd_dv (include/lrp_hip_attn_cp.h), for the CPU model; the GPU test asks attn_bwd_dv_ok


def masks(S):
    """the mask variants of one (d, heads, S): (name, causal, window, row_iv kind or None, q_begin).  tests/test_kernels_gpu.py::_intervals cannot
    build left_pad intervals at S = 1 (the pad width is taken modulo S // 2), so S = 1 runs the `packed` and `random` kinds."""
    out = [("causal", True, 0, None, 0), ("full", False, 0, None, 0), ("w48", True, 48, None, 0), ("w129", True, 129, None, 0)]
    out += [(kind, None, 0, kind, 0) for kind in (("left_pad", "packed", "random") if S > 1 else ("packed", "random"))]
    out += [(f"qb{qb}", True, 0, None, qb) for qb in sorted({37, S - 1}) if 0 < qb < S]
    return out


def bias_case(S, mask):
    """is (S, mask) a case of the signed-bias statistic (part c of tests/test_attn_bound_cpu.py)?  Left out, of the bias check only: S = 1 (one
    key per row: p = 1, dq = dk = 0, a few hundred elements in all) and the q_begin cases (dq has S - q_begin live rows, one at q_begin = S - 1:
    the round-to-nearest model's mean does not settle under a sixth of the truncating model's there, which the bar needs)."""
    return S > 1 and mask[4] == 0


def visible(Bn, S, causal, window, row_iv=None, q_begin=0, device="cpu"):
    """bool [B, 1, S, S] (query, key), built as tests/test_kernels_gpu.py and tests/test_kernel_edges_gpu.py build it; q_begin removes the query
    rows below it (they carry no gradient)"""
    i = torch.arange(S, device=device)
    vis = torch.ones(S, S, dtype=torch.bool, device=device)
    if causal:
        vis &= i[None, :] <= i[:, None]
    if window > 0:
        vis &= i[None, :] > i[:, None] - window
    vis = vis[None].repeat(Bn, 1, 1)
    if row_iv is not None:
        lo, hi = (t.to(device) for t in row_iv)
        vis &= (i[None, None, :] >= lo[:, :, None]) & (i[None, None, :] < hi[:, :, None])
    if q_begin:
        vis &= (i >= q_begin)[None, :, None]
    return vis[:, None]


def h4(x, Bn, S, H, d):
    """token-major [B S, H d] -> fp64 [B, H, S, d]"""
    return x.double().reshape(Bn, S, H, d).permute(0, 2, 1, 3)


def forward_ref(q, k, v, vis, scale):
    """q [B, Hq, S, d], k, v [B, Hkv, S, d] fp64 -> dict(P, s, o, A_o, lse, A_s, E_s, L, empty_q)"""
    rep, d = q.shape[1] // k.shape[1], q.shape[-1]
    S = q.shape[2]
    kx, vx = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    s = (q @ kx.transpose(-1, -2)) * scale
    sm = s.masked_fill(~vis, float("-inf"))
    P = torch.nan_to_num(torch.softmax(sm, -1), nan=0.0)
    lse = torch.logsumexp(sm, -1)
    A_s = ((q.abs() @ kx.abs().transpose(-1, -2)) * scale).masked_fill(~vis, 0.0).amax(-1)
    E_s = (d + 8) * F * A_s
    L = E_s + 8 * F * (1 + torch.nan_to_num(lse.abs(), posinf=0.0))
    return dict(P=P, s=s, o=P @ vx, A_o=P @ vx.abs(), lse=lse, A_s=A_s, E_s=E_s, L=L, empty_q=~vis.any(-1).expand_as(lse), rep=rep, d=d, S=S,
                scale=scale)


def bound_o(R):
    return U * (R["A_o"] + R["o"].abs()) + R["E_s"][..., None] * R["A_o"]


def bound_lse(R):
    return R["L"]


def d_ref(Gho, o_kernel):
    """D = rowsum(Gho o) of the kernel's own (bf16) Gho and o -> (D, bound)"""
    d = Gho.shape[-1]
    return (Gho * o_kernel).sum(-1), (d + 8) * F * (Gho.abs() * o_kernel.abs()).sum(-1)


def _group(x, rep):
    Bn, Hq, S, d = x.shape
    return x.reshape(Bn, Hq // rep, rep, S, d).sum(2)


def backward_ref(R, q, k, v, Gho, D, vis, parts=("dq", "dk", "dv")):
    """the backward on the kernel's own Gho [B, Hq, S, d] and D [B, Hq, S] (fp64 casts) -> dict of (reference, bound) per output; P is the
    normalised softmax of forward_ref"""
    rep, d, S, sg = R["rep"], R["d"], R["S"], 0.5 * R["scale"]
    kx, vx = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    P = R["P"]
    dP = Gho @ vx.transpose(-1, -2)
    A_dP = Gho.abs() @ vx.abs().transpose(-1, -2)
    dS = P * (dP - D[..., None])
    e = (R["E_s"] + R["L"])[..., None]                                 # relative error of p: its own score / exp and the forward's lse
    C = P * (e * (dP.abs() + D.abs()[..., None]) + (d + 8) * F * A_dP)      # |error| of dS before its bf16 rounding
    out = {}
    dq, A_dq = sg * (dS @ kx), sg * (dS.abs() @ kx.abs())
    out["dq"] = (dq, U * (A_dq + dq.abs()) + sg * (C @ kx.abs()))
    if "dk" not in parts:
        return out
    dk_h, A_dk = sg * (dS.transpose(-1, -2) @ q), sg * (dS.abs().transpose(-1, -2) @ q.abs())
    f_dk = sg * (C.transpose(-1, -2) @ q.abs())
    out["dk_h"] = (dk_h, U * (A_dk + dk_h.abs()) + f_dk)
    dv_h, A_dv = P.transpose(-1, -2) @ Gho, P.transpose(-1, -2) @ Gho.abs()
    f_dv = (e * P).transpose(-1, -2) @ Gho.abs()
    out["dv_h"] = (dv_h, U * (A_dv + dv_h.abs()) + f_dv)
    for name, x_h, A_h, f_h in (("dk", dk_h, A_dk, f_dk), ("dv", dv_h, A_dv, f_dv)):
        x = _group(x_h, rep)
        out[name] = (x, U * (_group(A_h + x_h.abs(), rep) + x.abs()) + _group(f_h, rep))
    out["empty_k"] = ~vis.any(-2).expand(q.shape[0], q.shape[1], S)                   # [B, Hq, S]: keys no query sees (vis has 1 or Hq heads)
    return out


def cp_dv_ref(R, q, k, G, lse_kernel, vis):
    """lrp_attn_bwd_dv's own definition: P = exp(scale q.k - lse) on the lse it is handed -> (dv [B, Hkv, S, d], bound)"""
    rep = R["rep"]
    P = torch.where(vis, torch.exp(R["s"] - lse_kernel[..., None]), torch.zeros_like(R["s"]))
    e = (R["E_s"] + 8 * F * (1 + torch.nan_to_num(lse_kernel.abs(), nan=0.0, posinf=0.0)))[..., None]      # (a row that sees nothing: P = 0)
    dv, A = _group(P.transpose(-1, -2) @ G, rep), _group(P.transpose(-1, -2) @ G.abs(), rep)
    return dv, U * (A + dv.abs()) + _group((e * P).transpose(-1, -2) @ G.abs(), rep)


def ratio(x, ref, bound):
    """worst |x - ref| / bound and its index; an element with bound 0 counts as 0 when it is exact and inf when it is not"""
    err = (x - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))                    # a reference or an output that is not finite is outside every bound
    if r.numel() == 0:
        return 0.0, ()
    flat = int(r.argmax())
    return float(r.reshape(-1)[flat]), tuple(int(t) for t in torch.unravel_index(torch.tensor(flat), r.shape))


def check(name, x, ref, bound, empty=None, rows=0, log=None, strict=True):
    """x, ref, bound [B, H, S, d] or [B, H, S] (fp64): finite; |x - ref| <= bound element-wise; exact zeros where `empty` [B, H, S] says that the
    reference sum has no term (a query row or a key that nothing sees); rows: check query rows >= rows only.  Prints the worst err / bound and
    where it sits, and appends it to log[name].  strict = False (the planted faults of the CPU test): nothing is asserted, the ratio is returned."""
    if rows:
        x, ref, bound = x[:, :, rows:], ref[:, :, rows:], bound[:, :, rows:]
        empty = None if empty is None else empty[:, :, rows:]
    if strict:
        assert torch.isfinite(x).all(), f"{name}: not finite"
        if empty is not None and bool(empty.any()):
            assert bool((x[empty] == 0).all()), f"{name}: an empty sum is not an exact zero"
    worst, at = ratio(torch.nan_to_num(x, nan=float("inf")), ref, bound)
    if rows and at:
        at = at[:2] + (at[2] + rows,) + at[3:]
    if log is not None:
        log[name] = max(log.get(name, 0.0), worst)
    if strict:
        print(f"  {name}: worst err / bound = {worst:.3f} at (b, head, row, col) = {at}")
        assert worst <= 1.0, (name, worst, at)
    return worst


def bias(x, ref):
    """the signed statistic that tells truncation from round-to-nearest: mean over |ref| > 1e-3 max|ref| of (x - ref) sign(ref) / |ref|, in units of u"""
    m = ref.abs() > 1e-3 * ref.abs().max()
    return float((((x - ref) * torch.sign(ref))[m] / ref.abs()[m]).mean()) / U


def evaluate(out, q, k, v, vis, scale, q_begin=0, log=None, strict=True):
    """every output of one pipeline call against its bound.  q, k, v: fp64 [B, H, S, d]; vis: visible(...) WITHOUT q_begin; out: fp64 tensors
    [B, H, S, d] / [B, H, S] under the keys o, lse (the forward under test: rows >= q_begin), o_bwd, lse_bwd (the forward the backward was
    fed; default o, lse), Gho, D, dq, dk_h, dv_h, dk, dv and, where they were run, D2, dq2, cp_dv.  -> {name: worst err / bound}"""
    log = {} if log is None else log
    Hkv = k.shape[1]
    R = forward_ref(q, k, v, vis, scale)
    kw = dict(log=log, strict=strict)
    check("o", out["o"], R["o"], bound_o(R), empty=R["empty_q"], rows=q_begin, **kw)
    seen = ~R["empty_q"]
    check("lse", torch.where(seen, out["lse"], torch.zeros_like(out["lse"])), torch.where(seen, R["lse"], torch.zeros_like(R["lse"])),
          bound_lse(R), rows=q_begin, **kw)
    if "Gho" not in out:
        return log
    if q_begin:
        i = torch.arange(vis.shape[-1], device=vis.device)
        vis = vis & (i >= q_begin)[None, None, :, None]
        R = forward_ref(q, k, v, vis, scale)
    Gho, D = out["Gho"], out["D"]
    D_ref, D_bound = d_ref(Gho, out.get("o_bwd", out["o"]))
    check("D", D, D_ref, D_bound, **kw)
    Bk = backward_ref(R, q, k, v, Gho, D, vis)
    empty_k = Bk["empty_k"]
    check("dq", out["dq"], *Bk["dq"], empty=R["empty_q"], rows=q_begin, **kw)
    for name in ("dk_h", "dv_h"):
        check(name, out[name], *Bk[name], empty=empty_k, **kw)
    for name in ("dk", "dv"):
        check(name, out[name], *Bk[name], empty=empty_k[:, :Hkv], **kw)
    if "dq2" in out:
        check("D2", out["D2"], D_ref, D_bound, **kw)
        check("dq2", out["dq2"], *backward_ref(R, q, k, v, Gho, out["D2"], vis, parts=("dq",))["dq"], empty=R["empty_q"], **kw)
    if "cp_dv" in out:
        check("cp_dv", out["cp_dv"], *cp_dv_ref(R, q, k, Gho, out.get("lse_bwd", out["lse"]), vis), empty=empty_k[:, :Hkv], **kw)
    return log


# ---- the torch model of the kernels' arithmetic (tests/test_attn_bound_cpu.py; the GPU test takes its bias bars from the truncating form)
LOG2E = 1.4426950408889634


def rne(x):
    return x.to(torch.bfloat16).float()


def trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def model(q, k, v, Go, vis, scale, rnd=rne, kv_map=None, dv_skip=None, cp=True):
    """the kernels' arithmetic in torch: fp32 everywhere, `rnd` (fp32 -> bf16 -> fp32) where the kernels convert.  vis [B, 1, S, S] is the mask the
    MODEL applies (a fault hands it a wrong one); kv_map [Hq]: the kv head each query head reads (fault: a neighbour's); dv_skip: a query head
    left out of the dv group sums (fault).  -> fp64 outputs under the keys of attn_bound.evaluate"""
    Bn, Hq, S, d = q.shape
    Hkv = k.shape[1]
    rep = Hq // Hkv
    kv_map = torch.arange(Hq, device=q.device) // rep if kv_map is None else kv_map
    kx, vx = k[:, kv_map], v[:, kv_map]
    c1 = torch.tensor(scale * LOG2E, dtype=torch.float32, device=q.device)
    s = q @ kx.transpose(-1, -2)                                           # raw scores, fp32
    zero = torch.zeros_like(s)
    # forward: p against the row maximum (the kernels' running / lazy maxima move the exponent only), l from the un-rounded p, P -> bf16, o -> bf16
    m = s.masked_fill(~vis, float("-inf")).amax(-1, keepdim=True)
    m_use = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.where(vis, torch.exp2(s * c1 - m_use * c1), zero)
    l = p.sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o = rnd((rnd(p) @ vx) * inv)
    lse = (m * scale + torch.log(l)).squeeze(-1)
    # attn_bwd_prep: Gho = Go / 2 (exact), D from the rounded Gho and the stored o
    Gho = rnd(0.5 * Go)
    D = (Gho * o).sum(-1)
    # backward: p from lse, dS = p (dP - D) -> bf16, the contractions in fp32, scale / 2 at the store
    p2 = torch.where(vis, torch.exp2(s * c1 - (lse * LOG2E)[..., None]), zero)
    dS = rnd(p2 * (Gho @ vx.transpose(-1, -2) - D[..., None]))
    sg = 0.5 * scale
    dq = rnd((dS @ kx) * sg)
    dk_h = rnd((dS.transpose(-1, -2) @ q) * sg)
    pb = rnd(p2)
    dv_h = rnd(pb.transpose(-1, -2) @ Gho)
    grp = lambda x: x.reshape(Bn, Hkv, rep, S, d).sum(2)      # noqa: E731
    keep = torch.ones(Hq, device=q.device)
    if dv_skip is not None:
        keep[dv_skip] = 0
    keep = keep[None, :, None, None]
    out = dict(o=o, lse=lse, Gho=Gho, D=D, dq=dq, dk_h=dk_h, dv_h=dv_h, dk=rnd(grp(dk_h)), dv=rnd(grp(dv_h * keep)))
    if cp:
        out["cp_dv"] = rnd(grp((pb.transpose(-1, -2) @ Gho) * keep))      # one fp32 accumulator across the group, one store
    return {key: x.double() for key, x in out.items()}


def references(out, q, k, v, vis, scale):
    """the fp64 references attn_bound.evaluate holds o, dq, dk, dv (and the CP dv) to; vis: with q_begin applied"""
    R = forward_ref(q, k, v, vis, scale)
    Bk = backward_ref(R, q, k, v, out["Gho"], out["D"], vis)
    refs = dict(o=R["o"], dq=Bk["dq"][0], dk=Bk["dk"][0], dv=Bk["dv"][0])
    if "cp_dv" in out:
        refs["cp_dv"] = cp_dv_ref(R, q, k, out["Gho"], out.get("lse_bwd", out["lse"]), vis)[0]
    return refs


def biases(out, q, k, v, vis, scale):
    """the signed statistic of o, dq, dk, dv (and the CP dv) of one call (q_begin = 0), in units of u"""
    return {name: bias(out[name], ref) for name, ref in references(out, q, k, v, vis, scale).items()}
