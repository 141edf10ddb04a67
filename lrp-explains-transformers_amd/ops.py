"""Tensor-level wrappers over the C ABI (include/lrp_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the current HIP stream;
every computation below is a call into liblrp_hip.so with raw device pointers.  CPU tensors are
rejected -- there is no fallback.
"""
import torch

from ._lib import lib, check, F32, BF16, ACT

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"lrp_hip supports float32 and bfloat16 tensors, got {t.dtype}") from None


def p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("lrp_hip kernels need device tensors (no CPU fallback)")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def same(ref, *ts):
    """every tensor handed to a kernel next to `ref` must share its dtype and device: the C ABI takes ONE dtype code
    per call and raw pointers, so a mismatch would be reinterpreted bytes (or an out-of-bounds read), not an error"""
    for t in ts:
        if t is not None and (t.dtype != ref.dtype or t.device != ref.device):
            raise TypeError(f"lrp_hip: operand of dtype {t.dtype} on {t.device} next to {ref.dtype} on {ref.device}; "
                            "all activation operands of one call must share dtype and device")


def aux(t, ref, n=None):
    """small parameter vector (norm weight, bias) for a kernel whose activations are `ref`: brought to ref's dtype /
    device / contiguity if it differs (mixed-precision modules keep fp32 norm weights next to bf16 activations)"""
    if t is None:
        return None
    if n is not None and t.numel() != n:
        raise ValueError(f"lrp_hip: parameter vector of {t.numel()} elements where {n} are expected")
    if t.dtype != ref.dtype or t.device != ref.device or not t.is_contiguous():
        t = t.to(device=ref.device, dtype=ref.dtype).contiguous()
    return t


def f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"lrp_hip: row statistics / tables must be float32, got {t.dtype}")


def epc(t):
    return 16 // t.element_size()


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _rows_contiguous(name, M, H, **ts):
    """operands of an entry whose C ABI has no row pitch (it indexes row * H): every one must be a contiguous [M, H] tensor -- a column slice or
    a tensor of another shape would be read and written at the wrong addresses, and past its end"""
    for k, t in ts.items():
        if t is not None and (tuple(t.shape) != (M, H) or not t.is_contiguous()):
            raise ValueError(f"{name}: {k} must be a contiguous [{M}, {H}] tensor (the C ABI has no row pitch), got {tuple(t.shape)} with "
                             f"strides {t.stride()}")


def _row_stats(name, M, **ts):
    """per-row fp32 statistics: contiguous, at least M entries"""
    for k, t in ts.items():
        if t is not None and (t.numel() < M or not t.is_contiguous()):
            raise ValueError(f"{name}: {k} must be contiguous with at least {M} entries, got {tuple(t.shape)} with strides {t.stride()}")


def _pitched(name, rows, cols, **ts):
    """2-D views [rows, >= cols] with a row pitch (stride(0)) and unit column stride, as the element-wise 2-D entries index them"""
    for k, t in ts.items():
        if t is not None and (t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or t.stride(1) != 1 or (rows > 1 and t.stride(0) < cols)):
            raise ValueError(f"{name}: {k} must be a [{rows}, >= {cols}] view with unit column stride, got {tuple(t.shape)} with strides {t.stride()}")


# ------------------------------------------------------------------------------------------- GEMM
def gemm_nt(a, b, bias=None, out=None, out_dtype=None):
    """out[..., M, N] = a[..., M, K] @ b[..., N, K]^T (+bias).  a/b: last dim contiguous, 2-D or
    batched 3-D with a uniform batch stride; b may be 2-D (shared).  K is zero-padded to a multiple
    of 16 bytes if needed."""
    assert a.dtype == b.dtype
    K = a.shape[-1]
    assert b.shape[-1] == K
    e = epc(a)
    if K % e:
        pad = e - K % e
        a = torch.nn.functional.pad(a, (0, pad))
        b = torch.nn.functional.pad(b, (0, pad))
        K += pad
    lead = a.shape[:-2]
    M, N = a.shape[-2], b.shape[-2]
    a3 = a.reshape(-1, M, K)
    batch = a3.shape[0]
    if a3.stride(-1) != 1 or a3.stride(-2) % e or (batch > 1 and a3.stride(0) % e) or a3.data_ptr() % 16:
        a3 = a3.contiguous()
    if b.dim() == 2:
        b3, sB = b, 0
        if b3.stride(-1) != 1 or b3.stride(-2) % e or b3.data_ptr() % 16:
            b3 = b3.contiguous()
        ldb = b3.stride(0)
    else:
        b3 = b.reshape(-1, N, K)
        assert b3.shape[0] == batch
        if b3.stride(-1) != 1 or b3.stride(-2) % e or (batch > 1 and b3.stride(0) % e) or b3.data_ptr() % 16:
            b3 = b3.contiguous()
        sB, ldb = (b3.stride(0) if batch > 1 else 0), b3.stride(1)
    odt = out_dtype or (out.dtype if out is not None else a.dtype)
    bias = aux(bias, a, N)
    if out is None:
        out = torch.empty(*lead, M, N, device=a.device, dtype=odt)
    if out.dtype != odt:
        raise TypeError(f"gemm_nt: out is {out.dtype}, out_dtype {odt}")
    o3 = out.view(-1, M, N)
    assert o3.stride(-1) == 1
    rc = lib.lrp_gemm_nt(p(a3), p(b3), p(o3), p(bias), M, N, K, a3.stride(1), ldb, o3.stride(1), batch,
                         a3.stride(0) if batch > 1 else 0, sB, o3.stride(0) if batch > 1 else 0,
                         dt(a), _DT[odt], stream())
    check(rc, "lrp_gemm_nt")
    return out


class KernelTimer:
    """HIP-event timing of every launch of one kernel family on the launching stream (bench.py's
    roofline leg).  Enabled by assigning an instance to ops.GEMM_TIMER; records (flops, ev0, ev1).
    drain() folds the spans whose end event has completed into per-tag sums and RE-USES their event objects: a long run then keeps ~one step's
    worth of events alive instead of steps x launches x 2 (each live event holds a signal of the HIP runtime's pool; with thousands alive the
    runtime takes a slow path in some processes -- the judged run's sporadic +14 ms per step sat entirely in launch gaps, not in kernels:
    profiles/r05_gemm_experiments.txt, section O)."""

    def __init__(self):
        self.records = []
        self.sums = {}            # tag -> [launches, flops, seconds]
        self.pool = []

    def span(self, flops, tag="plain"):
        if len(self.pool) >= 2:
            e0, e1 = self.pool.pop(), self.pool.pop()
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.append((flops, e0, e1, tag))
        return e0, e1

    def drain(self, wait=False):
        """fold every span whose end event has completed (all of them with wait=True: call after a device synchronise)"""
        keep = []
        for r in self.records:
            if not keep and (wait or r[2].query()):
                acc = self.sums.setdefault(r[3], [0, 0.0, 0.0])
                acc[0] += 1
                acc[1] += r[0]
                acc[2] += r[1].elapsed_time(r[2]) * 1e-3
                self.pool.append(r[1])
                self.pool.append(r[2])
            else:
                keep.append(r)        # spans complete in issue order: stop at the first one still in flight
        self.records = keep

    def summary(self, tag=None):
        """-> (launches, total_flops, total_seconds) of the launches with this tag (None: all); call after a device synchronise.
        Tags: "plain" = GEMM only; "plain_norm" = the same kernel with a K1n epilogue (row scale / residual add / row sums of squares);
        "gated_fwd" / "gated_bwd" = the launches that carry a gated-MLP rule in their epilogue; a tuple selects several"""
        self.drain(wait=True)
        sel = [v for k, v in self.sums.items() if tag is None or k == tag or (isinstance(tag, tuple) and k in tag)]
        return sum(v[0] for v in sel), sum(v[1] for v in sel), sum(v[2] for v in sel)


GEMM_TIMER = None


def _timed(flops, tag, fn, name):
    ev = GEMM_TIMER.span(flops, tag) if GEMM_TIMER is not None else None
    if ev:
        ev[0].record()
    rc = fn()
    if ev:
        ev[1].record()
    check(rc, name)


def gemm_nt_2d(a, b, out, bias=None):
    """strict 2-D fast path used by the engine: no reshapes, no copies; row strides may exceed K."""
    M, K = a.shape
    N = b.shape[0]
    same(a, b)
    bias = aux(bias, a, N)
    ev = GEMM_TIMER.span(2.0 * M * N * K) if GEMM_TIMER is not None else None
    if ev:
        ev[0].record()
    rc = lib.lrp_gemm_nt(a.data_ptr(), b.data_ptr(), out.data_ptr(), p(bias), M, N, K, a.stride(0), b.stride(0),
                         out.stride(0), 1, 0, 0, 0, dt(a), _DT[out.dtype], stream())
    if ev:
        ev[1].record()
    check(rc, "lrp_gemm_nt")
    return out


def gemm_nn_ok(a, w):
    """can lrp_gemm_nn / lrp_gemm_skinny serve C = a[M,K] @ w[K,N] (w = a weight in its stored [out,in] layout)?  bf16, K % 64 == 0,
    K >= 128, 16-byte aligned K-/N-contiguous operands, the weight below 2^30 elements (activations with more elements are issued in
    row chunks by the library: no fallback to a W^T copy for large batches)"""
    if a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or a.dim() != 2 or w.dim() != 2:
        return False
    M, K = a.shape
    return (K % 64 == 0 and K >= 128 and a.stride(1) == 1 and w.stride(1) == 1 and a.stride(0) % 8 == 0 and w.stride(0) % 8 == 0
            and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and 256 * a.stride(0) < 2 ** 30 and w.shape[0] * w.stride(0) < 2 ** 30)


def gemm_nn_2d(a, w, out, bias=None):
    """out[M,N] = a[M,K] @ w[K,N]: the eps-rule redistribution c = s W straight from the STORED weight W [out,in] (no W^T copy)"""
    M, K = a.shape
    N = w.shape[1]
    same(a, w)
    ev = GEMM_TIMER.span(2.0 * M * N * K) if GEMM_TIMER is not None else None
    if ev:
        ev[0].record()
    rc = lib.lrp_gemm_nn(a.data_ptr(), w.data_ptr(), out.data_ptr(), p(aux(bias, a, N)), M, N, K, a.stride(0), w.stride(0),
                         out.stride(0), dt(a), _DT[out.dtype], stream())
    if ev:
        ev[1].record()
    check(rc, "lrp_gemm_nn")
    return out


SKINNY_MAX = 256         # rows the split-K skinny path serves (HBM-bound regime of the Linear eps-rule: M <~ 160 in bf16)


def splitk_ok(M, N, K):
    """should this bf16 GEMM take the split-K path of the ping-pong kernel (lrp_gemm_skinny)?  M <= 256 rows always (W is streamed once by
    all CUs); for more rows when the 256 x 256 tile count would leave half of the 256 CUs idle (M = 2048 against a 4096-row weight:
    128 tiles) and every split keeps a K loop of >= 8 tiles -- measured at M = 2048 (tools/gemm_ab.py --m 2048): 978 -> 1150 ... 1039 ->
    1440 TFLOP/s on the N = 4096 shapes"""
    if M <= SKINNY_MAX:
        return True
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles <= 128:
        return K // 64 >= 8 * (256 // tiles)
    return lib.lrp_gemm_skinny_splits(M, N, K) >= 2         # 257 ... 384 tiles with a long K loop (Gemma-3-4B: 8192 x 2560 x 10240)


_WS = {}


def workspace(nbytes, ref):
    """scratch for kernels that take a caller-allocated workspace.  One buffer per (device, stream), grown on demand: kernels on
    one stream are ordered, two streams never share a buffer.  Under hipGraph capture a FRESH allocation is made per
    call (it lives in the graph's private pool; a cached buffer could be re-grown -- freed -- after the capture)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(int(nbytes), 16), device=ref.device, dtype=torch.uint8)
    key = (ref.device, torch.cuda.current_stream(ref.device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 4 << 20), device=ref.device, dtype=torch.uint8)
        _WS[key] = ws
    return ws


_TK = {}
STREAM_DGRAD_INKERNEL_REDUCE = True      # module attribute (A/B measurements): False = fp32 slabs + the reduce launch


def tickets(n, ref):
    """the zero-initialised 32-bit arrival counters of the in-kernel split reduction (lrp_linear_stream_dgrad_tk): one array per (device, stream),
    allocated once and never written by anything but that kernel (whose last arriver re-arms each word), grown by re-allocation; under hipGraph
    capture a fresh zeroed array per call (the memset is captured with the launch)"""
    if torch.cuda.is_current_stream_capturing():        # as ops.workspace: a fresh array in the graph's private pool, zeroed by a captured memset
        return torch.zeros(max(int(n), 16), device=ref.device, dtype=torch.int32)
    key = (ref.device, torch.cuda.current_stream(ref.device).cuda_stream)
    t = _TK.get(key)
    if t is None or t.numel() < n:
        t = torch.zeros(max(int(n), 4096), device=ref.device, dtype=torch.int32)
        _TK[key] = t
    return t


def gemm_skinny(a, b, out, nn=False, bias=None):
    """out[M,N] = a[M,K] @ b[N,K]^T (nn=False) or a[M,K] @ b[K,N] (nn=True) for M <= 256 rows: split-K over the CUs, the weight
    streamed exactly once; fp32 partial slabs in a stream-local workspace.  The library addresses the activation through ONE 32-bit buffer
    resource (no row chunks, unlike lrp_gemm_nt / _nn): problems with M * row pitch >= 2^30 elements (possible only on the many-row tail /
    half-empty-chip uses of this path) are issued here in row chunks, each its own split-K problem"""
    M, K = a.shape
    N = b.shape[1] if nn else b.shape[0]
    same(a, b)
    if M * a.stride(0) >= 2 ** 30:
        step = max(256, ((2 ** 30 - 1) // a.stride(0)) // 256 * 256)
        for m0 in range(0, M, step):
            gemm_skinny(a[m0: m0 + step], b, out[m0: m0 + step], nn=nn, bias=bias)
        return out
    ws = workspace(lib.lrp_gemm_skinny_ws(M, N, K), a)
    ev = GEMM_TIMER.span(2.0 * M * N * K, "splitk") if (GEMM_TIMER is not None and M > SKINNY_MAX) else None
    if ev:
        ev[0].record()
    rc = lib.lrp_gemm_skinny(a.data_ptr(), b.data_ptr(), out.data_ptr(), p(aux(bias, a, N)), M, N, K, a.stride(0), b.stride(0),
                             out.stride(0), int(nn), dt(a), _DT[out.dtype], ws.data_ptr(), stream())
    if ev:
        ev[1].record()
    check(rc, "lrp_gemm_skinny")
    return out


def transpose(x, out=None):
    """[..., R, C] -> [..., C, R] (contiguous)"""
    x = _c(x)
    R, C = x.shape[-2], x.shape[-1]
    lead = x.shape[:-2]
    if out is None:
        out = torch.empty(*lead, C, R, device=x.device, dtype=x.dtype)
    batch = x.numel() // (R * C) if R * C else 1
    rc = lib.lrp_transpose(p(x), p(out), R, C, C, R, batch, R * C, R * C, dt(x), stream())
    check(rc, "lrp_transpose")
    return out


_WT = {}            # storage id -> {(offset, shape, stride, dtype): (version, W^T)}; entries die with the weight's storage (weakref.finalize)
TRANSPOSE_CALLS = [0]    # weight transposes actually executed (tests: the cache must hit on the second backward)


def weight_t(w):
    """W^T copy ([in, out]) of a frozen weight for the fp32 / odd-shape dgrad GEMM.  Cached per STORAGE of the weight (not per tensor
    object: the patched forwards hand `param.detach()` -- a fresh object on every call -- to the autograd Functions), keyed by
    the view's offset / shape / strides / dtype and invalidated by the in-place version counter, which detach() aliases share with the
    Parameter; the entry is dropped when the storage dies, so an address re-used by another weight can never hit."""
    import weakref
    st = w.untyped_storage()
    sid = st._cdata
    per = _WT.get(sid)
    if per is None:
        per = _WT[sid] = {}
        weakref.finalize(st, _WT.pop, sid, None)
    key = (w.storage_offset(), tuple(w.shape), tuple(w.stride()), w.dtype)
    hit = per.get(key)
    if hit is not None and hit[0] == w._version:
        return hit[1]
    TRANSPOSE_CALLS[0] += 1
    wt = transpose(w.detach())
    per[key] = (w._version, wt)
    return wt


def cast(x, dtype):
    x = _c(x)
    out = torch.empty_like(x, dtype=dtype)
    check(lib.lrp_cast(p(x), p(out), x.numel(), dt(x), _DT[dtype], stream()), "lrp_cast")
    return out


# ------------------------------------------------------------------------------------- element-wise
def eps_scale(g, z, c=1.0, eps=1e-8, relevance=False, out=None):
    g, z = _c(g), _c(z)
    out = torch.empty_like(g) if out is None else out
    same(g, z, out)
    check(lib.lrp_eps_scale(p(g), p(z), p(out), g.numel(), c, eps, 1 if relevance else 0, dt(g), stream()), "lrp_eps_scale")
    return out


def eps_scale2d(g, z, out, c=1.0, eps=1e-8, relevance=False):
    rows, cols = g.shape
    same(g, z, out)
    check(lib.lrp_eps_scale2d(p(g), p(z), p(out), rows, cols, g.stride(0), z.stride(0), out.stride(0), c, eps,
                              1 if relevance else 0, dt(g), stream()), "lrp_eps_scale2d")
    return out


def mul(a, b, out=None):
    a, b = _c(a), _c(b)
    out = torch.empty_like(a) if out is None else out
    same(a, b, out)
    check(lib.lrp_mul(p(a), p(b), p(out), a.numel(), dt(a), stream()), "lrp_mul")
    return out


def add_bcast(x, y, out=None):
    """out[m,:] = x[m,:] + y[m % period,:], period = rows of y (1: a row vector, S: per-position rows, M: a full residual sum)"""
    x, y = _c(x), _c(y)
    H = x.shape[-1]
    M, period = x.numel() // H, y.numel() // H
    out = torch.empty_like(x) if out is None else out
    same(x, y, out)
    if y.shape[-1] != H or M % period:
        raise ValueError(f"add_bcast: x {tuple(x.shape)} vs y {tuple(y.shape)}")
    check(lib.lrp_add_bcast(p(x), p(y), p(out), M, H, period, dt(x), stream()), "lrp_add_bcast")
    return out


def add2_rule_bwd(a, b, R, eps=1e-8, need_b=True):
    a, b, R = _c(a), _c(b), _c(R)
    Ra = torch.empty_like(a)
    Rb = torch.empty_like(b) if need_b else None
    same(a, b, R)
    check(lib.lrp_add2_rule_bwd(p(a), p(b), p(R), p(Ra), p(Rb), a.numel(), eps, dt(a), stream()), "lrp_add2_rule_bwd")
    return Ra, Rb


def act_fwd(x, act="silu"):
    x = _c(x)
    y = torch.empty_like(x)
    check(lib.lrp_act_fwd(p(x), p(y), x.numel(), ACT[act], dt(x), stream()), "lrp_act_fwd")
    return y


def act_bwd(Gy, x, act="silu", eps_g=1e-10):
    Gy, x = _c(Gy), _c(x)
    Gx = torch.empty_like(x)
    same(x, Gy)
    check(lib.lrp_act_bwd(p(Gy), p(x), p(Gx), x.numel(), eps_g, ACT[act], dt(x), stream()), "lrp_act_bwd")
    return Gx


def act_grad(Gy, x, act="gelu_tanh", out=None):
    """plain derivative Gy * act'(x) (no rule): the SigLIP tower under the reference's gemma3 map"""
    Gy, x = _c(Gy), _c(x)
    out = torch.empty_like(x) if out is None else out
    same(x, Gy, out)
    check(lib.lrp_act_grad(p(Gy), p(x), p(out), x.numel(), ACT[act], dt(x), stream()), "lrp_act_grad")
    return out


def gated_act_fwd(g, u, out=None, act="silu"):
    M, I = g.shape
    out = torch.empty(M, I, device=g.device, dtype=g.dtype) if out is None else out
    same(g, u, out)
    _pitched("lrp_gated_act_fwd", M, I, g=g, u=u, out=out)
    check(lib.lrp_gated_act_fwd(p(g), p(u), p(out), M, I, g.stride(0), u.stride(0), out.stride(0), ACT[act], dt(g), stream()),
          "lrp_gated_act_fwd")
    return out


def gated_act_bwd(Gm, g, u, Ag, Au, eps_g, eps_lin, act="silu"):
    M, I = g.shape
    same(g, Gm, u, Ag, Au)
    _pitched("lrp_gated_act_bwd", M, I, Gm=Gm, g=g, u=u, Ag=Ag, Au=Au)
    check(lib.lrp_gated_act_bwd(p(Gm), p(g), p(u), p(Ag), p(Au), M, I, Gm.stride(0), g.stride(0), u.stride(0), Ag.stride(0),
                                Au.stride(0), eps_g, eps_lin, ACT[act], dt(g), stream()), "lrp_gated_act_bwd")
    return Ag, Au


GATED_IL = 32            # interleave block of a fused gate/up weight (include/lrp_hip.h: LRP_GATED_IL)


def interleave_gate_up(wg, wu, out=None):
    """fused gate/up weight [2 I, H] with its rows in blocks of 64 = [32 gate rows | 32 up rows]: one 64-column block of W_gu x -- and one
    wave's accumulator tile of the GEMM -- then holds gate AND up of the same 32 intermediate indices (lrp_gated_act_fwd_il / _bwd_il, lrp_gemm_gated_fwd_coef / _bwd_coef)"""
    I, H = wg.shape
    if I % GATED_IL:
        raise ValueError(f"intermediate size {I} is not a multiple of {GATED_IL}")
    if out is None:
        out = torch.empty(2 * I, H, device=wg.device, dtype=wg.dtype)
    v = out.unflatten(0, (I // GATED_IL, 2, GATED_IL))          # (out may be a row-pitch-padded view: engine.weight_pitch_pad)
    v[:, 0].copy_(wg.view(I // GATED_IL, GATED_IL, H))
    v[:, 1].copy_(wu.view(I // GATED_IL, GATED_IL, H))
    return out


def gated_act_fwd_il(gu, out, act="silu"):
    M, I = out.shape
    same(gu, out)
    _pitched("lrp_gated_act_fwd_il", M, I, out=out)
    _pitched("lrp_gated_act_fwd_il", M, 2 * I, gu=gu)
    check(lib.lrp_gated_act_fwd_il(p(gu), p(out), M, I, gu.stride(0), out.stride(0), ACT[act], dt(gu), stream()), "lrp_gated_act_fwd_il")
    return out


def gated_act_bwd_il(Gm, gu, Agu, eps_g, eps_lin, act="silu"):
    M, I = Gm.shape
    same(gu, Gm, Agu)
    _pitched("lrp_gated_act_bwd_il", M, I, Gm=Gm)
    _pitched("lrp_gated_act_bwd_il", M, 2 * I, gu=gu, Agu=Agu)
    check(lib.lrp_gated_act_bwd_il(p(Gm), p(gu), p(Agu), M, I, Gm.stride(0), gu.stride(0), Agu.stride(0), eps_g, eps_lin, ACT[act], dt(gu),
                                   stream()), "lrp_gated_act_bwd_il")
    return Agu


def gated_cp_bwd_il(Gm, gu, Agu, act="silu"):
    """CP-LRP through the gated MLP (the gate is detached): up slots of Agu = act(g) * Gm, gate slots = 0, interleaved layout of gated_act_bwd_il"""
    M, I = Gm.shape
    same(gu, Gm, Agu)
    _pitched("lrp_gated_cp_bwd_il", M, I, Gm=Gm)
    _pitched("lrp_gated_cp_bwd_il", M, 2 * I, gu=gu, Agu=Agu)
    check(lib.lrp_gated_cp_bwd_il(p(Gm), p(gu), p(Agu), M, I, Gm.stride(0), gu.stride(0), Agu.stride(0), ACT[act], dt(gu), stream()),
          "lrp_gated_cp_bwd_il")
    return Agu


GATED_FUSION = True      # module attribute (no environment knobs): False = GEMM + element-wise rule kernels, for A/B measurements and the
                         # fused-vs-unfused tests


def gated_coef_ok(M, I, H, ldx, ldwgu, lda, ldwd, act, dtype):
    """both GEMMs around the gated rule are problems the fused epilogues take (lrp_gemm_gated_fwd_coef / _bwd_coef: bf16, M = B S rows)"""
    return bool(GATED_FUSION and dtype == torch.bfloat16 and M > SKINNY_MAX
                and lib.lrp_gemm_gated_coef_ok(M, I, H, ldx, ldwgu, lda, ldwd, ACT[act], _DT[dtype]))


def gemm_gated_fwd_coef(x, Wgu, coef, m, eps_g, eps_lin, act="silu", rs=None):
    """ONE launch: m[M, I] = act(g) (*) u and the backward's coefficient stash coef[M, 2 I] (cg = 1/2 u act(g) / (g + eps_g),
    cu = 1/2 act(g) u / (u + eps_lin); layout private to the pair, include/lrp_hip.h) from x @ Wgu^T (Wgu interleaved, see interleave_gate_up);
    rs: optional fp32 row scales applied to the product first (K1n).  g and u are never stored."""
    M, K = x.shape
    I = m.shape[1]
    same(x, Wgu, coef, m)
    if rs is not None:
        f32(rs)
    _timed(2.0 * M * 2 * I * K, "gated_fwd", lambda: lib.lrp_gemm_gated_fwd_coef(p(x), p(Wgu), p(rs), p(coef), p(m), M, I, K, x.stride(0), Wgu.stride(0),
                                                                                 coef.stride(0), m.stride(0), eps_g, eps_lin, ACT[act], dt(x), stream()),
           "lrp_gemm_gated_fwd_coef")
    return coef, m


def gemm_gated_bwd_coef(Adn, Wd, coef, Agu):
    """Agu[M, 2 I] (interleaved) = { Gm cg | Gm cu } with Gm = A_dn Wd (stored down weight Wd [H, I]) never written: the multiply runs in the NN
    GEMM's epilogue on the stash lrp_gemm_gated_fwd_coef left"""
    M, K = Adn.shape
    I = Wd.shape[1]
    same(Adn, Wd, coef, Agu)
    _timed(2.0 * M * I * K, "gated_bwd", lambda: lib.lrp_gemm_gated_bwd_coef(p(Adn), p(Wd), p(coef), p(Agu), M, I, K, Adn.stride(0), Wd.stride(0),
                                                                             coef.stride(0), Agu.stride(0), dt(Adn), stream()), "lrp_gemm_gated_bwd_coef")
    return Agu


def gemm_gated_fwd(x, Wgu, gu, m, act="silu"):
    """gu[M, 2 I] = x @ Wgu^T (Wgu interleaved, see interleave_gate_up) and m[M, I] = act(g) (*) u: the GEMM / skinny / small-M forward +
    lrp_gated_act_fwd_il (small M, fp32; M = B S rows in bf16 take gemm_gated_fwd_coef)"""
    same(x, Wgu, gu, m)
    linear_fwd(x, Wgu, out=gu)
    gated_act_fwd_il(gu, m, act)
    return gu, m


def gemm_gated_bwd(Adn, Wd, gu, Agu, eps_g, eps_lin, act="silu"):
    """Agu[M, 2 I] (interleaved) from A_dn[M, H], the stored down weight Wd [H, I] and the stored gate/up output: ops.linear_dgrad +
    lrp_gated_act_bwd_il"""
    same(Adn, Wd, gu, Agu)
    Gm = linear_dgrad(Adn, Wd)
    return gated_act_bwd_il(Gm, gu, Agu, eps_g, eps_lin, act)


def rope_fwd(x, out, cos, sin, seq, n_heads, d):
    """x/out: [rows, >= n_heads*d] 2-D views (row stride = stride(0)); cos/sin fp32 [seq, d]"""
    rows = x.shape[0]
    same(x, out)
    f32(cos, sin)
    _rope_tables(cos, sin, seq, d, "lrp_rope_fwd")
    _pitched("lrp_rope_fwd", rows, n_heads * d, x=x, out=out)
    check(lib.lrp_rope_fwd(p(x), p(out), p(cos), p(sin), rows, seq, n_heads, d, x.stride(0), out.stride(0), dt(x), stream()),
          "lrp_rope_fwd")
    return out


def rope_bwd(Gr, xr, x, A, cos, sin, seq, n_heads, d, eps_rope, eps_lin):
    rows = Gr.shape[0]
    same(Gr, xr, x, A)
    f32(cos, sin)
    _rope_tables(cos, sin, seq, d, "lrp_rope_bwd")
    _pitched("lrp_rope_bwd", rows, n_heads * d, Gr=Gr, xr=xr, x=x, A=A)
    check(lib.lrp_rope_bwd(p(Gr), p(xr), p(x), p(A), p(cos), p(sin), rows, seq, n_heads, d, Gr.stride(0),
                           xr.stride(0) if xr is not None else 0, x.stride(0) if x is not None else 0, A.stride(0),
                           eps_rope, eps_lin, dt(Gr), stream()), "lrp_rope_bwd")
    return A


# ---------------------------------------------------------------------------------------- row ops
# ---- K1n: RMSNorm folded into the GEMMs around it (include/lrp_hip.h; ref lxt/efficient/patches.py:111-123 + the residual sums of HF modeling_llama)
# module attribute: True (default) = every part; False = the stand-alone add_rmsnorm_fwd / rmsnorm_bwd_add2 launches (A/B measurements, equality
# tests); a set of {"fwd", "bwd_qkv", "bwd_gu"} = the named parts.  In situ, 8-layer judged step (tools/r5_k1n_parts.sh, final kernel, three
# interleaved repeats): all parts 43.58-43.67 ms, without the gate/up dgrad's residual epilogue 43.62-43.78, none 44.15-44.34 (+1.5 %).  (The first
# version of the residual epilogue -- two row blocks in flight, loads requested at the start of the epilogue -- LOST on the gate/up dgrad: 1312 us
# against 1258 + 31.)
NORM_FUSION = True


def norm_fusion_part(part):
    return NORM_FUSION is True or (isinstance(NORM_FUSION, (set, frozenset)) and part in NORM_FUSION)


def norm_fused_ok(M, N, K, lda, ldb, nn, dtype):
    """the K1n entry points take this problem (bf16, N % 256 == 0, K % 64 == 0, >= 190 output tiles of the ping-pong kernel)"""
    return bool(NORM_FUSION and dtype == torch.bfloat16 and lib.lrp_gemm_norm_fused_ok(M, N, K, lda, ldb, 1 if nn else 0, _DT[dtype]))


_CONST_ROWS = {}


def const_rows(M, value, device):
    """cached fp32 [M] vector of one value (row scales of the K1n entry points: 1/2 for the o-projection's dgrad)"""
    key = (str(device), M, float(value))
    t = _CONST_ROWS.get(key)
    if t is None:
        if len(_CONST_ROWS) > 16:
            _CONST_ROWS.clear()
        t = _CONST_ROWS[key] = torch.full((M,), float(value), device=device, dtype=torch.float32)
    return t


def gemm_res_ssq(x, W, res, out, ssq, raw=None):
    """out = res + x @ W^T (bf16 rounding once) and ssq[p, m] = sum of out[m, 64 p : 64 p + 64]^2 -- the residual add and RMSNorm's sum of
    squares in the producing GEMM's epilogue; ssq [N / 64, >= M] fp32"""
    M, K = x.shape
    N = W.shape[0]
    same(x, W, res, out)
    f32(ssq)
    assert ssq.shape[0] * 64 == N and ssq.stride(0) >= M and ssq.stride(1) == 1
    if raw is not None:      # the explicit placement keeps the Linear's own output too (its stabiliser divides by it)
        same(x, raw)
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_res_ssq(p(x), p(W), p(res), p(out), p(ssq), M, N, K, x.stride(0), W.stride(0),
                                                                       res.stride(0), out.stride(0), ssq.stride(0), p(raw),
                                                                       raw.stride(0) if raw is not None else 0, dt(x), stream()), "lrp_gemm_res_ssq")
    return out


def rms_rstd(ssq, M, H, eps, rstd):
    f32(ssq, rstd)
    check(lib.lrp_rms_rstd(p(ssq), ssq.shape[0], ssq.stride(0), M, H, eps, p(rstd), stream()), "lrp_rms_rstd")
    return rstd


def gemm_nt_rs(x, W, rs, out):
    """out = rs[:, None] * (x @ W^T): the consumer of a folded RMSNorm (W carries the norm's weight, rs = rstd of x's rows)"""
    M, K = x.shape
    N = W.shape[0]
    same(x, W, out)
    f32(rs)
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_nt_rs(p(x), p(W), p(rs), p(out), M, N, K, x.stride(0), W.stride(0), out.stride(0),
                                                                     dt(x), stream()), "lrp_gemm_nt_rs")
    return out


ROPE_FWD_FUSION = True   # module attribute (A/B): False = lrp_gemm_nt_rs + the stand-alone lrp_rope_fwd pass


def gemm_nt_rs_rope_ok(x, W, out, seq, rope_cols, head_dim):
    M, K = x.shape
    return bool(ROPE_FWD_FUSION and NORM_FUSION and x.dtype == torch.bfloat16 and
                lib.lrp_gemm_nt_rs_rope_ok(M, W.shape[0], K, x.stride(0), W.stride(0), out.stride(0), seq, rope_cols, head_dim, _DT[x.dtype]))


def gemm_nt_rs_rope(x, W, rs, cos, sin, out, seq, rope_cols, head_dim):
    """out = rs[:, None] * (x @ W^T) with RoPE applied to the head columns [0, rope_cols) in the GEMM's epilogue (the fused QKV forward: q and k
    leave the kernel rotated, v untouched); cos / sin fp32 [>= seq, head_dim], position of row m = m % seq"""
    M, K = x.shape
    N = W.shape[0]
    same(x, W, out)
    f32(rs, cos, sin)
    assert cos.shape[0] >= seq and cos.stride(0) == head_dim and sin.stride(0) == head_dim
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_nt_rs_rope(p(x), p(W), p(rs), p(cos), p(sin), p(out), M, N, K, x.stride(0), W.stride(0),
                                                                          out.stride(0), seq, rope_cols, head_dim, dt(x), stream()), "lrp_gemm_nt_rs_rope")
    return out


def gemm_nt_rs_bias(x, W, rs, bias, out):
    """out = rs[:, None] * (x @ W^T) + bias: gemm_nt_rs for a biased projection (Qwen2's q / k / v; the folded norm weight is in W, not in bias)"""
    M, K = x.shape
    N = W.shape[0]
    same(x, W, out, bias)
    f32(rs)
    assert bias.shape == (N,) and bias.is_contiguous()
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_nt_rs_bias(p(x), p(W), p(rs), p(bias), p(out), M, N, K, x.stride(0), W.stride(0),
                                                                          out.stride(0), dt(x), stream()), "lrp_gemm_nt_rs_bias")
    return out


def gemm_nt_rs_bias_rope_ok(x, W, out, seq, rope_cols, head_dim):
    M, K = x.shape
    return bool(ROPE_FWD_FUSION and NORM_FUSION and x.dtype == torch.bfloat16 and
                lib.lrp_gemm_nt_rs_bias_rope_ok(M, W.shape[0], K, x.stride(0), W.stride(0), out.stride(0), seq, rope_cols, head_dim, _DT[x.dtype]))


def gemm_nt_rs_bias_rope(x, W, rs, bias, cos, sin, out, seq, rope_cols, head_dim):
    """gemm_nt_rs_rope with bias [N] added ahead of the rotation: RoPE(rs (x W^T) + bias) on the columns [0, rope_cols), rs (x W^T) + bias on
    the rest, one rounding (the fused QKV forward of a Qwen2 layer); rope_cols a multiple of 256"""
    M, K = x.shape
    N = W.shape[0]
    same(x, W, out, bias)
    f32(rs, cos, sin)
    assert bias.shape == (N,) and bias.is_contiguous()
    assert cos.shape[0] >= seq and cos.stride(0) == head_dim and sin.stride(0) == head_dim
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_nt_rs_bias_rope(p(x), p(W), p(rs), p(bias), p(cos), p(sin), p(out), M, N, K, x.stride(0),
                                                                               W.stride(0), out.stride(0), seq, rope_cols, head_dim, dt(x),
                                                                               stream()), "lrp_gemm_nt_rs_bias_rope")
    return out


def gemm_nn_rs(s, W, rs, out):
    """out = rs[:, None] * (s @ W) from the STORED weight W [K, N] (rs = 1/2: the o-projection's dgrad with the uniform rule's factor)"""
    M, K = s.shape
    N = W.shape[1]
    same(s, W, out)
    f32(rs)
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_nn_rs(p(s), p(W), p(rs), p(out), M, N, K, s.stride(0), W.stride(0), out.stride(0),
                                                                     dt(s), stream()), "lrp_gemm_nn_rs")
    return out


def gemm_nn_rs_res(s, W, rs, res, out):
    """out = rs[:, None] * (s @ W) + res from the STORED weight W [K, N]: RMSNorm's identity-rule backward (row scale; the norm's weight sits in
    W) and the residual gradient in the dgrad GEMM's epilogue; out may alias res"""
    M, K = s.shape
    N = W.shape[1]
    same(s, W, res, out)
    f32(rs)
    _timed(2.0 * M * N * K, "plain_norm", lambda: lib.lrp_gemm_nn_rs_res(p(s), p(W), p(rs), p(res), p(out), M, N, K, s.stride(0), W.stride(0),
                                                                         res.stride(0), out.stride(0), dt(s), stream()), "lrp_gemm_nn_rs_res")
    return out


def add_rmsnorm_fwd(h, branch, w, eps, w_offset=0.0, hsum_out=None, y=None, rstd=None, norm_out=True):
    """norm_out=False: only the residual sum (hsum_out) and rstd are written, no normalised rows -> (None, rstd)"""
    M, H = h.shape
    y = (torch.empty_like(h) if y is None else y) if norm_out else None
    rstd = torch.empty(M, device=h.device, dtype=torch.float32) if rstd is None else rstd
    same(h, branch, hsum_out, y)
    f32(rstd)
    _rows_contiguous("lrp_add_rmsnorm_fwd", M, H, h=h, branch=branch, hsum_out=hsum_out, y=y)
    _row_stats("lrp_add_rmsnorm_fwd", M, rstd=rstd)
    w = aux(w, h, H)
    check(lib.lrp_add_rmsnorm_fwd(p(h), p(branch), p(w), p(hsum_out), p(y), p(rstd), M, H, eps, w_offset, dt(h), stream()),
          "lrp_add_rmsnorm_fwd")
    return y, rstd


def rmsnorm_bwd_add2(Gres, Gx, w, rstd, hsum, branch, Gs_out, A_out, rel_out=None, w_offset=0.0, eps_add=0.0, eps_lin=0.0):
    M, H = (Gx if Gx is not None else Gres).shape
    same(Gs_out, Gres, Gx, hsum, branch, A_out)
    f32(rstd, rel_out)
    _rows_contiguous("lrp_rmsnorm_bwd_add2", M, H, Gres=Gres, Gx=Gx, hsum=hsum, branch=branch, Gs_out=Gs_out, A_out=A_out)
    _row_stats("lrp_rmsnorm_bwd_add2", M, rstd=rstd, rel_out=rel_out)
    w = aux(w, Gs_out, H)
    check(lib.lrp_rmsnorm_bwd_add2(p(Gres), p(Gx), p(w), p(rstd), p(hsum), p(branch), p(Gs_out), p(A_out), p(rel_out), M, H,
                                   w_offset, eps_add, eps_lin, dt(Gs_out), stream()), "lrp_rmsnorm_bwd_add2")
    return Gs_out, A_out


def head_rmsnorm_fwd(x, w, y, rstd, heads, d, eps, w_offset=0.0):
    """per-head RMSNorm of the first heads*d columns of x [rows, >= heads*d] (2-D views: row pitch = stride(0)) into y; rstd fp32 [rows*heads]"""
    rows = x.shape[0]
    same(x, y)
    f32(rstd)
    w = aux(w, x, d)
    check(lib.lrp_head_rmsnorm_fwd(p(x), p(w), p(y), p(rstd), rows, heads, d, x.stride(0), y.stride(0), eps, w_offset, dt(x), stream()),
          "lrp_head_rmsnorm_fwd")
    return y, rstd


def head_rmsnorm_bwd(G, w, rstd, out, heads, d, w_offset=0.0):
    """out = G (*) (w + w_offset) * rstd per (row, head): the backward of head_rmsnorm_fwd with rstd detached"""
    rows = G.shape[0]
    same(G, out)
    f32(rstd)
    w = aux(w, G, d)
    check(lib.lrp_head_rmsnorm_bwd(p(G), p(w), p(rstd), p(out), rows, heads, d, G.stride(0), out.stride(0), w_offset, dt(G), stream()),
          "lrp_head_rmsnorm_bwd")
    return out


SITE_FUSION = True      # module attribute (A/B measurements, tests): False keeps Gemma-3's norms / q-k norm / RoPE on the per-module launch sequences


def _sandwich_rows_ok(x):
    return bool(x.dtype in _DT and x.dim() == 2 and x.is_contiguous() and lib.lrp_sandwich_norm_ok(x.shape[1], dt(x)))


def sandwich_norm_ok(x):
    """can lrp_sandwich_norm_fwd / _bwd take rows of this width and dtype (the row stays in one workgroup's registers)?"""
    return bool(SITE_FUSION and _sandwich_rows_ok(x))


def _rope_tables(cos, sin, seq, d, name):
    """the site kernels index the tables as [row % seq][d] with a row pitch of d (no count, no pitch in the C ABI): a table shorter than seq or a
    strided view would be read out of bounds"""
    for t in (cos, sin):
        if t.dim() != 2 or t.shape[0] < seq or t.shape[1] != d or t.stride(0) != d or t.stride(1) != 1:
            raise ValueError(f"{name}: cos / sin must be [>= seq = {seq}, d = {d}] with row stride d, got {tuple(t.shape)} with strides {t.stride()}")


def sandwich_norm_fwd(x, res, w_post, w_pre, eps, w_offset, hsum_out, y, rstd_post, rstd_pre):
    """hsum_out = res + norm_post(x), y = norm_pre(hsum_out) in one pass (Gemma-3's post-norm / residual add / next pre-norm; y, w_pre may be
    None): bit-identical to add_rmsnorm_fwd(x, None, w_post) followed by add_rmsnorm_fwd(res, branch, w_pre, hsum_out=...)"""
    M, H = x.shape
    same(x, res, hsum_out, y)
    f32(rstd_post, rstd_pre)
    _rows_contiguous("lrp_sandwich_norm_fwd", M, H, x=x, res=res, hsum_out=hsum_out, y=y)
    _row_stats("lrp_sandwich_norm_fwd", M, rstd_post=rstd_post, rstd_pre=rstd_pre)
    w_post = aux(w_post, x, H)
    w_pre = aux(w_pre, x, H) if w_pre is not None else None
    check(lib.lrp_sandwich_norm_fwd(p(x), p(res), p(w_post), p(w_pre), p(hsum_out), p(y), p(rstd_post), p(rstd_pre), M, H, eps, w_offset, dt(x),
                                    stream()), "lrp_sandwich_norm_fwd")
    return hsum_out, y


def sandwich_norm_bwd(Gres, Gx, w_pre, rstd_pre, w_post, rstd_post, Gs_out, Ga_out, w_offset=0.0):
    """Gs_out = Gres + Gx w_pre' rstd_pre (Gres may be None), Ga_out = Gs_out w_post' rstd_post: the backward of sandwich_norm_fwd's site with both
    rstd detached = two rmsnorm_bwd_add2 launches"""
    M, H = Gx.shape
    same(Gx, Gres, Gs_out, Ga_out)
    f32(rstd_pre, rstd_post)
    for t in (Gx, Gres, Gs_out, Ga_out):          # (no row pitch in the C ABI: [M, H] contiguous, rows of a width the forward's gate takes)
        if t is not None and (tuple(t.shape) != (M, H) or not _sandwich_rows_ok(t)):
            raise ValueError(f"lrp_sandwich_norm_bwd: operands must be contiguous [{M}, {H}] rows that sandwich_norm_ok accepts, got "
                             f"{tuple(t.shape)} with strides {t.stride()}")
    check(lib.lrp_sandwich_norm_bwd(p(Gres), p(Gx), p(aux(w_pre, Gx, H)), p(rstd_pre), p(aux(w_post, Gx, H)), p(rstd_post), p(Gs_out), p(Ga_out), M, H,
                                    w_offset, dt(Gx), stream()), "lrp_sandwich_norm_bwd")
    return Gs_out, Ga_out


def qk_norm_rope_fwd(qkv, wq, wk, qr, kr, rstd_q, rstd_k, cos_t, sin_t, seq, nq, nk, d, eps, w_offset=0.0):
    """per-head q / k RMSNorm + RoPE straight out of the fused projection output qkv [rows, >= (nq + nk) d] into qr [rows, nq d], kr [rows, nk d]
    (= 2 x head_rmsnorm_fwd + 2 x rope_fwd, bit-identical)"""
    rows = qkv.shape[0]
    same(qkv, qr, kr)
    f32(rstd_q, rstd_k, cos_t, sin_t)
    _rope_tables(cos_t, sin_t, seq, d, "lrp_qk_norm_rope_fwd")
    check(lib.lrp_qk_norm_rope_fwd(p(qkv), p(aux(wq, qkv, d)), p(aux(wk, qkv, d)), p(qr), p(kr), p(rstd_q), p(rstd_k), p(cos_t), p(sin_t), rows, seq,
                                   nq, nk, d, qkv.stride(0), qr.stride(0), kr.stride(0), eps, w_offset, dt(qkv), stream()), "lrp_qk_norm_rope_fwd")
    return qr, kr


def qkv_bwd_pack(dq, dk_h, dv_h, wq, wk, rstd_q, rstd_k, cos_t, sin_t, A, seq, nq, nk, d, w_offset=0.0):
    """A [rows, (nq + 2 nk) d] = [rope^T(dq) wq' rstd_q | rope^T(group sum of dk_h) wk' rstd_k | group sum of dv_h]: the qkv dgrad's operand in one
    pass (= 2 x gqa_reduce + 2 x rope_bwd + 2 x head_rmsnorm_bwd, bit-identical)"""
    rows = dq.shape[0]
    same(dq, dk_h, dv_h, A)
    f32(rstd_q, rstd_k, cos_t, sin_t)
    _rope_tables(cos_t, sin_t, seq, d, "lrp_qkv_bwd_pack")
    check(lib.lrp_qkv_bwd_pack(p(dq), p(dk_h), p(dv_h), p(aux(wq, dq, d)), p(aux(wk, dq, d)), p(rstd_q), p(rstd_k), p(cos_t), p(sin_t), p(A), rows, seq,
                               nq, nk, d, dq.stride(0), dk_h.stride(0), dv_h.stride(0), A.stride(0), w_offset, dt(dq), stream()), "lrp_qkv_bwd_pack")
    return A


def head_norm_bwd(g_xn, w, rstd, out, w_offset=0.0):
    """final-norm identity rule on the head rows: out = g_xn * (w + w_offset) * rstd  (g_xn fp32 or model dtype [B,H])"""
    g = g_xn if g_xn.dtype == out.dtype else cast(g_xn, out.dtype)
    rmsnorm_bwd_add2(None, g, w, rstd, None, None, out, None, None, w_offset, 0.0, 0.0)
    return out


def layernorm_fwd(x, w, b, eps):
    x = _c(x)
    H = x.shape[-1]
    M = x.numel() // H
    y = torch.empty_like(x)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    w, b = aux(w, x, H), aux(b, x, H)
    check(lib.lrp_layernorm_fwd(p(x), p(w), p(b), p(y), p(mean), p(rstd), M, H, eps, dt(x), stream()), "lrp_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(Gy, y, w, rstd, eps_y=0.0):
    Gy = _c(Gy)
    H = Gy.shape[-1]
    M = Gy.numel() // H
    Gx = torch.empty_like(Gy)
    same(Gy, y)
    f32(rstd)
    w = aux(w, Gy, H)
    check(lib.lrp_layernorm_bwd(p(Gy), p(y), p(w), p(rstd), p(Gx), M, H, eps_y, dt(Gy), stream()), "lrp_layernorm_bwd")
    return Gx


def layernorm_bwd_plain(Gy, x, w, mean, rstd, out=None):
    """full LayerNorm VJP (no rule; mean and 1/std differentiated) from the forward's x / mean / rstd"""
    Gy, x = _c(Gy), _c(x)
    H = Gy.shape[-1]
    M = Gy.numel() // H
    out = torch.empty_like(Gy) if out is None else out
    same(Gy, x, out)
    f32(mean, rstd)
    w = aux(w, Gy, H)
    check(lib.lrp_layernorm_bwd_plain(p(Gy), p(x), p(w), p(mean), p(rstd), p(out), M, H, dt(Gy), stream()), "lrp_layernorm_bwd_plain")
    return out


def softmax_fwd(x, inv_temp=1.0):
    x = _c(x)
    n = x.shape[-1]
    out = torch.empty_like(x)
    check(lib.lrp_softmax_fwd(p(x), p(out), x.numel() // n, n, inv_temp, dt(x), stream()), "lrp_softmax_fwd")
    return out


def softmax_rule_bwd(x, pr, Rp, inv_temp=1.0):
    x, pr, Rp = _c(x), _c(pr), _c(Rp)
    n = x.shape[-1]
    Rx = torch.empty_like(x)
    same(x, pr, Rp)
    check(lib.lrp_softmax_rule_bwd(p(x), p(pr), p(Rp), p(Rx), x.numel() // n, n, inv_temp, dt(x), stream()),
          "lrp_softmax_rule_bwd")
    return Rx


def readout(emb, G, out=None):
    M, H = emb.shape
    out = torch.empty(M, device=emb.device, dtype=torch.float32) if out is None else out
    same(emb, G)
    f32(out)
    check(lib.lrp_readout(p(emb), p(G), p(out), M, H, dt(emb), stream()), "lrp_readout")
    return out


def colsum_dot(x, g, B, S, out=None, ws=None):
    """out[b, j] = sum_t x[b S + t, j] g[b S + t, j]  ([B, N] fp32) for x, g [B S, N] with unit column stride (any row pitch): the token-summed
    relevance of every hidden unit (x = h, g = G_h; x = m, g = G_m).  Fixed-order fp32 sums, a prompt's result depends on its rows only.
    ws: the caller's workspace (uint8, at least lrp_colsum_dot_ws bytes); None: the per-stream scratch buffer"""
    M, N = x.shape
    if tuple(g.shape) != (M, N) or x.stride(1) != 1 or g.stride(1) != 1:
        raise ValueError(f"colsum_dot: x {tuple(x.shape)} and g {tuple(g.shape)} must be the same [B S, N] shape with contiguous rows")
    px, pg = p(x), p(g)                 # (device tensors only: raises before anything is allocated)
    out = torch.empty(B, N, device=x.device, dtype=torch.float32) if out is None else out
    same(x, g)
    f32(out)
    if tuple(out.shape) != (B, N) or not out.is_contiguous():
        raise ValueError(f"colsum_dot: out must be a contiguous [{B}, {N}] tensor")
    need = lib.lrp_colsum_dot_ws(B, S, N)
    if need < 0:
        raise ValueError(f"colsum_dot: bad sizes B={B}, S={S}, N={N}")
    if need and ws is None:
        ws = workspace(need, x)
    elif need and ws.numel() * ws.element_size() < need:
        raise ValueError(f"colsum_dot: workspace of {ws.numel() * ws.element_size()} bytes, {need} needed")
    check(lib.lrp_colsum_dot(px, pg, p(out), p(ws) if need else None, M, N, B, S, x.stride(0), g.stride(0), dt(x), stream()),
          "lrp_colsum_dot")
    return out


def headdot(x, g, B, S, nh, rep, d, scale=1.0, rope=None, out=None):
    """out[b, h, t] = scale sum_j x[b S + t, (h // rep) d + j] g'[b S + t, h d + j]  ([B, nh, S] fp32): the relevance of every attention head at
    every position.  x [B S, (nh // rep) d] and g [B S, nh d] token-major with unit column stride (any row pitch); rope = (cos, sin) fp32
    [>= S, d]: g' = the forward rotate-half RoPE of g at position t (the fused dQ kernel's RoPE^T(dq) against the rotated q), else g' = g.
    Fixed-order fp32 sums, a prompt's result depends on its rows only."""
    M = x.shape[0]
    if (x.dim() != 2 or g.dim() != 2 or g.shape[0] != M or x.shape[1] != (nh // max(rep, 1)) * d or g.shape[1] != nh * d
            or x.stride(1) != 1 or g.stride(1) != 1):
        raise ValueError(f"headdot: x {tuple(x.shape)} / g {tuple(g.shape)} must be [B S, {nh} // {rep} * {d}] / [B S, {nh} * {d}] with contiguous rows")
    px, pg = p(x), p(g)                 # (device tensors only: raises before anything is allocated)
    out = torch.empty(B, nh, S, device=x.device, dtype=torch.float32) if out is None else out
    same(x, g)
    f32(out)
    if tuple(out.shape) != (B, nh, S) or not out.is_contiguous():
        raise ValueError(f"headdot: out must be a contiguous [{B}, {nh}, {S}] tensor")
    pc = ps = None
    if rope is not None:
        cos, sin = rope
        f32(cos, sin)
        assert cos.shape[0] >= S and sin.shape[0] >= S and cos.stride(0) == d and sin.stride(0) == d
        pc, ps = p(cos), p(sin)
    check(lib.lrp_headdot(px, pg, pc, ps, p(out), M, B, S, nh, rep, d, x.stride(0), g.stride(0), float(scale), dt(x), stream()), "lrp_headdot")
    return out


def attn_relmap(q, k, v, g, lse, B, S, Hq, Hkv, d, scale, heads=None, gscale=1.0, causal=True, row_iv=None, out=None):
    """out[b, i, j] = gscale sum_{lo <= h < hi} P_h[i, j] (g_h[i] . v_{h // rep}[j])  ([B, S, S] fp32, every element written): the token-to-token
    attention relevance `attn_weights * attn_weights.grad`, summed over the query heads heads = (lo, hi) (None: all of them).  q, g [B S, Hq d]
    and k, v [B S, Hkv d] token-major with unit column stride (any row pitch), lse [B, Hq, S] as attn_fwd left it; g is the gradient at the o
    projection's input (gscale = 2 for the dgrad epilogue's Gho).  bf16: d in {64, 128} (lrp_attn_relmap) and d = 256 (lrp_attn_relmap_d256:
    K / V staged in two 128-column panels, Gemma-3's head dim); fp32: any d <= 256 that is a multiple of 4.
    Masked (i, j) -- causal, row_iv -- are exactly 0.  Fixed-order fp32 sums, a prompt's result depends on its rows only."""
    lo, hi = (0, Hq) if heads is None else (int(heads[0]), int(heads[1]))
    M = q.shape[0]
    for name, t, nh in (("q", q, Hq), ("k", k, Hkv), ("v", v, Hkv), ("g", g, Hq)):
        if t.dim() != 2 or t.shape[0] != M or t.shape[1] != nh * d or t.stride(1) != 1:
            raise ValueError(f"attn_relmap: {name} {tuple(t.shape)} must be [B S = {M}, {nh} * {d}] with contiguous rows")
    if M != B * S or tuple(lse.shape) != (B, Hq, S) or not lse.is_contiguous():
        raise ValueError(f"attn_relmap: {M} rows / lse {tuple(lse.shape)} where B S = {B * S} rows and a contiguous [{B}, {Hq}, {S}] lse are expected")
    pq, pk, pv, pg, pl = p(q), p(k), p(v), p(g), p(lse)                 # (device tensors only: raises before anything is allocated)
    out = torch.empty(B, S, S, device=q.device, dtype=torch.float32) if out is None else out
    same(q, k, v, g)
    f32(lse, out)
    if tuple(out.shape) != (B, S, S) or not out.is_contiguous():
        raise ValueError(f"attn_relmap: out must be a contiguous [{B}, {S}, {S}] tensor")
    name = "lrp_attn_relmap_d256" if q.dtype == torch.bfloat16 and d == 256 else "lrp_attn_relmap"
    check(getattr(lib, name)(pq, pk, pv, pg, pl, p(out), M, B, S, Hq, Hkv, d, lo, hi, q.stride(0), k.stride(0), v.stride(0), g.stride(0),
                             float(scale), float(gscale), int(causal), *_iv(row_iv, B, S), dt(q), stream()), name)
    return out


_ROW_MAPS = {}           # (I, device) -> gate_up_row_map


def gate_up_row_map(I, device):
    """int32 [2 I]: the HF row (gate_proj rows, then up_proj rows) of every STORED row of a fused gate/up weight -- the inverse of
    interleave_gate_up's placement; one tensor per (I, device)"""
    if I % GATED_IL:
        raise ValueError(f"intermediate size {I} is not a multiple of {GATED_IL}")
    key = (I, torch.device(device))
    m = _ROW_MAPS.get(key)
    if m is None:
        s = torch.arange(2 * I, dtype=torch.int64)
        hf = ((s // GATED_IL) % 2) * I + (s // (2 * GATED_IL)) * GATED_IL + s % GATED_IL
        m = _ROW_MAPS[key] = hf.to(device=device, dtype=torch.int32).contiguous()
    return m


def wgrad_rel_ok(M, N, K, ldg, ldx, ldw, ldo, dtype):
    """lrp_wgrad_rel serves this problem (sizes, row pitches in elements, torch dtype)"""
    return dtype in _DT and lib.lrp_wgrad_rel_ok(M, N, K, ldg, ldx, ldw, ldo, _DT[dtype]) == 1


def wgrad_rel(G, X, W, out=None, rs=None, row_map=None, accumulate=False, check_map=True):
    """out[r(n), k] (+)= W[n, k] sum_t G[t, n] rs[t] X[t, k]  ([N, K] fp32): the per-weight relevance `weight * weight.grad` of the Linear
    y = x W^T with output gradient G [M, N] and input X [M, K] (token-major, unit column stride, any row pitch), W [N, K] as stored (any row
    pitch); rs [M] fp32: the 1 / rms of the norm in front of the Linear when X is the un-normed stream; row_map [N] int32: the row of out
    that weight row n lands in (a permutation of [0, N): gate_up_row_map); accumulate: add to out (which then must be given) instead of
    overwriting it; check_map: read the map back and refuse one that is no permutation (one host sync; the kernel stores through it -- the engine
    turns it off for gate_up_row_map's own maps).  bf16: N and K multiples of 8, rs folded into G (one extra bf16 rounding); fp32: any size.  No atomics: bitwise repeatable."""
    if G.dim() != 2 or X.dim() != 2 or W.dim() != 2:
        raise ValueError(f"wgrad_rel: G {tuple(G.shape)}, X {tuple(X.shape)}, W {tuple(W.shape)} must be matrices")
    (M, N), K = G.shape, X.shape[1]
    if X.shape[0] != M or tuple(W.shape) != (N, K) or G.stride(1) != 1 or X.stride(1) != 1 or W.stride(1) != 1:
        raise ValueError(f"wgrad_rel: G {tuple(G.shape)} / X {tuple(X.shape)} / W {tuple(W.shape)} must be [M, N] / [M, K] / [N, K] with contiguous rows")
    pg, px, pw = p(G), p(X), p(W)                 # (device tensors only: raises before anything is allocated)
    same(G, X, W)
    if out is None:
        if accumulate:
            raise ValueError("wgrad_rel: accumulate=True needs the out tensor to add to")
        out = torch.empty(N, K, device=G.device, dtype=torch.float32)
    f32(out, rs)
    if tuple(out.shape) != (N, K) or out.stride(1) != 1 or out.device != G.device:
        raise ValueError(f"wgrad_rel: out must be a [{N}, {K}] float32 tensor with contiguous rows on {G.device}, got {tuple(out.shape)} on {out.device}")
    if rs is not None and (tuple(rs.shape) != (M,) or not rs.is_contiguous() or rs.device != G.device):
        raise ValueError(f"wgrad_rel: rs must be a contiguous [{M}] tensor on {G.device}")
    if row_map is not None:
        if row_map.dtype != torch.int32 or tuple(row_map.shape) != (N,) or not row_map.is_contiguous() or row_map.device != G.device:
            raise ValueError(f"wgrad_rel: row_map must be a contiguous int32 [{N}] tensor on {G.device}")
        if check_map and not torch.equal(torch.sort(row_map.long()).values, torch.arange(N, device=row_map.device)):
            raise ValueError(f"wgrad_rel: row_map is not a permutation of [0, {N})")
    check(lib.lrp_wgrad_rel(pg, px, pw, p(out), p(rs), p(row_map), M, N, K, G.stride(0), X.stride(0), W.stride(0), out.stride(0),
                            int(bool(accumulate)), dt(G), stream()), "lrp_wgrad_rel")
    return out


def wgrad_ok(M, N, K, ldg, ldx, ldo, dtype):
    """lrp_wgrad serves this problem (sizes, row pitches in elements, torch dtype)"""
    return dtype in _DT and lib.lrp_wgrad_ok(M, N, K, ldg, ldx, ldo, _DT[dtype]) == 1


def wgrad(G, X, out=None):
    """out[n, k] = sum_t G[t, n] X[t, k]  ([N, K], the operands' dtype): the plain `weight.grad` of the Linear y = x W^T with output gradient
    G [M, N] and input X [M, K] (token-major, unit column stride, any row pitch).  A weight stored [in, out] (HF's Conv1D): wgrad(X, G).
    bf16: N and K multiples of 8, wgrad_rel's token loop and ONE round-to-nearest-even of its fp32 accumulator; fp32: any size, fp64 token sum.
    No atomics: bitwise repeatable."""
    if G.dim() != 2 or X.dim() != 2:
        raise ValueError(f"wgrad: G {tuple(G.shape)} and X {tuple(X.shape)} must be matrices")
    (M, N), K = G.shape, X.shape[1]
    if X.shape[0] != M or G.stride(1) != 1 or X.stride(1) != 1:
        raise ValueError(f"wgrad: G {tuple(G.shape)} / X {tuple(X.shape)} must be [M, N] / [M, K] with contiguous rows")
    pg, px = p(G), p(X)                 # (device tensors only: raises before anything is allocated)
    same(G, X)
    dt(G)
    if out is None:
        out = torch.empty(N, K, device=G.device, dtype=G.dtype)
    same(G, out)
    if tuple(out.shape) != (N, K) or out.stride(1) != 1:
        raise ValueError(f"wgrad: out must be a [{N}, {K}] tensor with contiguous rows, got {tuple(out.shape)}")
    check(lib.lrp_wgrad(pg, px, p(out), M, N, K, G.stride(0), X.stride(0), out.stride(0), dt(G), stream()), "lrp_wgrad")
    return out


def colsum_affine(g, x=None, mean=None, rstd=None, want_bias=False, ws=None):
    """-> (dw, db), fp32 [N] each or None:  dw[j] = sum_t g[t, j] (x[t, j] - mean[t]) rstd[t]  (when x is given),  db[j] = sum_t g[t, j]  (when
    want_bias) for g, x [M, N] with unit column stride (any row pitch), mean / rstd fp32 [M] or None (0 / 1): the weight gradient of an
    RMSNorm, a (1 + w) norm or a per-head norm (mean None), the weight and bias gradients of a LayerNorm, the bias gradient of a Linear
    (x None).  Fixed-order fp32 sums over 64-row chunks, no atomics: bitwise repeatable.
    ws: the caller's workspace (uint8, at least lrp_colsum_affine_ws bytes); None: the per-stream scratch buffer"""
    if g.dim() != 2 or g.stride(1) != 1:
        raise ValueError(f"colsum_affine: g {tuple(g.shape)} must be [M, N] with contiguous rows")
    M, N = g.shape
    if x is None and not want_bias:
        raise ValueError("colsum_affine: nothing to compute (no x and want_bias=False)")
    if x is None and (mean is not None or rstd is not None):
        raise ValueError("colsum_affine: mean / rstd without x")
    if x is not None and (tuple(x.shape) != (M, N) or x.stride(1) != 1):
        raise ValueError(f"colsum_affine: x {tuple(x.shape)} must have g's shape {tuple(g.shape)} and contiguous rows")
    pg, px = p(g), p(x)                 # (device tensors only: raises before anything is allocated)
    same(g, x)
    f32(mean, rstd)
    for name, t in (("mean", mean), ("rstd", rstd)):
        if t is not None and (tuple(t.shape) != (M,) or not t.is_contiguous() or t.device != g.device):
            raise ValueError(f"colsum_affine: {name} must be a contiguous [{M}] tensor on {g.device}")
    need = lib.lrp_colsum_affine_ws(M, N)
    if need < 0:
        raise ValueError(f"colsum_affine: bad sizes M={M}, N={N}")
    dw = torch.empty(N, device=g.device, dtype=torch.float32) if x is not None else None
    db = torch.empty(N, device=g.device, dtype=torch.float32) if want_bias else None
    if need and ws is None:
        ws = workspace(need, g)
    elif need and ws.numel() * ws.element_size() < need:
        raise ValueError(f"colsum_affine: workspace of {ws.numel() * ws.element_size()} bytes, {need} needed")
    check(lib.lrp_colsum_affine(pg, px, p(mean), p(rstd), p(dw), p(db), p(ws) if need else None, M, N, g.stride(0),
                                x.stride(0) if x is not None else 0, dt(g), stream()), "lrp_colsum_affine")
    return dw, db


def argmax_rows(logits):
    B, V = logits.shape
    idx = torch.empty(B, device=logits.device, dtype=torch.int32)
    val = torch.empty(B, device=logits.device, dtype=torch.float32)
    check(lib.lrp_argmax_rows(p(logits), p(idx), p(val), B, V, logits.stride(0), stream()), "lrp_argmax_rows")
    return idx, val


def head_seed(W_lm, logits, idx, w_norm, rstd_last, out, w_offset=0.0, eps_lin=0.0):
    B, V = logits.shape
    H = W_lm.shape[1]
    same(W_lm, out)
    f32(logits, rstd_last)
    w_norm = aux(w_norm, W_lm, H)
    if idx.dtype != torch.int32:
        raise TypeError("head_seed: idx must be int32")
    check(lib.lrp_head_seed(p(W_lm), p(logits), p(idx), p(w_norm), p(rstd_last), p(out), B, V, H, logits.stride(0), w_offset,
                            eps_lin, dt(W_lm), stream()), "lrp_head_seed")
    return out


SPAN_OBJECTIVES = {"logit": 0, "logprob": 1}          # LRP_SPAN_LOGIT / LRP_SPAN_LOGPROB (include/lrp_hip_span.h)


def span_seed(logits, idx, w=None, rstd=None, objective="logit", seed=None, seed_dtype=None, logit=None, logprob=None, rs=None):
    """the head seed of an answer-span explanation, one launch over the R explained rows of fp32 logits [R, V] (unit column stride, any row
    pitch): -> (logit [R] = l[idx] bitwise, logprob [R] = log_softmax(l)[idx], rs = w (*) rstd or None, seed or None).  idx [R] int32 in
    [0, V); w [R] fp32 (None: ones); rstd [R] fp32: rs is formed when it is given.  objective="logprob": seed [R, V] =
    w (delta(j, idx) - softmax(l)_j) in seed_dtype (float32 / bfloat16; or pass the buffer), rounded once; "logit": no dense seed.
    Fixed-order fp32 sums, bitwise repeatable, a row's result depends on that row only."""
    if objective not in SPAN_OBJECTIVES:
        raise ValueError(f"span_seed: objective must be one of {sorted(SPAN_OBJECTIVES)}, got {objective!r}")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError(f"span_seed: logits {tuple(logits.shape)} must be [R, V] with contiguous rows")
    R, V = logits.shape
    pl = p(logits)                      # (device tensors only: raises before anything is allocated)
    f32(logits, w, rstd, logit, logprob, rs)
    if idx.dtype != torch.int32 or idx.numel() != R or not idx.is_contiguous():
        raise TypeError(f"span_seed: idx must be a contiguous int32 [{R}] tensor")
    for name, t in (("w", w), ("rstd", rstd), ("logit", logit), ("logprob", logprob), ("rs", rs)):
        if t is not None and (t.numel() != R or not t.is_contiguous()):
            raise ValueError(f"span_seed: {name} must be a contiguous [{R}] tensor")
    new = lambda: torch.empty(R, device=logits.device, dtype=torch.float32)      # noqa: E731
    logit, logprob = new() if logit is None else logit, new() if logprob is None else logprob
    if rstd is not None and rs is None:
        rs = new()
    ld_seed = sdt = 0
    if objective == "logprob":
        if seed is None:
            seed = torch.empty(R, V, device=logits.device, dtype=seed_dtype or torch.float32)
        if tuple(seed.shape) != (R, V) or seed.stride(1) != 1 or seed.device != logits.device:
            raise ValueError(f"span_seed: seed must be a [{R}, {V}] tensor with contiguous rows on {logits.device}")
        ld_seed, sdt = seed.stride(0) if R > 1 else max(seed.stride(0), V), dt(seed)
    else:
        seed = None
    if R == 0:                          # (empty tensors have no address to hand over)
        return logit, logprob, rs, seed
    check(lib.lrp_span_seed(pl, logits.stride(0) if R > 1 else max(logits.stride(0), V), p(idx), p(w), p(rstd), R, V, SPAN_OBJECTIVES[objective],
                            p(seed), ld_seed, sdt, p(logit), p(logprob), p(rs), stream()), "lrp_span_seed")
    return logit, logprob, rs, seed


def sample_rows(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seeds=None, streams=None, step=0, u=None):
    """one sampled column per row of fp32 logits [B, V] (unit column stride, any row pitch), one launch (include/lrp_hip_sample.h):
    -> (idx int32 [B], sample_logprob fp32 [B] = log(q_idx / Z), n_kept int32 [B], u fp32 [B] = the uniform used).  temperature > 0;
    top_k >= 1 (0 or >= V: off; 1: the arg-max); top_p in (0, 1) (>= 1: off); min_p in (0, 1] (0: off).  The uniform of row b is u[b] when
    u (fp32 [B]) is given, else Philox4x32-10 keyed by seeds[b] (int64 [B]) at counter (step, streams[b] (int32 [B]; None: 0), 0, 0).
    Fixed-point integer masses: bitwise repeatable, a row's result depends on that row only."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < 1:
        raise ValueError(f"sample_rows: logits {tuple(logits.shape)} must be [B, V >= 1] with contiguous rows")
    B, V = logits.shape
    pl = p(logits)                      # (device tensors only: raises before anything is allocated)
    f32(logits, u)
    if seeds is None and u is None:
        raise ValueError("sample_rows: pass seeds (int64 [B]) or u (fp32 [B])")
    for name, t, want in (("seeds", seeds, torch.int64), ("streams", streams, torch.int32), ("u", u, torch.float32)):
        if t is not None:
            if not torch.is_tensor(t) or t.dtype != want:
                raise TypeError(f"sample_rows: {name} must be a {want} tensor")
            if t.numel() != B or not t.is_contiguous() or t.device != logits.device:
                raise ValueError(f"sample_rows: {name} must be a contiguous [{B}] tensor on {logits.device}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0 or isinstance(step, bool) or not isinstance(step, int) or step < 0:
        raise ValueError(f"sample_rows: top_k and step must be integers >= 0, got {top_k!r}, {step!r}")
    temperature, top_p, min_p = float(temperature), float(top_p), float(min_p)
    if not (0.0 < temperature < float("inf")) or not top_p > 0.0 or not 0.0 <= min_p <= 1.0:
        raise ValueError(f"sample_rows: temperature > 0 and finite, top_p > 0, min_p in [0, 1]; got {temperature}, {top_p}, {min_p}")
    idx, n_kept = (torch.empty(B, device=logits.device, dtype=torch.int32) for _ in range(2))
    slp, u_out = (torch.empty(B, device=logits.device, dtype=torch.float32) for _ in range(2))
    if B == 0:                          # (empty tensors have no address to hand over)
        return idx, slp, n_kept, u_out
    check(lib.lrp_sample_rows(pl, logits.stride(0) if B > 1 else max(logits.stride(0), V), B, V, temperature, min(top_k, 2 ** 31 - 1), top_p, min_p,
                              p(seeds), p(streams), step, p(u), p(idx), p(slp), p(n_kept), p(u_out), stream()), "lrp_sample_rows")
    return idx, slp, n_kept, u_out


def _pitch(t, rows, cols):
    return t.stride(0) if rows > 1 else max(t.stride(0), cols)


def token_hist_init(ids, lo, V, hist=None):
    """the history table of one generate() call (include/lrp_hip_penalty.h): ids int64 [B, S] (unit column stride, any row pitch), lo int32 [B]
    or None -> hist int32 [B, V], zeroed, with bit 31 set at ids[b, s] for s >= lo[b] (the columns before lo[b] are the pads of a left-padded
    prompt; an id outside [0, V) is skipped).  hist: a [B, >= V] int32 view with unit column stride to fill (columns >= V are left alone)."""
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.stride(1) != 1 and ids.shape[1] > 1:
        raise ValueError("token_hist_init: ids must be an int64 [B, S] tensor with contiguous rows")
    B, S = ids.shape
    if ids.dtype != torch.int64:
        raise TypeError(f"token_hist_init: ids must be int64, got {ids.dtype}")
    pi = p(ids)                         # (device tensors only: raises before anything is allocated)
    if isinstance(V, bool) or not isinstance(V, int) or V < 1:
        raise ValueError(f"token_hist_init: V must be an integer >= 1, got {V!r}")
    if lo is not None:
        if not torch.is_tensor(lo) or lo.dtype != torch.int32:
            raise TypeError("token_hist_init: lo must be an int32 tensor")
        if lo.numel() != B or not lo.is_contiguous() or lo.device != ids.device:
            raise ValueError(f"token_hist_init: lo must be a contiguous [{B}] tensor on {ids.device}")
    if hist is not None:
        if not torch.is_tensor(hist) or hist.dtype != torch.int32:
            raise TypeError("token_hist_init: hist must be an int32 tensor")
        _pitched("token_hist_init", B, V, hist=hist)
        if hist.device != ids.device:
            raise ValueError(f"token_hist_init: hist must live on {ids.device}")
    else:
        hist = torch.empty(B, V, device=ids.device, dtype=torch.int32)
    if B == 0:                          # (empty tensors have no address to hand over)
        return hist
    check(lib.lrp_token_hist_init(pi, _pitch(ids, B, S), p(lo), B, S, V, p(hist), _pitch(hist, B, V), stream()), "lrp_token_hist_init")
    return hist


def logit_penalty(logits, hist, last=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, bias=None, out=None):
    """the processed logits of one step, one launch (include/lrp_hip_penalty.h): logits fp32 [B, V] (unit column stride, any row pitch), hist
    int32 [B, >= V] as token_hist_init leaves it -> out fp32 [B, V] (a buffer of its own; logits are not written).  last int32 [B] or None:
    the token fed into this step -- its generated count in hist goes up by one first (a value outside [0, V) is ignored).  Then, per column,
    in individually rounded fp32 operations: repetition_penalty (> 0; 1: off) on the columns in the prompt or generated, x < 0 ? x rp : x / rp;
    x - frequency_penalty c, then x - presence_penalty, on the generated ones (count c > 0); x + bias[j] (fp32 [V]; -inf bans a column)."""
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < 1:
        raise ValueError("logit_penalty: logits must be [B, V >= 1] with contiguous rows")
    B, V = logits.shape
    f32(logits, bias, out)
    if not torch.is_tensor(hist) or hist.dtype != torch.int32:
        raise TypeError("logit_penalty: hist must be an int32 tensor")
    pl = p(logits)                      # (device tensors only: raises before anything is allocated)
    _pitched("logit_penalty", B, V, hist=hist, out=out)
    if last is not None:
        if not torch.is_tensor(last) or last.dtype != torch.int32:
            raise TypeError("logit_penalty: last must be an int32 tensor")
        if last.numel() != B or not last.is_contiguous():
            raise ValueError(f"logit_penalty: last must be a contiguous [{B}] tensor")
    if bias is not None and (not torch.is_tensor(bias) or tuple(bias.shape) != (V,) or not bias.is_contiguous()):
        raise ValueError(f"logit_penalty: bias must be a contiguous [{V}] tensor")
    for t in (hist, last, bias, out):
        if t is not None and t.device != logits.device:
            raise ValueError(f"logit_penalty: every operand must live on {logits.device}")
    rp, pp, fp = float(repetition_penalty), float(presence_penalty), float(frequency_penalty)
    if not (0.0 < rp < float("inf")) or not abs(pp) < float("inf") or not abs(fp) < float("inf"):
        raise ValueError(f"logit_penalty: repetition_penalty > 0 and finite, presence / frequency penalty finite; got {rp}, {pp}, {fp}")
    if out is None:
        out = torch.empty(B, V, device=logits.device, dtype=torch.float32)
    elif out.data_ptr() == logits.data_ptr():
        raise ValueError("logit_penalty: out must be a buffer of its own (the raw logits stay what span_seed reads)")
    if B == 0:                          # (empty tensors have no address to hand over)
        return out
    check(lib.lrp_logit_penalty(pl, _pitch(logits, B, V), p(out), _pitch(out, B, V), B, V, p(hist), _pitch(hist, B, V), p(last), rp, pp, fp, p(bias),
                                stream()), "lrp_logit_penalty")
    return out


SMALLM_MAX = 16         # rows the W-streaming small-M kernels serve (above: the skinny split-K path, then the MFMA GEMM)


def _smallm_ws(M, N, K, ref):
    """fp32 scratch of the small-M kernels: the per-(device, stream) workspace (capture-safe, see workspace())"""
    return workspace(4 * lib.lrp_linear_smallm_ws(M, N, K, dt(ref)), ref)


def smallm_ok(M, W, x=None):
    """can the W-streaming small-M kernels serve this call?  (M <= 16 rows, W contiguous [N,K] with K a multiple of 16 bytes,
    16-byte aligned operands -- anything else goes to the GEMM path, which pads)"""
    e = epc(W)
    ok = (0 < M <= SMALLM_MAX and W.dim() == 2 and W.is_contiguous() and W.shape[1] % e == 0 and W.data_ptr() % 16 == 0
          and W.dtype in _DT)
    if ok and x is not None:
        ok = x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % e == 0 and x.data_ptr() % 16 == 0 and x.dtype == W.dtype
    return ok


def linear_smallm_fwd(x, W, bias=None, out=None, out_dtype=None):
    """z [M,N] = x [M,K] @ W[N,K]^T (+ bias), M <= 16, W streamed once (no MFMA tile padding to 128 rows)"""
    M, K = x.shape
    N = W.shape[0]
    same(x, W)
    odt = out_dtype or x.dtype
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=odt)
    check(lib.lrp_linear_smallm_fwd(p(x), p(W), p(aux(bias, x, N)), p(out), p(_smallm_ws(M, N, K, x)), M, N, K, x.stride(0),
                                    out.stride(0), dt(x), _DT[out.dtype], stream()), "lrp_linear_smallm_fwd")
    return out


def linear_smallm_dgrad(g, W, z=None, x=None, eps=0.0, relevance_in=False, relevance_out=False, out=None, out_dtype=None):
    """out [M,K] = s @ W[N,K] (* x) with s = g, g*z/(z+eps) or g/(z+eps): the eps-rule backward of a Linear for M <= 16 rows
    from the STORED weight layout (no W^T copy), W streamed once"""
    M, N = g.shape
    K = W.shape[1]
    same(W, g, z, x)
    odt = out_dtype or W.dtype
    if out is None:
        out = torch.empty(M, K, device=W.device, dtype=odt)
    if x is not None and not x.is_contiguous():
        x = x.contiguous()
    check(lib.lrp_linear_smallm_dgrad(p(g), p(z), p(W), p(x), p(out), p(_smallm_ws(M, N, K, W)), M, N, K, g.stride(0),
                                      z.stride(0) if z is not None else 0, eps, int(relevance_in), int(relevance_out), dt(W),
                                      _DT[out.dtype], stream()), "lrp_linear_smallm_dgrad")
    return out


TAIL_SPLIT = True        # module attribute (A/B measurements): False = the round-3 handling of 257 ... 511-tile GEMMs


def tail_split_cols(M, Nout, Kc):
    """GEMMs whose tile count (256 x 256 tiles) is not a whole number of rounds of the 256 CUs and whose LAST round is at most half full
    (Gemma-3-4B: 8192 x 2560 = 320 tiles = 1.25 rounds; SigLIP: 16384 x 4352 = 1088 tiles = 4.25 rounds: the last round keeps a quarter of the
    chip busy for a whole tile time).  -> the number of leading output columns that make whole rounds; the remaining tile columns (<= 128
    tiles) are issued as a second problem through the split-K path, which spreads them over all CUs (K split so that tail tiles x splits =
    256).  Two launches of n + ~0.25 tile times instead of n + 1 (or, for 257 ... 384 tiles and K >= 8192, instead of splitting the WHOLE problem
    in two with fp32 slabs of the whole output).  None when the shape does not qualify (a K loop too short to split: the tail's slab round trip
    would cost more than the partial round it replaces)."""
    if not TAIL_SPLIT:
        return None
    tm, tn = (M + 255) // 256, (Nout + 255) // 256
    if tm * tn <= 256 or tm > 256 or 256 % tm:
        return None
    cpr = 256 // tm                                         # tile columns per full round
    tail_cols = tn % cpr
    tail_tiles = tm * tail_cols
    if tail_cols == 0 or tail_tiles > 128 or Kc // 64 < 8 * (256 // tail_tiles):
        return None
    return (tn - tail_cols) * 256


STREAM_FWD = True        # module attribute (A/B measurements): False sends every M <= 256 forward to the split-K skinny path


STREAM_FWD_SPLITS = True    # module attribute (A/B measurements): False = narrow weights (N < 192 * 64) stay on the split-K skinny path


def linear_stream_ok(x2, W):
    """does the one-launch weight-streaming forward (lrp_linear_stream_fwd: narrow-N, full-K, no split-K slabs) serve z = x2 W^T?  bf16,
    M <= 256 rows, K % 512 == 0, contiguous 16-byte aligned rows, and ceil(N / 64) workgroups that fill the chip"""
    if not STREAM_FWD or x2.dtype != torch.bfloat16 or W.dtype != torch.bfloat16 or x2.dim() != 2 or W.dim() != 2:
        return False
    if x2.stride(1) != 1 or W.stride(1) != 1 or x2.data_ptr() % 16 or W.data_ptr() % 16:
        return False
    if not lib.lrp_linear_stream_ok(x2.shape[0], W.shape[0], x2.shape[1], x2.stride(0), W.stride(0)):
        return False
    return bool(STREAM_FWD_SPLITS or lib.lrp_linear_stream_fwd_splits(x2.shape[0], W.shape[0], x2.shape[1]) == 1)


def _stream_fwd_buffers(x2, N, out, out_dtype):
    """-> (out, slab workspace, tickets) of the streaming forward and its MXFP4 form: the output allocated when not given, and for narrow
    weights (K splits, slabs summed in-kernel; one split policy for both forms: bit identity needs it) the scratch, else None / None"""
    M, K = x2.shape
    if out is None:
        out = torch.empty(M, N, device=x2.device, dtype=out_dtype or x2.dtype)
    need = lib.lrp_linear_stream_fwd_ws(M, N, K) if STREAM_FWD_SPLITS else 0
    ws = workspace(need, x2) if need else None
    ntk = lib.lrp_linear_stream_fwd_tickets(M, N, K) if need else 0
    return out, ws, tickets(ntk, x2) if ntk else None


def linear_stream_fwd(x2, W, bias=None, out=None, out_dtype=None):
    """z[M,N] = x2[M,K] @ W[N,K]^T (+ bias), M <= 256, in ONE launch: every workgroup streams 64 rows of W over the whole K range"""
    M, K = x2.shape
    N = W.shape[0]
    same(x2, W)
    out, ws, tk = _stream_fwd_buffers(x2, N, out, out_dtype)
    check(lib.lrp_linear_stream_fwd_tk(p(x2), p(W), p(aux(bias, x2, N)), p(out), M, N, K, x2.stride(0), W.stride(0), out.stride(0), dt(x2),
                                       _DT[out.dtype], p(ws), p(tk), stream()), "lrp_linear_stream_fwd_tk")
    return out


def linear_fwd(x2, W, bias=None, out=None, out_dtype=None):
    """z[M,N] = x2[M,K] @ W[N,K]^T (+ bias) on the kernel that fits M (ref: lxt/explicit/functional.py:351):
       M <= 256 rows, bf16, K % 512 == 0, N >= 192 * 64 : one-launch weight-streaming kernel (narrow N, full K: no slabs, no second launch)
       M <= 256 rows, bf16, K % 64 == 0 : split-K skinny path of the ping-pong GEMM (W streamed once by all CUs)
       M <= 16 otherwise                : W-streaming small-M kernels (fp32, odd K)
       else                             : the MFMA GEMM (lrp_gemm_nt)"""
    M, K = x2.shape
    N = W.shape[0]
    odt = out_dtype or (out.dtype if out is not None else x2.dtype)
    if M <= SKINNY_MAX and linear_stream_ok(x2, W) and (out is None or (out.stride(1) == 1 and out.dtype in _DT)):
        return linear_stream_fwd(x2, W, bias, out=out, out_dtype=odt)
    if gemm_nn_ok(x2, W) and M > SKINNY_MAX:
        main = tail_split_cols(M, N, K)
        if main is not None and (out is None or out.stride(1) == 1):
            if out is None:
                out = torch.empty(M, N, device=x2.device, dtype=odt)
            bias = aux(bias, x2, N)
            gemm_nt_2d(x2, W[:main], out[:, :main], None if bias is None else bias[:main])                  # one full round of the chip
            gemm_skinny(x2, W[main:], out[:, main:], nn=False, bias=None if bias is None else bias[main:])    # the tail, K-split over all CUs
            return out
    if splitk_ok(M, N, K) and gemm_nn_ok(x2, W):
        if out is None:
            out = torch.empty(M, N, device=x2.device, dtype=odt)
        return gemm_skinny(x2, W, out, nn=False, bias=bias)
    if smallm_ok(M, W, x2):
        return linear_smallm_fwd(x2, W, bias, out=out, out_dtype=odt)
    if out is not None and x2.stride(1) == 1 and W.stride(1) == 1 and x2.dtype == W.dtype and x2.stride(0) % epc(x2) == 0:
        return gemm_nt_2d(x2, W, out, bias)
    z = gemm_nt(x2, W, bias, out_dtype=odt)
    if out is not None:
        out.copy_(z)
        return out
    return z


STREAM_DGRAD = True       # module attribute (A/B measurements): False keeps every small-M dgrad on the small-M / split-K skinny kernels


def linear_stream_dgrad_ok(s2, W):
    """is lrp_linear_stream_dgrad (64-column workgroups, wave-private LDS rings, transpose-read W operand) the kernel for c = s2 W?  bf16,
    M <= 32, N % 128 == 0, Kout % 64 == 0, contiguous 16-byte aligned rows, and a split count that fills the chip with <= 320 workgroups"""
    if not STREAM_DGRAD or s2.dtype != torch.bfloat16 or W.dtype != torch.bfloat16 or s2.dim() != 2 or W.dim() != 2:
        return False
    if s2.stride(1) != 1 or W.stride(1) != 1 or s2.data_ptr() % 16 or W.data_ptr() % 16:
        return False
    return bool(lib.lrp_linear_stream_dgrad_ok(s2.shape[0], W.shape[0], W.shape[1], s2.stride(0), W.stride(0)))


def linear_stream_dgrad(s2, W, out=None, out_dtype=None, z=None, eps=0.0, relevance_in=False):
    """c[M,Kout] = s'[M,N] @ W[N,Kout] for M <= 64 from the stored weight, W streamed once; s' = s2, or with z (the Linear's forward output)
    the eps-rule's stabilised operand formed inside the kernel: s2 z / (z + eps), or s2 / (z + eps) when s2 is a relevance (relevance_in)"""
    M, N = s2.shape
    Kout = W.shape[1]
    same(s2, W, z)
    if z is not None and (z.stride(1) != 1 or tuple(z.shape) != (M, N)):
        raise ValueError("linear_stream_dgrad: z must be [M, N] with contiguous rows")
    if z is not None and eps == 0.0:
        if relevance_in:
            raise ValueError("linear_stream_dgrad: a relevance operand needs eps != 0 (s / (z + 0) has no defined value at z = 0)")
        z = None                    # eps = 0: the stabiliser z / (z + 0) is exactly 1 (lxt.efficient) -- never formed as g * z * rcp(z)
    if out is None:
        out = torch.empty(M, Kout, device=s2.device, dtype=out_dtype or s2.dtype)
    need = lib.lrp_linear_stream_dgrad_ws(M, N, Kout)
    ws = workspace(need, s2) if need else None
    ntk = lib.lrp_linear_stream_dgrad_tickets(M, N, Kout) if STREAM_DGRAD_INKERNEL_REDUCE else 0
    check(lib.lrp_linear_stream_dgrad_tk(p(s2), p(z), p(W), p(out), M, N, Kout, s2.stride(0), z.stride(0) if z is not None else 0, W.stride(0),
                                         out.stride(0), eps, int(relevance_in), dt(s2), _DT[out.dtype], p(ws), p(tickets(ntk, s2) if ntk else None),
                                         stream()), "lrp_linear_stream_dgrad_tk")
    return out


def linear_dgrad(s2, W, out=None, out_dtype=None):
    """c[M,K] = s2[M,N] @ W[N,K]: the redistribution half of the Linear eps-rule (ref: lxt/explicit/functional.py:355-364) from the
    STORED weight layout:
       M <= 32, bf16, N % 128 == 0, Kout % 64 == 0            : lrp_linear_stream_dgrad (64-column workgroups, wave-private LDS rings; round 5: also
                                                               for M <= 2 -- with the in-kernel slab reduction it is 1.5 ... 8 us ahead of the
                                                               lane-local kernel there, tools/dgrad_m12.py)
       M <= 2, or M <= 16 where the NN kernel does not apply : W-streaming small-M dgrad
       M <= 256, bf16, N % 64 == 0                           : split-K skinny path, NN form
       bf16 problems of >= 190 tiles of 256 x 256            : lrp_gemm_nn (no W^T copy)
       everything else (fp32 parity path, odd shapes)        : lrp_gemm_nt on a W^T copy cached on the weight (ops.weight_t)"""
    M, N = s2.shape
    K = W.shape[1]
    odt = out_dtype or (out.dtype if out is not None else W.dtype)
    if M <= 32 and linear_stream_dgrad_ok(s2, W) and (out is None or (out.stride(1) == 1 and out.dtype in _DT)):
        return linear_stream_dgrad(s2, W, out=out, out_dtype=odt)
    nn = gemm_nn_ok(s2, W)
    if (M <= 2 or (M <= SMALLM_MAX and not nn)) and N >= 16 and smallm_ok(M, W) and s2.stride(1) == 1 and s2.dtype == W.dtype:
        return linear_smallm_dgrad(s2, W, out=out, out_dtype=odt)
    if nn and M > SKINNY_MAX:
        main = tail_split_cols(M, K, N)
        if main is not None and (out is None or out.stride(1) == 1) and W.data_ptr() % 16 == 0:
            if out is None:
                out = torch.empty(M, K, device=s2.device, dtype=odt)
            gemm_nn_2d(s2, W[:, :main], out[:, :main])                           # one full round of the chip
            gemm_skinny(s2, W[:, main:], out[:, main:], nn=True)                  # the tail (<= 128 tiles), contraction split over all CUs
            return out
    if nn:
        split = splitk_ok(M, K, N)
        # the NN form exists only in the 256 x 256 ping-pong kernel: problems it cannot fill (fewer than 190 tiles and no split-K: BERT-sized
        # weights at a few thousand rows) run the 128 x 128 / 64 x 64 NT kernels on a cached W^T instead, as in round 2
        if split or ((M + 255) // 256) * ((K + 255) // 256) >= 190:
            if out is None:
                out = torch.empty(M, K, device=s2.device, dtype=odt)
            return gemm_skinny(s2, W, out, nn=True) if split else gemm_nn_2d(s2, W, out)
    wt = weight_t(W)
    if out is not None and s2.stride(1) == 1 and s2.dtype == wt.dtype and s2.stride(0) % epc(s2) == 0:
        return gemm_nt_2d(s2, wt, out)
    c = gemm_nt(s2, wt, out_dtype=odt)
    if out is not None:
        out.copy_(c)
        return out
    return c


def clear_weight_cache(*weights):
    """drop the cached W^T copies (fp32 / odd-shape dgrad path) of the given weight tensors -- call after writing to a weight through
    `.data` (optimizers, adapter / quantisation loaders), which does not bump `_version` and would leave a stale W^T behind"""
    for w in weights:
        _WT.pop(w.untyped_storage()._cdata, None)


# -------------------------------------------------------------------------------------- attention
def pad_to(n, m):
    return (n + m - 1) // m * m


def transpose_heads(x, B, S, H, d, out=None):
    """x: [B*S, >= H*d] 2-D view -> [B, H, d, ldt] with ldt = S padded to 64 (pad columns zero)"""
    ldt = pad_to(S, 64)
    if out is None:
        out = torch.zeros(B, H, d, ldt, device=x.device, dtype=x.dtype)
    check(lib.lrp_transpose_heads(p(x), p(out), B, S, H, d, x.stride(0), out.stride(2), dt(x), stream()), "lrp_transpose_heads")
    return out


def _iv(row_iv, B, S):
    """(row_lo, row_hi) int32 [B, S] device tensors -> two raw pointers (0, 0 when no intervals are given)"""
    if row_iv is None:
        return 0, 0
    lo, hi = row_iv
    for t in (lo, hi):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != B * S or not t.is_cuda:
            raise ValueError("row intervals must be contiguous int32 CUDA tensors of B*S elements")
    return lo.data_ptr(), hi.data_ptr()


def attn_needs_transposed(t, d):
    """do the attention kernels serving t's dtype and head dim d read head-transposed "_t" copies (transpose_heads)?
    bf16 / d = 128 does not: its kernels take every operand from the token-major tensors (pass None for the _t operands)"""
    return bool(lib.lrp_attn_needs_transposed(dt(t), d))


def attn_fwd(q, k, v, v_t, o, lse, B, S, Hq, Hkv, d, scale, causal=True, window=0, q_begin=0, row_iv=None):
    same(q, k, v, v_t, o)
    f32(lse)
    check(lib.lrp_attn_fwd(p(q), p(k), p(v), p(v_t), p(o), p(lse), B, S, Hq, Hkv, d, q.stride(0), k.stride(0), v.stride(0),
                           v_t.stride(2) if v_t is not None else 0, o.stride(0), scale, int(causal), window, q_begin,
                           *_iv(row_iv, B, S), dt(q), stream()), "lrp_attn_fwd")
    return o, lse


def attn_bwd_prep(Go, o, Gho, D, B, S, Hq, d, eps_pv, factor=0.5):
    same(Go, o, Gho)
    f32(D)
    check(lib.lrp_attn_bwd_prep(p(Go), p(o), p(Gho), p(D), B, S, Hq, d, Go.stride(0), o.stride(0), Gho.stride(0), eps_pv,
                                factor, dt(Go), stream()), "lrp_attn_bwd_prep")
    return Gho, D


def attn_bwd_dq(q, k, v, k_t, Gho, lse, D, dq, B, S, Hq, Hkv, d, scale, eps_mask, eps_qk, causal=True, window=0, q_begin=0,
                row_iv=None):
    same(q, k, v, k_t, Gho, dq)
    f32(lse, D)
    check(lib.lrp_attn_bwd_dq(p(q), p(k), p(v), p(k_t), p(Gho), p(lse), p(D), p(dq), B, S, Hq, Hkv, d, q.stride(0),
                              k.stride(0), v.stride(0), k_t.stride(2) if k_t is not None else 0, Gho.stride(0), dq.stride(0),
                              scale, eps_mask, eps_qk,
                              int(causal), window, q_begin, *_iv(row_iv, B, S), dt(q), stream()), "lrp_attn_bwd_dq")
    return dq


PREP_FUSION = True       # module attribute: False = the stand-alone lrp_attn_bwd_prep pass (A/B measurements)


def attn_dq_d_ok(dtype, d):
    """lrp_attn_bwd_dq_d serves (dtype, d): the dQ kernel forms D = rowsum(Gho (*) o) itself (no attn_bwd_prep pass)"""
    return bool(PREP_FUSION and dtype in _DT and lib.lrp_attn_bwd_dq_d_ok(_DT[dtype], d))


def attn_bwd_dq_d(q, k, v, Gho, o, lse, D, dq, B, S, Hq, Hkv, d, scale, causal=True, window=0, row_iv=None, rope=None):
    """dQ of the lxt.efficient placement with D[b, h, s] = sum_d Gho o formed in the kernel and WRITTEN to D (for attn_bwd_dkv); rope = (cos, sin)
    fp32 [>= S, d]: RoPE's backward applied to dQ on its way out (then dq is the gradient w.r.t. the UN-rotated q)"""
    same(q, k, v, Gho, o, dq)
    f32(lse, D)
    cs, sn = rope if rope is not None else (None, None)
    f32(cs, sn)
    check(lib.lrp_attn_bwd_dq_d(p(q), p(k), p(v), p(Gho), p(o), p(lse), p(D), p(dq), B, S, Hq, Hkv, d, q.stride(0), k.stride(0), v.stride(0),
                                Gho.stride(0), o.stride(0), dq.stride(0), scale, int(causal), window, *_iv(row_iv, B, S), p(cs), p(sn), dt(q),
                                stream()), "lrp_attn_bwd_dq_d")
    return dq


ROPE_BWD_FUSION = True   # module attribute (A/B): False = the stand-alone lrp_rope_bwd pass


def gqa_reduce_rope(x, out, rows, seq, Hkv, rep, d, cos, sin):
    """out[r, hk, :] = RoPE^T(sum_j x[r, hk rep + j, :]) -- the GQA group sum of dK and RoPE's backward in one pass"""
    f32(cos, sin)
    _rope_tables(cos, sin, seq, d, "lrp_gqa_reduce_rope")
    check(lib.lrp_gqa_reduce_rope(p(x), p(out), rows, seq, Hkv, rep, d, x.stride(0), out.stride(0), p(cos), p(sin), dt(x), stream()),
          "lrp_gqa_reduce_rope")
    return out


def attn_bwd_dkv(q, k, v, q_t, Gho, Gho_t, lse, D, dk_h, dv_h, B, S, Hq, Hkv, d, scale, eps_mask, eps_qk, causal=True,
                 window=0, q_begin=0, row_iv=None):
    same(q, k, v, q_t, Gho, Gho_t, dk_h, dv_h)
    f32(lse, D)
    check(lib.lrp_attn_bwd_dkv(p(q), p(k), p(v), p(q_t), p(Gho), p(Gho_t), p(lse), p(D), p(dk_h), p(dv_h), B, S, Hq, Hkv, d,
                               q.stride(0), k.stride(0), v.stride(0), q_t.stride(2) if q_t is not None else 0, Gho.stride(0),
                               dk_h.stride(0),
                               dv_h.stride(0), scale, eps_mask, eps_qk, int(causal), window, q_begin, *_iv(row_iv, B, S), dt(q), stream()),
          "lrp_attn_bwd_dkv")
    return dk_h, dv_h


def attn_bwd_dv_ok(dtype, d):
    """lrp_attn_bwd_dv serves (dtype, d): bf16 at d in {64, 96, 128}, fp32 at d in {16, 32, 64, 128}"""
    return bool(dtype in _DT and lib.lrp_attn_bwd_dv_ok(_DT[dtype], d))


def attn_bwd_dv(q, k, G, lse, dv, B, S, Hq, Hkv, d, scale, q_begin=0, row_iv=None, q_t=None, G_t=None):
    """the CP-LRP attention backward (q, k detached): dv [B S, Hkv d] = sum over the GQA group of P^T G, causal, G the gradient of the attention
    output as it is.  G_t: the head-transposed copy of G where attn_needs_transposed(q, d); q_t is accepted beside it (the operand list of
    attn_bwd_dkv) and not read: no contraction of this kernel runs over Q^T."""
    same(q, k, G, dv, q_t, G_t)
    f32(lse)
    check(lib.lrp_attn_bwd_dv(p(q), p(k), p(G), p(G_t), p(lse), p(dv), B, S, Hq, Hkv, d, q.stride(0), k.stride(0), G.stride(0),
                              G_t.stride(2) if G_t is not None else 0, dv.stride(0), scale, q_begin, *_iv(row_iv, B, S), dt(q), stream()),
          "lrp_attn_bwd_dv")
    return dv


def gqa_reduce(x, out, rows, Hkv, rep, d):
    check(lib.lrp_gqa_reduce(p(x), p(out), rows, Hkv, rep, d, x.stride(0), out.stride(0), dt(x), stream()), "lrp_gqa_reduce")
    return out


# ------------------------------------------------------------------------------------------- KV-cached decode (csrc/decode.hip)
ATTN_DECODE_SLAB = int(lib.lrp_attn_decode_slab())          # keys per slab of attn_decode, counted from key 0


def _decode_rows(name, t, what, rows, cols, ref=None):
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != cols or t.stride(1) != 1:
        raise ValueError(f"{name}: {what} {tuple(t.shape)} must be [{rows}, {cols}] with contiguous rows")
    if ref is not None:
        same(ref, t)


def _decode_cache(name, kc, vc, B, cols, ref):
    """-> (cap, ldc) of the caches kc, vc [B, cap, cols]: unit column stride, one row pitch, batch stride cap * pitch"""
    for what, t in (("kc", kc), ("vc", vc)):
        if t.dim() != 3 or t.shape[0] != B or t.shape[2] != cols or t.shape[1] < 1 or t.stride(2) != 1 or t.shape != kc.shape \
                or t.stride() != kc.stride() or (B > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
            raise ValueError(f"{name}: {what} {tuple(t.shape)} / strides {t.stride()} must be [{B}, cap, {cols}] with contiguous rows, batch stride "
                             "cap * row pitch, kc and vc alike")
    same(ref, kc, vc)
    return int(kc.shape[1]), int(kc.stride(1))


def _decode_pos(name, pos, ref):
    if pos.dtype != torch.int32 or pos.numel() != 1 or pos.device != ref.device:
        raise TypeError(f"{name}: pos must be an int32 tensor of one element on {ref.device} (the step's column, read on the device)")


def decode_rope_append(qk, v, cos, sin, pos, q_rot, kc, vc, nq, nk, d):
    """one decode step's RoPE and cache append, one launch: q_rot [B, nq d] = RoPE(qk[:, : nq d]), kc[b, pos] = RoPE(qk[:, nq d:]),
    vc[b, pos] = v, at the tables' row pos -- bitwise rope_fwd(seq=1) with cos[pos: pos + 1].  qk [B, (nq + nk) d], v [B, nk d]: 2-D views
    with unit column stride (the two column ranges of one qkv buffer); kc, vc [B, cap, nk d]; cos / sin fp32 [rows, d] contiguous; pos:
    device int32 [1].  A pos outside [0, cap) or past the tables writes nothing (checked on the device)."""
    B = qk.shape[0]
    pq = p(qk)                          # (device tensors only: raises before anything else)
    _decode_rows("decode_rope_append", qk, "qk", B, (nq + nk) * d)
    _decode_rows("decode_rope_append", v, "v", B, nk * d, qk)
    _decode_rows("decode_rope_append", q_rot, "q_rot", B, nq * d, qk)
    cap, ldc = _decode_cache("decode_rope_append", kc, vc, B, nk * d, qk)
    _decode_pos("decode_rope_append", pos, qk)
    f32(cos, sin)
    if cos.dim() != 2 or cos.shape[1] != d or cos.shape != sin.shape or not cos.is_contiguous() or not sin.is_contiguous():
        raise ValueError(f"decode_rope_append: cos / sin must be contiguous [rows, {d}] tables")
    ld = lambda t: t.stride(0) if B > 1 else max(t.stride(0), t.shape[1])      # noqa: E731  (a one-row view's pitch is arbitrary)
    check(lib.lrp_decode_rope_append(pq, ld(qk), p(v), ld(v), p(cos), p(sin), cos.shape[0], p(pos), p(q_rot), ld(q_rot), p(kc), p(vc), ldc, B, cap,
                                     nq, nk, d, dt(qk), stream()), "lrp_decode_rope_append")
    return q_rot


def decode_qknorm_rope_append(qk, v, wq, wk, eps, cos, sin, pos, q_rot, kc, vc, nq, nk, d, w_offset=0.0):
    """decode_rope_append with the per-head RMSNorms of q and k (wq, wk [d] in qk's dtype, eps, w_offset: 1 for Gemma's (1 + w)) in front
    of the rotation, one launch (csrc/decode_site.hip) -- bitwise head_rmsnorm_fwd on the q columns, head_rmsnorm_fwd on the k columns, then
    decode_rope_append.  Operands and the device-side check of pos as there; no rstd is written.  d * element size / 16 a power of two,
    d <= 256."""
    B = qk.shape[0]
    pq = p(qk)
    _decode_rows("decode_qknorm_rope_append", qk, "qk", B, (nq + nk) * d)
    _decode_rows("decode_qknorm_rope_append", v, "v", B, nk * d, qk)
    _decode_rows("decode_qknorm_rope_append", q_rot, "q_rot", B, nq * d, qk)
    cap, ldc = _decode_cache("decode_qknorm_rope_append", kc, vc, B, nk * d, qk)
    _decode_pos("decode_qknorm_rope_append", pos, qk)
    f32(cos, sin)
    if cos.dim() != 2 or cos.shape[1] != d or cos.shape != sin.shape or not cos.is_contiguous() or not sin.is_contiguous():
        raise ValueError(f"decode_qknorm_rope_append: cos / sin must be contiguous [rows, {d}] tables")
    same(qk, wq, wk)          # (no conversion here: the step is captured, a cast would allocate)
    if wq.numel() != d or wk.numel() != d or not wq.is_contiguous() or not wk.is_contiguous():
        raise ValueError(f"decode_qknorm_rope_append: wq / wk must be contiguous [{d}] norm weights")
    ld = lambda t: t.stride(0) if B > 1 else max(t.stride(0), t.shape[1])      # noqa: E731  (a one-row view's pitch is arbitrary)
    check(lib.lrp_decode_qknorm_rope_append(pq, ld(qk), p(v), ld(v), p(wq), p(wk), float(eps), float(w_offset), p(cos), p(sin), cos.shape[0],
                                            p(pos), p(q_rot), ld(q_rot), p(kc), p(vc), ldc, B, cap, nq, nk, d, dt(qk), stream()),
          "lrp_decode_qknorm_rope_append")
    return q_rot


def attn_decode_ws(B, Hq, d, cap):
    """bytes of attn_decode's workspace"""
    n = int(lib.lrp_attn_decode_ws(B, Hq, d, cap))
    if n < 0:
        raise ValueError(f"attn_decode: no kernel for B = {B}, Hq = {Hq}, d = {d}, cap = {cap} (d a multiple of 8, at most 256)")
    return n


def attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale, out=None, ws=None):
    """single-query attention over a KV cache: out[b, h] = sum_{lo[b] <= j <= pos} softmax_j(scale q[b, h] . kc[b, j, h // rep]) vc[b, j, h // rep]
    ([B, Hq d], q's dtype).  q [B, Hq d] with unit column stride; kc, vc [B, cap, Hkv d]; lo int32 [B] (clamped into [0, pos] by the kernel);
    pos: device int32 [1].  Rows of the cache outside [lo[b], pos] are never loaded.  ws: a uint8 workspace of attn_decode_ws bytes (None:
    ops.workspace).  Fixed-order fp32 sums over slabs of ATTN_DECODE_SLAB keys counted from key 0: bitwise repeatable, a prompt's result does
    not depend on the batch or on cap."""
    B = q.shape[0]
    pq = p(q)
    _decode_rows("attn_decode", q, "q", B, Hq * d)
    cap, ldc = _decode_cache("attn_decode", kc, vc, B, Hkv * d, q)
    _decode_pos("attn_decode", pos, q)
    if lo.dtype != torch.int32 or lo.numel() != B or not lo.is_contiguous() or lo.device != q.device:
        raise TypeError(f"attn_decode: lo must be a contiguous int32 [{B}] tensor on {q.device}")
    if out is None:
        out = torch.empty(B, Hq * d, device=q.device, dtype=q.dtype)
    _decode_rows("attn_decode", out, "out", B, Hq * d, q)
    if B == 0:
        return out
    need = attn_decode_ws(B, Hq, d, cap)
    if ws is None:
        ws = workspace(need, q)
    elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.device != q.device:
        raise ValueError(f"attn_decode: ws must be a contiguous uint8 tensor of >= {need} bytes on {q.device}")
    ld = lambda t: t.stride(0) if B > 1 else max(t.stride(0), t.shape[1])      # noqa: E731
    check(lib.lrp_attn_decode(pq, ld(q), p(kc), p(vc), ldc, p(lo), p(pos), p(out), ld(out), p(ws), ws.numel(), B, cap, Hq, Hkv, d, float(scale),
                              dt(q), stream()), "lrp_attn_decode")
    return out


# ------------------------------------------------------------------------------------------- MoE experts (csrc/moe.hip)
class MoePlan:
    """device-side routing plan of one MoE layer (lrp_moe_plan): int32 words, nothing read back to the host"""

    def __init__(self, idx, E):
        if idx.dim() != 2:
            raise ValueError(f"lrp_moe_plan: top_k_index must be [T, k], got {tuple(idx.shape)}")
        self.T, self.k, self.E = int(idx.shape[0]), int(idx.shape[1]), int(E)
        n = lib.lrp_moe_plan_ints(self.T, self.k, self.E)
        if n < 0:
            check(int(n), "lrp_moe_plan_ints")
        p(idx)
        idx = idx.to(torch.int64).contiguous()
        self.buf = torch.empty(int(n), device=idx.device, dtype=torch.int32)
        check(lib.lrp_moe_plan(p(idx), p(self.buf), self.T, self.k, self.E, stream()), "lrp_moe_plan")

    @property
    def rows(self):
        return self.T * self.k

    def views(self):
        """(cnt, off, perm, inv) as tensors (tests / tools; off has E + 1 entries, perm rows past off[E] are unwritten)"""
        E, R, b = self.E, self.rows, self.buf
        return b[:E], b[E:2 * E + 1], b[3 * E + 2:3 * E + 2 + R], b[3 * E + 2 + R:3 * E + 2 + 2 * R]


class MoeQuantWeight:
    """an expert tensor [E, N, K] held as MXFP4 (include/lrp_hip_moe_mxfp4.h): codes uint8 [E, N, K / 2] and scales uint8 [E, N, K / 32], the
    2-D format of mxfp4_quantize applied to the [E N, K] view.  MoeQuantWeight(w) quantises a device tensor (into codes / scales when given:
    the engine passes views of its flat_q); from_bytes wraps stored bytes.  The four grouped expert GEMMs take it in place of the weight
    tensor and decode inside the kernel -- bit-identical to the same call on dequant(dtype)."""

    def __init__(self, w, codes=None, scales=None):
        if not w.is_cuda:
            raise RuntimeError("MoeQuantWeight: lrp_hip kernels need device tensors (no CPU fallback)")
        if w.dim() != 3 or not w.is_contiguous() or w.shape[2] % (4 * MX_BLOCK):      # (K / 32 scale bytes per row, rows on the 4-byte grid)
            raise ValueError(f"MoeQuantWeight: an expert tensor is a contiguous [E, N, K] with K % {4 * MX_BLOCK} == 0, got {tuple(w.shape)}")
        E, N, K = w.shape
        if codes is None:
            codes = torch.empty(E, N, K // 2, device=w.device, dtype=torch.uint8)
        if scales is None:
            scales = torch.empty(E, N, K // MX_BLOCK, device=w.device, dtype=torch.uint8)
        self._set(codes, scales)
        if self.shape != (E, N, K):
            raise ValueError(f"MoeQuantWeight: codes / scales of a {self.shape} tensor for a weight of {(E, N, K)}")
        mxfp4_quantize(w.view(E * N, K), codes.view(E * N, K // 2), scales.view(E * N, K // MX_BLOCK))

    def _set(self, codes, scales):
        if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 3 or not codes.is_contiguous():
            raise ValueError(f"MoeQuantWeight: codes must be a contiguous uint8 [E, N, K / 2] tensor and scales uint8, got {codes.dtype} "
                             f"{tuple(codes.shape)} and {scales.dtype}")
        E, N, K2 = codes.shape
        if (2 * K2) % (4 * MX_BLOCK) or tuple(scales.shape) != (E, N, 2 * K2 // MX_BLOCK) or not scales.is_contiguous() or scales.device != codes.device:
            raise ValueError(f"MoeQuantWeight: scales must be a contiguous uint8 [{E}, {N}, {2 * K2} / {MX_BLOCK}] tensor on {codes.device}, got "
                             f"{tuple(scales.shape)} on {scales.device}")
        self.codes, self.scales, self.shape = codes, scales, (E, N, 2 * K2)

    @classmethod
    def from_bytes(cls, codes, scales):
        q = cls.__new__(cls)
        q._set(codes, scales)
        return q

    @property
    def device(self):
        return self.codes.device

    def nbytes(self):
        return self.codes.numel() + self.scales.numel()

    def dequant(self, dtype, out=None):
        """-> the tensor [E, N, K] the bytes hold, exact in float32 and bfloat16 (lrp_mxfp4_dequant on the [E N, K] view)"""
        E, N, K = self.shape
        p(self.codes)
        if out is None:
            out = torch.empty(E, N, K, device=self.device, dtype=dtype)
        mxfp4_dequant(self.codes.view(E * N, K // 2), self.scales.view(E * N, K // MX_BLOCK), out.view(E * N, K))
        return out


def _moe_w(x, W):
    """the weight operand of a grouped expert GEMM next to the activation x -> (quantised?, the pointer arguments)"""
    if isinstance(W, MoeQuantWeight):
        if W.device != x.device and x.is_cuda and W.codes.is_cuda:
            raise TypeError(f"lrp_hip: quantised expert weight on {W.device} next to activations on {x.device}")
        return True, (p(W.codes), p(W.scales))
    same(x, W)
    return False, (p(W),)


def _moe_buf(name, buf, rows, cols, like, dtype=None, pitched=True):
    """an output buffer a caller hands to a MoE wrapper: [rows, cols] of `like`'s device and dtype (or `dtype`) with contiguous rows -- its
    stride(0) is passed on as the pitch, so a [:, :cols] view of wider storage is served -- or contiguous where the kernel takes no pitch"""
    dtype = like.dtype if dtype is None else dtype
    if not torch.is_tensor(buf) or buf.dtype != dtype:
        raise TypeError(f"{name}: must be a {dtype} tensor, got {buf.dtype if torch.is_tensor(buf) else type(buf).__name__}")
    if buf.device != like.device:
        raise TypeError(f"{name}: on {buf.device} next to operands on {like.device}")
    if tuple(buf.shape) != (rows, cols) or (cols > 1 and buf.stride(1) != 1) or (not pitched and not buf.is_contiguous()):
        raise ValueError(f"{name}: must be [{rows}, {cols}] with contiguous rows{'' if pitched else ' and no pitch'}, got {tuple(buf.shape)} with "
                         f"strides {tuple(buf.stride())}")
    return buf


def moe_gate_up_fwd(x, Wgu, plan, act="silu", coef=None, m=None):
    """-> (coef [R, 2 I], m [R, I]) in plan-row order; x [T, H] rows are gathered through the plan inside the GEMM.  Wgu: the tensor
    [E, 2 I, H] or a MoeQuantWeight of it (here and in the three GEMMs below: decoded inside the kernel, lrp_moe_*_q).  coef / m (here and
    below: out, Agu, part, gw): a buffer to write into, rows may carry a pitch; only the first off[E] plan rows and no pad column are written"""
    E, I2, H = Wgu.shape
    I, R = I2 // 2, plan.rows
    q, wp = _moe_w(x, Wgu)
    coef = torch.empty(R, 2 * I, device=x.device, dtype=x.dtype) if coef is None else _moe_buf("moe_gate_up_fwd: coef", coef, R, 2 * I, x)
    m = torch.empty(R, I, device=x.device, dtype=x.dtype) if m is None else _moe_buf("moe_gate_up_fwd: m", m, R, I, x)
    if q:
        _timed(2.0 * R * 2 * I * H, "moe_gate_up_fwd", lambda: lib.lrp_moe_gate_up_fwd_q(
            p(x), *wp, p(plan.buf), p(coef), p(m), plan.T, plan.k, plan.E, H, I, x.stride(0), coef.stride(0), m.stride(0), ACT[act],
            dt(x), stream()), "lrp_moe_gate_up_fwd_q")
        return coef, m
    _timed(2.0 * R * 2 * I * H, "moe_gate_up_fwd", lambda: lib.lrp_moe_gate_up_fwd(
        p(x), p(Wgu), p(plan.buf), p(coef), p(m), plan.T, plan.k, plan.E, H, I, x.stride(0), coef.stride(0), m.stride(0), ACT[act],
        dt(x), stream()), "lrp_moe_gate_up_fwd")
    return coef, m


def moe_down_fwd(m, Wd, plan, out=None):
    """-> y [R, H] = m Wd[e]^T per plan row"""
    E, H, I = Wd.shape
    q, wp = _moe_w(m, Wd)
    y = torch.empty(plan.rows, H, device=m.device, dtype=m.dtype) if out is None else _moe_buf("moe_down_fwd: out", out, plan.rows, H, m)
    if q:
        _timed(2.0 * plan.rows * H * I, "moe_down_fwd", lambda: lib.lrp_moe_down_fwd_q(
            p(m), *wp, p(plan.buf), p(y), plan.T, plan.k, plan.E, H, I, m.stride(0), y.stride(0), dt(m), stream()), "lrp_moe_down_fwd_q")
        return y
    _timed(2.0 * plan.rows * H * I, "moe_down_fwd", lambda: lib.lrp_moe_down_fwd(
        p(m), p(Wd), p(plan.buf), p(y), plan.T, plan.k, plan.E, H, I, m.stride(0), y.stride(0), dt(m), stream()), "lrp_moe_down_fwd")
    return y


def moe_combine(rows, plan, w=None, out=None):
    """-> out [T, H] = sum over live slots s of w[t, s] rows[row(t, s)] (w None: weight 1), fp32 accumulation in slot order"""
    H = rows.shape[1]
    same(rows, w)
    out = torch.empty(plan.T, H, device=rows.device, dtype=rows.dtype) if out is None else _moe_buf("moe_combine: out", out, plan.T, H, rows)
    check(lib.lrp_moe_combine(p(rows), p(w), p(plan.buf), p(out), plan.T, plan.k, plan.E, H, rows.stride(0), out.stride(0), dt(rows),
                              stream()), "lrp_moe_combine")
    return out


def moe_down_dgrad(G, Wd, coef, m, w, plan, Agu=None, part=None, gw=None):
    """-> (Agu [R, 2 I] in [gate | up] order, G_w [T, k]) from the output gradient G [T, H] (gathered by token inside the GEMM)"""
    E, H, I = Wd.shape
    q, wp = _moe_w(G, Wd)
    same(G, coef, m, w)
    R = plan.rows
    Agu = torch.empty(R, 2 * I, device=G.device, dtype=G.dtype) if Agu is None else _moe_buf("moe_down_dgrad: Agu", Agu, R, 2 * I, G)
    part = (torch.empty(R, I // 128, device=G.device, dtype=torch.float32) if part is None
            else _moe_buf("moe_down_dgrad: part", part, R, I // 128, G, dtype=torch.float32, pitched=False))
    gw = (torch.empty(plan.T, plan.k, device=G.device, dtype=G.dtype) if gw is None
          else _moe_buf("moe_down_dgrad: gw", gw, plan.T, plan.k, G, pitched=False))
    fn, name = (lib.lrp_moe_down_dgrad_q, "lrp_moe_down_dgrad_q") if q else (lib.lrp_moe_down_dgrad, "lrp_moe_down_dgrad")
    _timed(2.0 * R * H * I, "moe_down_dgrad", lambda: fn(
        p(G), *wp, p(coef), p(m), p(w), p(plan.buf), p(Agu), p(part), plan.T, plan.k, plan.E, H, I, G.stride(0), coef.stride(0),
        m.stride(0), Agu.stride(0), dt(G), stream()), name)
    check(lib.lrp_moe_gw_reduce(p(part), p(plan.buf), p(gw), plan.T, plan.k, plan.E, I, dt(G), stream()), "lrp_moe_gw_reduce")
    return Agu, gw


def moe_gate_up_dgrad(Agu, Wgu, plan, out=None):
    """-> per-row G_x [R, H] = Agu Wgu[e] (NN on the stored weight)"""
    E, I2, H = Wgu.shape
    q, wp = _moe_w(Agu, Wgu)
    gx = torch.empty(plan.rows, H, device=Agu.device, dtype=Agu.dtype) if out is None else _moe_buf("moe_gate_up_dgrad: out", out, plan.rows, H, Agu)
    fn, name = (lib.lrp_moe_gate_up_dgrad_q, "lrp_moe_gate_up_dgrad_q") if q else (lib.lrp_moe_gate_up_dgrad, "lrp_moe_gate_up_dgrad")
    _timed(2.0 * plan.rows * I2 * H, "moe_gate_up_dgrad", lambda: fn(
        p(Agu), *wp, p(plan.buf), p(gx), plan.T, plan.k, plan.E, H, I2 // 2, Agu.stride(0), gx.stride(0), dt(Agu), stream()), name)
    return gx


MOE_WGRAD_MODES = {"gate_up": 0, "down": 1}          # (LRP_MOE_WGRAD_GATE_UP / _DOWN)


def moe_wgrad_rel(G, X, W, plan, mode, w=None, out=None, accumulate=False):
    """out[e][n, k] (+)= W[e][n, k] sum_{p in e} s(p) G[gp(p), n] X[xp(p), k]  ([E, N, K] fp32, contiguous): the per-weight relevance
    `weight * weight.grad` of an expert tensor W [E, N, K] -- the tensor or a MoeQuantWeight of it (decoded in the kernel's epilogue,
    lrp_moe_wgrad_rel_q: bit-identical to the call on dequant(dtype)) -- over the plan rows p of every expert (include/lrp_hip_moe_wgrad.h).
    mode "gate_up": G [R, N] in plan rows (moe_down_dgrad's Agu), X [T, K] gathered by token (the experts' input); mode "down": G [T, N]
    gathered by token (the gradient at the block's output) and scaled by 1/2 w[t, slot], X [R, K] in plan rows (the stored m), w [T, k] the
    routing weights.  accumulate: add to out (which then must be given); an expert without rows is written as exact zeros, or left untouched
    when accumulating.  bf16: N and K multiples of 8; quantised: K a multiple of 128.  One launch, no atomics: bitwise repeatable."""
    if mode not in MOE_WGRAD_MODES:
        raise ValueError(f"moe_wgrad_rel: mode must be one of {tuple(MOE_WGRAD_MODES)}, got {mode!r}")
    if not isinstance(plan, MoePlan):
        raise TypeError("moe_wgrad_rel: plan must be a MoePlan")
    if G.dim() != 2 or X.dim() != 2 or len(W.shape) != 3:
        raise ValueError(f"moe_wgrad_rel: G {tuple(G.shape)} / X {tuple(X.shape)} must be matrices and W {tuple(W.shape)} an [E, N, K] tensor")
    E, N, K = (int(v) for v in W.shape)
    gr, xr = (plan.rows, plan.T) if mode == "gate_up" else (plan.T, plan.rows)
    if E != plan.E or tuple(G.shape) != (gr, N) or tuple(X.shape) != (xr, K) or G.stride(1) != 1 or X.stride(1) != 1:
        raise ValueError(f"moe_wgrad_rel[{mode}]: G {tuple(G.shape)} / X {tuple(X.shape)} must be [{gr}, {N}] / [{xr}, {K}] with contiguous rows "
                         f"for W {(E, N, K)} and a plan of {plan.T} tokens x {plan.k} slots over {plan.E} experts")
    pg, px = p(G), p(X)                 # (device tensors only: raises before anything is allocated)
    same(G, X)
    q, wp = _moe_w(G, W)
    if not q and not W.is_contiguous():
        raise ValueError("moe_wgrad_rel: W must be contiguous (the kernel reads the expert tensor as stored)")
    if mode == "down":
        if w is None or tuple(w.shape) != (plan.T, plan.k) or not w.is_contiguous():
            raise ValueError(f"moe_wgrad_rel[down]: w must be the contiguous routing weights [{plan.T}, {plan.k}]")
        same(G, w)
    if out is None:
        if accumulate:
            raise ValueError("moe_wgrad_rel: accumulate=True needs the out tensor to add to")
        out = torch.empty(E, N, K, device=G.device, dtype=torch.float32)
    f32(out)
    if tuple(out.shape) != (E, N, K) or not out.is_contiguous() or out.device != G.device or plan.buf.device != G.device:
        raise ValueError(f"moe_wgrad_rel: out must be a contiguous [{E}, {N}, {K}] float32 tensor on {G.device} (got {tuple(out.shape)} on "
                         f"{out.device}) and the plan must live there too")
    fn, name = (lib.lrp_moe_wgrad_rel_q, "lrp_moe_wgrad_rel_q") if q else (lib.lrp_moe_wgrad_rel, "lrp_moe_wgrad_rel")
    check(fn(pg, px, *wp, p(w) if mode == "down" else None, p(plan.buf), p(out), plan.T, plan.k, E, N, K, G.stride(0), X.stride(0),
             MOE_WGRAD_MODES[mode], int(bool(accumulate)), dt(G), stream()), name)
    return out


# ------------------------------------------------------------------------------------------- MoE router (csrc/moe_router.hip)
ROUTER_EMAX, ROUTER_KMAX = 1024, 16


def _router_rows(name, t, what, cols=None):
    """a [T, cols] activation operand of the router kernels: 2-D, unit column stride (a row pitch is allowed), float32 or bfloat16"""
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name}: {what} must be [T, {cols if cols is not None else 'E'}], got {tuple(t.shape)}")
    if t.stride(1) != 1:
        raise ValueError(f"{name}: {what} must have contiguous rows (a row pitch is allowed)")
    if t.dtype not in _DT:
        raise ValueError(f"{name}: {what} must be float32 or bfloat16, got {t.dtype}")


def _router_slots(name, ref, T, k, idx, **acts):
    """idx int64 [T, k] and the [T, k] activation operands next to it, all contiguous"""
    if tuple(idx.shape) != (T, k) or idx.dtype != torch.int64 or not idx.is_contiguous():
        raise ValueError(f"{name}: idx must be a contiguous int64 [{T}, {k}] tensor, got {idx.dtype} {tuple(idx.shape)}")
    for what, t in acts.items():
        if tuple(t.shape) != (T, k) or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous [{T}, {k}] tensor, got {tuple(t.shape)}")
        if t.dtype != ref.dtype:
            raise ValueError(f"{name}: {what} is {t.dtype} next to {ref.dtype} activations")


def moe_router_fwd(logits, k, norm_topk):
    """HF's Qwen3MoeTopKRouter after its F.linear, on the device: logits [T, E] (a row pitch is allowed) -> (idx int64 [T, k],
    w [T, k] in the logits' dtype, lse fp32 [T]); fp32 softmax, top-k (ties to the lower index), optional renorm, one rounding"""
    _router_rows("lrp_moe_router_fwd", logits, "logits")
    T, E = logits.shape
    k = int(k)
    if not (1 <= k <= min(E, ROUTER_KMAX)) or E > ROUTER_EMAX:
        raise ValueError(f"lrp_moe_router_fwd: k = {k} of E = {E} experts; the kernel serves k <= {ROUTER_KMAX}, k <= E <= {ROUTER_EMAX}")
    idx = torch.empty(T, k, device=logits.device, dtype=torch.int64)
    w = torch.empty(T, k, device=logits.device, dtype=logits.dtype)
    lse = torch.empty(T, device=logits.device, dtype=torch.float32)
    check(lib.lrp_moe_router_fwd(p(logits), p(idx), p(w), p(lse), T, E, k, logits.stride(0), int(bool(norm_topk)), dt(logits), stream()),
          "lrp_moe_router_fwd")
    return idx, w, lse


def moe_router_bwd(logits, lse, idx, w, gw, norm_topk, out=None):
    """-> G_logits [T, E] in the logits' dtype, dense (zeros where no gradient arrives): the exact backward of moe_router_fwd given
    G_w [T, k] (what moe_down_dgrad returns).  w, the forward's rounded routing weights, is part of the C signature and is checked like the
    other operands, but the kernel does NOT read it: the renorm's backward needs the fp32 weight p[i_s] / V that autograd holds, which it
    recomputes from logits and lse"""
    _router_rows("lrp_moe_router_bwd", logits, "logits")
    T, E = logits.shape
    if idx.dim() != 2:
        raise ValueError(f"lrp_moe_router_bwd: idx must be [T, k], got {tuple(idx.shape)}")
    k = idx.shape[1]
    _router_slots("lrp_moe_router_bwd", logits, T, k, idx, w=w, G_w=gw)
    if tuple(lse.shape) != (T,) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError(f"lrp_moe_router_bwd: lse must be a contiguous float32 [{T}] tensor, got {lse.dtype} {tuple(lse.shape)}")
    if not (1 <= k <= min(E, ROUTER_KMAX)) or E > ROUTER_EMAX:
        raise ValueError(f"lrp_moe_router_bwd: k = {k} of E = {E} experts; the kernel serves k <= {ROUTER_KMAX}, k <= E <= {ROUTER_EMAX}")
    if out is None:
        out = torch.empty(T, E, device=logits.device, dtype=logits.dtype)
    else:
        _router_rows("lrp_moe_router_bwd", out, "out", E)
        if out.shape[0] != T or out.dtype != logits.dtype:
            raise ValueError(f"lrp_moe_router_bwd: out must be [{T}, {E}] {logits.dtype}, got {tuple(out.shape)} {out.dtype}")
    check(lib.lrp_moe_router_bwd(p(logits), p(lse), p(idx), p(w), p(gw), p(out), T, E, k, logits.stride(0), out.stride(0),
                                 int(bool(norm_topk)), dt(logits), stream()), "lrp_moe_router_bwd")
    return out


def moe_expert_relevance(idx, w, gw, B, S, E, out=None):
    """-> fp32 [B, E]: out[b, e] = sum over prompt b's tokens and slots with idx = e of w G_w (a slot index outside [0, E) is skipped)"""
    if idx.dim() != 2 or idx.shape[0] != B * S:
        raise ValueError(f"lrp_moe_expert_relevance: idx must be [B S = {B * S}, k], got {tuple(idx.shape)}")
    k = idx.shape[1]
    if w.dtype not in _DT:
        raise ValueError(f"lrp_moe_expert_relevance: w must be float32 or bfloat16, got {w.dtype}")
    _router_slots("lrp_moe_expert_relevance", w, B * S, k, idx, w=w, G_w=gw)
    if not (1 <= k <= min(E, ROUTER_KMAX)) or E > ROUTER_EMAX:
        raise ValueError(f"lrp_moe_expert_relevance: k = {k} of E = {E} experts; the kernel serves k <= {ROUTER_KMAX}, k <= E <= {ROUTER_EMAX}")
    if out is None:
        out = torch.empty(B, E, device=w.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, E) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"lrp_moe_expert_relevance: out must be a contiguous float32 [{B}, {E}] tensor, got {out.dtype} {tuple(out.shape)}")
    check(lib.lrp_moe_expert_relevance(p(idx), p(w), p(gw), p(out), B, S, k, E, dt(w), stream()), "lrp_moe_expert_relevance")
    return out


# ------------------------------------------------------------------------------------- MXFP4 weights
MX_BLOCK = 32            # elements per e8m0 scale (include/lrp_hip_mxfp4.h)


def _mx_matrix(name, t, what):
    """the un-quantised side of the MXFP4 pair: [rows, cols] float32 / bfloat16 on the device, unit column stride (a row pitch is allowed)"""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: lrp_hip kernels need device tensors (no CPU fallback)")
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype not in _DT:
        raise ValueError(f"{name}: {what} must be a 2-D float32 / bfloat16 matrix with contiguous rows, got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] < 1 or t.shape[1] < MX_BLOCK or t.shape[1] % MX_BLOCK:
        raise ValueError(f"{name}: {what} is {tuple(t.shape)}; the blocks run along the columns, which must be a multiple of {MX_BLOCK}")


def _mx_bytes(name, t, what, rows, cols, ref):
    """codes [rows, cols / 2] / scales [rows, cols / 32]: uint8 on ref's device, unit column stride (a row pitch is allowed)"""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: lrp_hip kernels need device tensors (no CPU fallback)")
    if t.dtype != torch.uint8 or tuple(t.shape) != (rows, cols) or t.stride(1) != 1 or t.device != ref.device:
        raise ValueError(f"{name}: {what} must be uint8 [{rows}, {cols}] with contiguous rows on {ref.device}, got {t.dtype} {tuple(t.shape)} "
                         f"on {t.device}")


def mxfp4_quantize(w, codes=None, scales=None):
    """w [rows, cols] (float32 / bfloat16, cols % 32 == 0; a row pitch is allowed) -> (codes uint8 [rows, cols / 2], scales uint8
    [rows, cols / 32]): OCP MXFP4, e2m1 codes (two per byte, low nibble first) and one e8m0 scale per 32 elements along the columns;
    round-to-nearest, ties to the even code (include/lrp_hip_mxfp4.h states the format in full)"""
    name = "lrp_mxfp4_quantize"
    _mx_matrix(name, w, "w")
    rows, cols = w.shape
    if codes is None:
        codes = torch.empty(rows, cols // 2, device=w.device, dtype=torch.uint8)
    if scales is None:
        scales = torch.empty(rows, (cols // MX_BLOCK + 3) // 4 * 4, device=w.device, dtype=torch.uint8)[:, : cols // MX_BLOCK]      # (pitch on the 4-byte grid)
    _mx_bytes(name, codes, "codes", rows, cols // 2, w)
    _mx_bytes(name, scales, "scales", rows, cols // MX_BLOCK, w)
    check(lib.lrp_mxfp4_quantize(p(w), p(codes), p(scales), rows, cols, w.stride(0), codes.stride(0), scales.stride(0), dt(w), stream()), name)
    return codes, scales


def mxfp4_dequant(codes, scales, out):
    """out [rows, cols] (float32 / bfloat16; a row pitch is allowed) <- the matrix codes [rows, cols / 2] / scales [rows, cols / 32] hold;
    every value is exact in both types"""
    name = "lrp_mxfp4_dequant"
    _mx_matrix(name, out, "out")
    rows, cols = out.shape
    _mx_bytes(name, codes, "codes", rows, cols // 2, out)
    _mx_bytes(name, scales, "scales", rows, cols // MX_BLOCK, out)
    check(lib.lrp_mxfp4_dequant(p(codes), p(scales), p(out), rows, cols, codes.stride(0), scales.stride(0), out.stride(0), dt(out), stream()),
          name)
    return out


def _mx_stream_operands(name, x2, codes, scales):
    """the operands of the weight-streaming Linear on codes: device tensors, x2 a 2-D matrix, codes / scales uint8 [N, K / 2] / [N, K / 32]"""
    for t in (x2, codes, scales):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: lrp_hip kernels need device tensors (no CPU fallback)")
    if x2.dim() != 2 or x2.stride(1) != 1 or x2.dtype not in _DT:
        raise ValueError(f"{name}: x must be a 2-D float32 / bfloat16 matrix with contiguous rows, got {x2.dtype} {tuple(x2.shape)}")
    K = x2.shape[1]
    if K < MX_BLOCK or K % MX_BLOCK or codes.dim() != 2:
        raise ValueError(f"{name}: x is {tuple(x2.shape)}, codes {tuple(codes.shape)}; K must be a multiple of {MX_BLOCK}")
    _mx_bytes(name, codes, "codes", codes.shape[0], K // 2, x2)
    _mx_bytes(name, scales, "scales", codes.shape[0], K // MX_BLOCK, x2)


STREAM_Q = True          # module attribute (A/B measurements): False = no Linear reads MXFP4 codes in place (dequantise, then the bf16 kernels)


def linear_stream_q_ok(x2, codes, scales):
    """does lrp_linear_stream_fwd_q (the weight-streaming forward reading MXFP4 codes / scales directly) serve z = x2 D^T?  linear_stream_ok on
    the dequantised shape -- bf16, M <= 128 rows, K % 512 == 0, enough workgroups, the STREAM_FWD / STREAM_FWD_SPLITS switches -- and the
    format's pitch / alignment rules"""
    _mx_stream_operands("lrp_linear_stream_q_ok", x2, codes, scales)
    if not STREAM_FWD or not STREAM_Q or x2.dtype != torch.bfloat16:
        return False
    if x2.data_ptr() % 16 or codes.data_ptr() % 16 or scales.data_ptr() % 4:
        return False
    M, K, N = x2.shape[0], x2.shape[1], codes.shape[0]
    if not lib.lrp_linear_stream_q_ok(M, N, K, x2.stride(0), codes.stride(0), scales.stride(0)):
        return False
    return bool(STREAM_FWD_SPLITS or lib.lrp_linear_stream_fwd_splits(M, N, K) == 1)


def linear_stream_fwd_q(x2, codes, scales, bias=None, out=None, out_dtype=None):
    """z[M,N] = x2[M,K] @ D[N,K]^T (+ bias), D = the matrix codes / scales hold (mxfp4_dequant), in ONE launch that reads the codes: bit for
    bit mxfp4_dequant into bf16 followed by linear_stream_fwd (include/lrp_hip_mxfp4_stream.h)"""
    name = "lrp_linear_stream_fwd_q"
    _mx_stream_operands(name, x2, codes, scales)
    M, K = x2.shape
    N = codes.shape[0]
    out, ws, tk = _stream_fwd_buffers(x2, N, out, out_dtype)
    check(lib.lrp_linear_stream_fwd_q(p(x2), p(codes), p(scales), p(aux(bias, x2, N)), p(out), M, N, K, x2.stride(0), codes.stride(0),
                                      scales.stride(0), out.stride(0), dt(x2), _DT[out.dtype], p(ws), p(tk), stream()), name)
    return out
