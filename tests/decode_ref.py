"""What the decode-kernel tests share (test_decode_kernels_gpu.py, test_decode_site_gpu.py, test_decode_edges_gpu.py): the fp64 restatement of
single-query attention over a KV cache, the case builder that poisons every cache row outside the live interval with NaN, and the bars."""
import torch

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
# fp32: the project's fp32 bar at a small multiple of the accumulation noise (fp32 sums in a fixed blocked order: ~1e-6 at 8000 keys).  bf16:
# against fp64 on the bf16-ROUNDED operands the only rounding between the fp32 accumulators and the store is one bf16 rounding, 2^-9; twice that
# 
BAR = {"fp32": 1e-5, "bf16": 2.0 ** -8}


def bits(t):
    """the storage bits of a tensor: NaN sentinels compare equal to themselves"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def reference(q, kc, vc, lo, n, Hq, Hkv, d, scale):
    """fp64 softmax attention of one query row per (prompt, head) over keys lo[b] .. n - 1 of the (already rounded) operands -> [B, Hq d]"""
    B, rep = q.shape[0], Hq // Hkv
    out = torch.zeros(B, Hq, d, dtype=torch.float64)
    q64 = q.double().cpu().reshape(B, Hkv, rep, d)
    for b in range(B):
        l0 = min(max(int(lo[b]), 0), n - 1)
        k = kc[b, l0:n, : Hkv * d].double().cpu().reshape(n - l0, Hkv, d)          # (query head h reads kv head h // rep)
        v = vc[b, l0:n, : Hkv * d].double().cpu().reshape(n - l0, Hkv, d)
        p = torch.softmax(scale * torch.einsum("grd,jgd->grj", q64[b], k), -1)
        out[b] = torch.einsum("grj,jgd->grd", p, v).reshape(Hq, d)
    return out.view(B, Hq * d)


def live_rows(dtype, B, n, Hq, Hkv, d, seed):
    """q [B, Hq d], k, v [B, n, Hkv d], rounded to the storage type, on the host"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq * d, generator=g).to(dtype)
    k = torch.randn(B, n, Hkv * d, generator=g).to(dtype)
    v = torch.randn(B, n, Hkv * d, generator=g).to(dtype)
    return q, k, v


def poisoned_cache(x, cap, lo, pad=0):
    """rows lo[b] .. n - 1 of x [B, n, cols] in the first cols columns of a NaN-filled [B, cap, cols + pad] device buffer"""
    B, n, cols = x.shape
    c = torch.full((B, cap, cols + pad), float("nan"), dtype=x.dtype)
    for b in range(B):
        c[b, lo[b]:n, :cols] = x[b, lo[b]:]
    return c.to(DEV)


def make_case(dtype, B, n, cap, Hq, Hkv, d, lo, seed):
    """operands with every cache row outside [lo[b], n - 1] NaN; the same live rows whatever cap is"""
    q, k, v = live_rows(dtype, B, n, Hq, Hkv, d, seed)
    return q.to(DEV), poisoned_cache(k, cap, lo), poisoned_cache(v, cap, lo)
