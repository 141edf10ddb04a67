"""The definition of lrp_sample_rows (include/lrp_hip_sample.h) restated in numpy, written from the definition and not
from the kernel: Philox4x32-10 on Python integers, the kept set of temperature / top-k / top-p / min-p on a row of logits, and the inverse-CDF
draw.  dtype=np.float64 is the reference; dtype=np.float32 is the same text evaluated in the kernel's number format, which gives the
distance an fp32 evaluation has from the reference on its own.  temperature, top_p and min_p pass through float32 first: the C ABI carries
them as floats, so that is the value the kernel is given."""
import math

import numpy as np

M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
KNOWN_ANSWER_ZERO = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)          # Random123's vector for key 0, counter 0


def philox4x32_10(key, counter):
    """key (k0, k1), counter (c0, c1, c2, c3) -> four 32-bit words; ten rounds, the key bumped between rounds"""
    k0, k1 = key
    c0, c1, c2, c3 = counter
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def uniform(seed, step, stream=0):
    """the uniform of (seed, stream) at new token `step`: (word 0 >> 8) 2^-24 in [0, 1), exact in float32"""
    seed &= (1 << 64) - 1
    return (philox4x32_10((seed & MASK, seed >> 32), (step, stream, 0, 0))[0] >> 8) * 2.0 ** -24


def streams_of(seed, B):
    """generate(seed=...) -> [(seed_b, stream_b)]: an int gives (seed, b), a list gives (seed[b], 0)"""
    return [(seed, b) for b in range(B)] if isinstance(seed, int) else [(s, 0) for s in seed]


def sample_row(l, u, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, dtype=np.float64, margin=1e-4):
    """one row -> dict(token, n_kept, kept (bool [V]), logprob = log(q_tok / Z), probs (kept q / Z), near: the case sits within `margin` of a
    boundary -- u within margin of an INNER end of its token's CDF interval (as a fraction of Z; 0 and Z themselves are no boundary between
    two tokens), or the top-p boundary mass within margin Z_k of top_p Z_k)"""
    f = dtype
    T, top_p, min_p = f(np.float32(temperature)), f(np.float32(top_p)), f(np.float32(min_p))
    l = np.asarray(l).astype(f)
    V, lmax = l.shape[0], l.max()
    with np.errstate(invalid="ignore"):
        q = np.exp((l - lmax) / T)
    kept, near = np.ones(V, dtype=bool), False
    if 1 <= top_k < V:
        kept &= l >= np.partition(l, V - top_k)[V - top_k]
    if top_p < 1:
        vals, inv = np.unique(l[kept], return_inverse=True)                       # ascending distinct values of the top-k set
        mass = np.bincount(inv, weights=q[kept].astype(np.float64), minlength=len(vals)).astype(f)[::-1]      # per value, largest first
        zk = q[kept].sum(dtype=f)
        above = np.concatenate((np.zeros(1, f), np.cumsum(mass, dtype=f)[:-1]))      # mass of the strictly larger kept values
        keep_v = above < top_p * zk
        keep_v[0] = True
        near |= bool((np.abs(above[1:] - top_p * zk) <= margin * zk).any())
        kept &= l >= vals[::-1][keep_v].min()
    if min_p > 0:
        kept &= l >= lmax + T * f(math.log(min_p))
    qk = np.where(kept, q, f(0))
    c = np.cumsum(qk, dtype=f)
    Z = c[-1]
    hit = np.nonzero(kept & (c > (f(0) if top_k == 1 else f(u)) * Z))[0]
    tok = int(hit[0]) if len(hit) else int(np.nonzero(kept)[0][-1])
    lo, hi = (c[tok] - qk[tok]) / Z, c[tok] / Z
    if top_k != 1:
        near |= bool((lo > 0 and abs(u - lo) <= margin) or (c[tok] < Z and abs(hi - u) <= margin))
    return dict(token=tok, n_kept=int(kept.sum()), kept=kept, logprob=float(np.log(qk[tok] / Z)), probs=(qk / Z).astype(np.float64), near=near)


def sample_rows(logits, u, **kw):
    """rows [B, V], u [B] -> the list of sample_row's dicts"""
    return [sample_row(row, float(ub), **kw) for row, ub in zip(np.asarray(logits), np.asarray(u))]
