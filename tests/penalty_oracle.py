"""numpy restatement of include/lrp_hip_penalty.h, written from the header's definition: the history table (bit 31 = the column occurs in
the prompt, bits 0..30 = how often it was generated) and the four steps of lrp_logit_penalty.  Two evaluations of one sequence of operations:
fp32, every operation individually rounded, which the kernel must equal bit for bit; and fp64, which is compared with HF's
RepetitionPenaltyLogitsProcessor (HF has no presence / frequency processor: those two steps are the stated formula only)."""
import numpy as np

SEEN = -2 ** 31          # bit 31 of an int32
CMAX = 2 ** 31 - 1


def hist_init(ids, lo, V):
    """ids int [B, S], lo [B] or None -> int32 [B, V]: SEEN at ids[b, s] for s >= lo[b]; an id outside [0, V) is skipped"""
    ids = np.asarray(ids)
    B, S = ids.shape
    hist = np.zeros((B, V), np.int32)
    for b in range(B):
        for s in range(0 if lo is None else max(int(lo[b]), 0), S):
            if 0 <= int(ids[b, s]) < V:
                hist[b, int(ids[b, s])] = SEEN
    return hist


def bump(hist, last):
    """the count of column last[b] goes up by one (saturating); a value outside [0, V) is ignored.  In place; -> hist"""
    if last is not None:
        for b, j in enumerate(np.asarray(last).tolist()):
            if 0 <= j < hist.shape[1] and (int(hist[b, j]) & CMAX) != CMAX:
                hist[b, j] += 1
    return hist


def penalise(logits, hist, rp=1.0, pp=0.0, fp=0.0, bias=None, dtype=np.float32):
    """the header's steps 1-4 on logits [B, V] with the table as it stands (bump first for `last`), every operation rounded to dtype"""
    f = dtype
    x = np.array(logits, dtype=f)
    hist = np.asarray(hist, dtype=np.int32)
    c = hist & np.int32(CMAX)
    gen = c > 0
    with np.errstate(all="ignore"):
        if f(rp) != f(1.0):
            hit = hist != 0
            x = np.where(hit, np.where(x < 0, x * f(rp), x / f(rp)), x).astype(f)
        t = (f(fp) * c.astype(f)).astype(f)
        x = np.where(gen, (x - t).astype(f), x)
        x = np.where(gen, (x - f(pp)).astype(f), x)
        if bias is not None:
            x = (x + np.asarray(bias, dtype=f)[None]).astype(f)
    return x.astype(f)


def step(logits, hist, last=None, **kw):
    """one lrp_logit_penalty call: bump (in place), then penalise"""
    return penalise(logits, bump(hist, last), **kw)
