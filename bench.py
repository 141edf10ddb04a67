#!/usr/bin/env python3
"""bench.py -- explanations/sec of the full AttnLRP pass (forward + LRP backward + read-out) on a
Llama-3-8B-shaped model, seq=2048, synthetic data, on N MI355X of one node.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 launched through
torch.distributed.run with one rank per GPU.  A "step" = every rank explains `--batch` prompts of
`--seq` tokens (weak scaling: per-GPU work fixed).  Rank 0 prints ONE JSON line.

  value        whole-job explanations/s = N * batch * K / max-over-ranks(time of K steps); inputs
               (ids, weights) are resident in HBM before the timed region.
  roofline     dominant kernel = the plain instantiations of the 8-wave ping-pong GEMM (gemm_pp_kernel<bf16, NT | NN, EPI 0>: Linear
               forward z = x W^T and eps-rule dgrad c = s W from the stored weight; 6 of the 8 GEMM launches per layer): achieved
               = sum over its launches of 2*M*N*K divided by the sum of their durations, both taken live with HIP events on the
               launching stream inside the timed region; peak = 2500 TFLOP/s (dense bf16 MFMA, MI355X_MICROARCH.md).  The two
               launches per layer that carry a gated-MLP rule in their epilogue are other instantiations (separate rows in the
               rocprofv3 summary) and are listed under roofline.with_fused_epilogue_launches.
  cpu_baseline the oracle (CPU port of the same op sequence, oracle/llama.py) timed on this box's
               host cores on a bounded sample (one decoder layer + head, fp32, extrapolated x32);
               rank 0, N=1, --full only.

A plain run does what `value` needs and no more: set-up, warm-up, the timed steps, --dump-outputs, the line (value, ms_per_step and the
roofline of the GEMM launches inside the timed region).  `--full` adds, after and outside the timed region, everything that takes runs of
its own: cpu_baseline, the small-M Linear tables (roofline_linear_eps_smallm), seq = 4096 (config5_seq4096), the explicit placement and
4 / 1 prompts per step (mode_explicit, batch4, batch1), the Gemma-3-4B probes (config4_*) and the HF model under monkey_patch
(dropin_monkey_patch); the timed region and the headline keys are the same in both.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

LLAMA3_8B = dict(hidden=4096, inter=14336, n_layers=32, n_heads=32, n_kv=8, head_dim=128, vocab=128256,
                 rope_theta=500000.0, rms_eps=1e-5, act="silu")


def synth_weights(cfg, device, dtype, seed=0, allocate_only=False):
    """HF-default-style random init N(0, 0.02), generated directly on the device (no checkpoint,
    no network).  allocate_only: the same tensors UNINITIALISED -- what every rank but 0 of a multi-GPU run holds before the broadcast
    delivers rank 0's replica (nothing is synthesised twice)."""
    g = torch.Generator(device=device).manual_seed(seed)
    H, I, d, nq, nk, V = cfg["hidden"], cfg["inter"], cfg["head_dim"], cfg["n_heads"], cfg["n_kv"], cfg["vocab"]

    def rn(*s):
        if allocate_only:
            return torch.empty(*s, device=device, dtype=dtype)
        return (torch.randn(*s, generator=g, device=device, dtype=torch.float32) * 0.02).to(dtype)

    W = dict(embed=rn(V, H), norm=torch.ones(H, device=device, dtype=dtype), lm_head=rn(V, H), layers=[])
    for _ in range(cfg["n_layers"]):
        W["layers"].append(dict(ln1=torch.ones(H, device=device, dtype=dtype), ln2=torch.ones(H, device=device, dtype=dtype),
                                wq=rn(nq * d, H), wk=rn(nk * d, H), wv=rn(nk * d, H), wo=rn(H, nq * d),
                                wg=rn(I, H), wu=rn(I, H), wd=rn(H, I)))
    return W


def pin_host(local_rank, world):
    """One process per GPU: give every rank its own contiguous block of the host's logical CPUs and size torch's intra-op pool to it (N ranks
    would otherwise each start a pool of ALL cores and migrate over the box while each issues ~1500 launches per explanation).  No-op for a
    single process.  -> {"cpus": logical CPUs visible to this rank, "threads": torch.get_num_threads()}"""
    try:
        avail = sorted(os.sched_getaffinity(0))
    except AttributeError:
        avail = list(range(os.cpu_count() or 1))
    if world > 1 and len(avail) >= world:
        k = len(avail) // world
        mine = avail[local_rank * k: (local_rank + 1) * k]
        try:
            os.sched_setaffinity(0, mine)
        except (AttributeError, OSError):
            mine = avail
        torch.set_num_threads(max(1, min(len(mine), 16)))
        avail = mine
    return {"cpus": len(avail), "threads": torch.get_num_threads()}


def cpu_baseline(cfg, S, layers=4):
    """the oracle (CPU port of the reference's op sequence: oracle/llama.py, pinned against the imported reference) timed on the host cores:
    `layers` decoder layers + the last-token head of the same shape, forward and LRP backward timed separately, in bf16 (the GPU line's dtype and
    the dtype of the reference's own CPU number) after a one-layer warm-up; extrapolated to the full depth (every layer costs the same).  fp32
    (the oracle's parity dtype) on one layer beside it.  About 30 s of CPU work.  Also carried: what the REAL `lxt.efficient` measured in the
    build container (8 vCPU, bf16) -- the reference itself does not travel to the GPU box."""
    from oracle import llama as ol
    L = cfg["n_layers"]
    cL = dict(cfg, n_layers=min(layers, L))
    W = ol.random_weights(cL, seed=0)
    ids = torch.randint(0, cL["vocab"], (S,), generator=torch.Generator().manual_seed(1234))
    threads = torch.get_num_threads()

    def timed(c, dt):
        Wd = ol.cast_weights(dict(W, layers=W["layers"][: c["n_layers"]]), dt)
        t0 = time.time()
        cache = ol.forward(c, Wd, Wd["embed"][ids])
        t1 = time.time()
        ol.backward(c, Wd, cache, int(cache["logits_last"].argmax()), "efficient")
        return t1 - t0, time.time() - t1
    out = dict(unit="explanations/s", cores=threads, host_logical_cpus=os.cpu_count(), kind="port",
               reference_measured_in_build_container=dict(value=0.0275, unit="explanations/s", cores=8, dtype="bf16",
                                                          what="the real lxt.efficient (monkey_patch(modeling_llama), sdpa) on the Llama-3-8B "
                                                               "shape at S=2048, median of 3 warm runs, 8 vCPU Xeon 2.1 GHz (BASELINE.md section 2)"))
    try:
        timed(dict(cL, n_layers=1), torch.bfloat16)                              # warm-up
        f, bk = timed(cL, torch.bfloat16)
        k = L / cL["n_layers"]
        out.update(value=1.0 / ((f + bk) * k), dtype="bf16",
                   sample=f"oracle/llama.py, {cL['n_layers']} of {L} decoder layers + last-token head at S={S}, bf16 (torch CPU bf16 matmuls), "
                          f"{threads} threads: forward {f:.2f} s + LRP backward {bk:.2f} s measured, extrapolated x{k:g}")
    except Exception as e:  # noqa: BLE001  (a CPU build without bf16 kernels for some op)
        out.update(value=None, note=f"bf16 oracle pass failed on this host: {type(e).__name__}")
    f32, b32 = timed(dict(cL, n_layers=1), torch.float32)
    out["fp32"] = dict(value=1.0 / ((f32 + b32) * L), unit="explanations/s",
                       sample=f"1 of {L} layers + head in fp32 (the oracle's parity dtype): forward {f32:.2f} s + backward {b32:.2f} s, extrapolated x{L}")
    if out.get("value") is None:
        out["value"] = out["fp32"]["value"]
    return out


def _sha16(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def pmc_traffic():
    """HBM-side bytes per GEMM launch from the committed rocprofv3 PMC passes of this same command (FETCH_SIZE x2 gfx950 correction +
    WRITE_SIZE; tools/traffic.py -> profiles/r0N_gemm_traffic.json); PMC counters cannot be collected inside the timed run itself.
    The JSON is stamped with the hash of the kernel source it was measured on (`gemm_pp_sha16`): the newest file whose stamp matches
    the gemm_pp.hip of THIS tree is used; a stale measurement is reported as null (+ `traffic_note`), never as a number."""
    import glob
    want = _sha16(os.path.join(ROOT, "lrp-explains-transformers_amd", "csrc", "gemm_pp.hip"))
    stale = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_gemm_traffic.json")), reverse=True):
        try:
            with open(path) as f:
                d = json.load(f)
            if d.get("gemm_pp_sha16") == want:
                return float(d["traffic_bytes_per_launch"]), f"{os.path.basename(path)} (kernel source hash {want} matches)"
            stale = stale or os.path.basename(path)
        except Exception:  # noqa: BLE001
            continue
    return None, (f"no PMC measurement for gemm_pp.hip {want} (newest: {stale}, measured on another version of the kernel)" if stale
                  else "no PMC measurement committed")


def smallm_roofline(ops, dtype, device, cfg, batch):
    """secondary roofline: the Linear eps-rule in its HBM-bound regime (north star: ">= 60 % HBM roofline on the Linear eps-rule
    kernel"; SURVEY.md 8d: bf16 arithmetic intensity ~2 M FLOP/B, HBM-bound for M <~ 160 rows).  Everything is timed THROUGH THE PRODUCT
    DISPATCH (ops.linear_fwd / ops.linear_dgrad: the one-launch weight-streaming forward / dgrad kernels of linear_stream.hip, the W-streaming
    small-M kernels, the split-K skinny path of the ping-pong GEMM in its NT and NN forms -- W is read ONCE per direction from its stored
    layout, no W^T copy); the stabiliser is formed inside the dgrad kernel for M <= 16 (one 16-row block: beyond that its
    element-wise work outweighs the launch it saves, profiles/r04_call8_*.txt) and by a separate lrp_eps_scale launch above.  Headline entry = what explain() itself runs on its one-row-per-prompt path: the LM-head-sized Linear
    [vocab, hidden] at M = prompts per step.  `table` = M = 1 ... 160 on the gate/up-sized weight [14336, 4096] and on the LM head.
    Weights in the ENGINE's layout (round 5): row pitch off the 4-KiB grid as `LlamaLRP` stores them (engine.weight_pitch_pad / pitch_pad: +256 / +128
    bytes per row) -- with a pitch of exactly 8 KiB (28 KiB) the stream kernels ran 12-25 % slower (channel aliasing, bimodal with the allocation).
    Algorithmic bytes = sizeof * (N K + M K + M N) forward, sizeof * (N K + M K + 2 M N) backward; HIP events on the launching
    stream, 21 launches each, ROTATING through three distinct layer-sized weights (3 x 117 MB > the 256-MB Infinity Cache: the figure is
    an HBM figure); the LM head is 1.05 GB by itself."""
    g = torch.Generator(device=device).manual_seed(3)
    es = torch.empty(0, dtype=dtype).element_size()

    NROT = 3      # distinct weights rotated through the timing loop: 3 x 117 MB > the 256-MB Infinity Cache, so the figure is HBM, not L3

    def timed(fn):
        for i in range(3):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(21):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / 21

    def pair(M, N, K, Ws=None):
        x = torch.randn(M, K, generator=g, device=device).to(dtype)
        if Ws is None:
            Ws = [(torch.randn(N, K, generator=g, device=device) * K ** -0.5).to(dtype) for _ in range(NROT)]
        gg = torch.randn(M, N, generator=g, device=device).to(dtype)
        z = ops.linear_fwd(x, Ws[0])
        out = torch.empty(M, K, device=device, dtype=dtype)

        def fwd(i):
            return ops.linear_fwd(x, Ws[i % len(Ws)], out=z)

        def bwd(i):      # eps-rule redistribution c = (g z/(z+eps)) W
            W = Ws[i % len(Ws)]
            if M <= 16 and ops.linear_stream_dgrad_ok(gg, W):
                return ops.linear_stream_dgrad(gg, W, z=z, eps=1e-6, out=out)            # stabiliser fused into the MFMA weight-streaming dgrad
            if M <= 2:
                return ops.linear_smallm_dgrad(gg, W, z=z, eps=1e-6, out=out)            # stabiliser fused into the W stream (lane-local FMA kernel)
            return ops.linear_dgrad(ops.eps_scale(gg, z, 1.0, 1e-6), W, out=out)
        bwd(0)
        tf = timed(fwd)
        tb = timed(bwd)
        bf, bb = es * (N * K + M * K + M * N), es * (N * K + M * K + 2 * M * N)
        return dict(M=M, N=N, K=K, fwd_us=tf * 1e6, fwd_GBs=bf / tf / 1e9, dgrad_us=tb * 1e6, dgrad_GBs=bb / tb / 1e9,
                    pair_GBs=(bf + bb) / (tf + tb) / 1e9, pair_frac=(bf + bb) / (tf + tb) / 1e9 / 8000.0)

    M = min(batch, 256)
    import lxt_amd.engine as E_
    Wh = [(torch.randn(cfg["vocab"], cfg["hidden"], generator=g, device=device) * cfg["hidden"] ** -0.5).to(dtype)]      # 1.05 GB: beyond any cache
    head = pair(M, cfg["vocab"], cfg["hidden"], Wh)
    rows = (1, 2, 4, 8, 16, 32, 64, 128, 160)
    # layer-sized weights in the ENGINE's layout: stored-weight row pitch off the 4-KiB grid (engine.weight_pitch_pad: +256 bytes per row)
    padw = E_.weight_pitch_pad(cfg["hidden"], es, cfg["inter"])
    Wl = [(torch.randn(cfg["inter"], cfg["hidden"] + padw, generator=g, device=device) * cfg["hidden"] ** -0.5).to(dtype)[:, : cfg["hidden"]] for _ in range(NROT)]
    table = [pair(m, cfg["inter"], cfg["hidden"], Wl) for m in rows]
    del Wl
    # the down-projection's shape [4096, 14336], in the engine's layout: row pitch off the 4-KiB grid (engine.pitch_pad: +128 bytes per row)
    padc = E_.pitch_pad(cfg["inter"], es)
    Wd = [(torch.randn(cfg["hidden"], cfg["inter"] + padc, generator=g, device=device) * cfg["inter"] ** -0.5).to(dtype)[:, : cfg["inter"]] for _ in range(NROT)]
    table_down = [pair(m, cfg["hidden"], cfg["inter"], Wd) for m in rows]
    del Wd
    table_head = [pair(m, cfg["vocab"], cfg["hidden"], Wh) for m in rows]
    del Wh
    # the key's headline = the WORST forward + dgrad pair over M <= 32 on the two layer-sized weights (not the friendliest
    # shape); the LM head -- what explain() itself runs on its one-row-per-prompt path -- is a side field
    worst = min((t for t in table + table_down if t["M"] <= 32), key=lambda t: t["pair_frac"])
    return {"bound": "hbm", "kernel": "ops.linear_fwd + ops.linear_dgrad (Linear eps-rule incl. the stabiliser; W-streaming forward / dgrad kernels of "
                                      f"linear_stream.hip, split-K skinny path): worst pair over M <= 32 on W [{cfg['inter']},{cfg['hidden']}] and "
                                      f"[{cfg['hidden']},{cfg['inter']}] = M {worst['M']} on [{worst['N']},{worst['K']}]",
            "achieved": worst["pair_GBs"], "peak": 8000.0, "unit": "GB/s", "frac": worst["pair_frac"],
            "avg_launch_us": (worst["fwd_us"] + worst["dgrad_us"]) / 2, "traffic": None, "weights_rotated": NROT,
            "lm_head": dict(head, note=f"W [{cfg['vocab']},{cfg['hidden']}] (1.05 GB), M = {M}: the largest one-row-per-prompt Linear explain() runs"),
            "table_gate_up_sized": table, "table_down_sized": table_down, "table_lm_head": table_head}


def config5_probe(eng, ops, cfg, dev, peak, steps=3):
    """BASELINE config 5's per-GPU workload (Llama-3-8B, seq = 4096; the 1024-prompt job is sharded 128 prompts per GPU, explained here
    2 prompts per step) AFTER and OUTSIDE the headline timed region: explanations/s and the GEMM's roofline fraction at S = 4096."""
    S5, B5 = 4096, 2
    ids = torch.randint(0, cfg["vocab"], (B5 * (steps + 1), S5), generator=torch.Generator().manual_seed(4321)).to(dev)
    R = eng.explain(ids[:B5])["R_tok"]
    torch.cuda.synchronize()
    timer = ops.KernelTimer()
    ops.GEMM_TIMER = timer
    t0 = time.perf_counter()
    for i in range(steps):
        R = eng.explain(ids[(i + 1) * B5: (i + 2) * B5])["R_tok"]
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ops.GEMM_TIMER = None
    n_launch, flops, secs = timer.summary()
    assert torch.isfinite(R).all()
    return {"workload": f"seq={S5}, {B5} prompts per step, {steps} steps after the headline region (same engine, same weights)",
            "value": B5 * steps / el, "unit": "explanations/s", "ms_per_step": el / steps * 1e3,
            "gemm_TFLOPs": flops / secs / 1e12, "gemm_frac_of_peak": flops / secs / 1e12 / peak, "gemm_time_frac_of_step": secs / el}


def mode_batch_probes(eng, ops, cfg, dev, peak, S, steps=3, B=8):
    """driver-visible numbers for the OTHER rule placement and for fewer prompts per step, AFTER and OUTSIDE the headline region, same
    engine and weights: `mode_explicit` = lxt.explicit placement (every stabiliser of lxt/explicit/models/llama.py:83-93 live), the headline's
    prompts per step; `batch4` = 4 prompts per step (the headline's configuration until round 5); `batch1` = one prompt per step (M = S rows:
    the 128-tile GEMMs take the split-K path), eager and as one hipGraph."""
    def run(B, n, graph=False, mode=None):
        if mode is not None:
            eng.set_mode(mode)
        ids = torch.randint(0, cfg["vocab"], (B * (n + 1), S), generator=torch.Generator().manual_seed(777 + B)).to(dev)
        R = eng.explain(ids[:B], graph=graph)["R_tok"]
        torch.cuda.synchronize()
        timer = ops.KernelTimer()
        ops.GEMM_TIMER = None if graph else timer
        t0 = time.perf_counter()
        for i in range(n):
            R = eng.explain(ids[(i + 1) * B: (i + 2) * B], graph=graph)["R_tok"]
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        ops.GEMM_TIMER = None
        assert torch.isfinite(R).all()
        d = {"value": B * n / el, "unit": "explanations/s", "ms_per_step": el / n * 1e3, "prompts_per_step": B}
        if not graph:
            _, flops, secs = timer.summary()
            d.update(gemm_TFLOPs=flops / secs / 1e12, gemm_frac_of_peak=flops / secs / 1e12 / peak, gemm_time_frac_of_step=secs / el)
        return d
    out = {}
    try:
        out["mode_explicit"] = dict(run(B, steps, mode="explicit"), workload=f"lxt.explicit placement, seq={S}, {B} prompts per step")
    finally:
        eng.set_mode("efficient")
    if B != 4:
        out["batch4"] = dict(run(4, steps), workload=f"lxt.efficient placement, seq={S}, 4 prompts per step (the headline's configuration of rounds 1-5)")
    out["batch1"] = {"workload": f"lxt.efficient placement, seq={S}, ONE prompt per step", "eager": run(1, 2 * steps),
                     "graph": run(1, 2 * steps, graph=True)}
    return out


def config4_text_engine(dev, dtype, S4=2048, L=34):
    """Gemma-3-4B text tower shape (L layers of H 2560, 8 / 4 heads of d = 256, I 10240, window 1024 on 5 of 6 layers, tied 262208-token head),
    random init on the device -> (engine, generator, vocab)"""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    H, I, nq, nk, d, V = 2560, 10240, 8, 4, 256, 262208
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda sd, *s: (torch.randn(*s, generator=g, device=dev) * sd).to(dtype)  # noqa: E731
    inv = lambda theta, f: 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d)) / f  # noqa: E731
    cfg = dict(hidden=H, inter=I, n_layers=L, n_heads=nq, n_kv=nk, head_dim=d, vocab=V, rms_eps=1e-6, act="gelu_tanh", scale=256 ** -0.5,
               layer_types=[("full_attention" if (i + 1) % 6 == 0 else "sliding_attention") for i in range(L)], window=1024,
               rope={"sliding_attention": (inv(1e4, 1.0), 1.0), "full_attention": (inv(1e6, 8.0), 1.0)}, embed_scale=H ** 0.5)
    emb = rn(0.02, V, H)
    W = dict(embed=emb, lm_head=emb, norm=rn(0.1, H), layers=[
        dict(ln_in=rn(0.1, H), ln_pa=rn(0.1, H), ln_pf=rn(0.1, H), ln_pff=rn(0.1, H), qn=rn(0.1, d), kn=rn(0.1, d), wq=rn(0.02, nq * d, H),
             wk=rn(0.02, nk * d, H), wv=rn(0.02, nk * d, H), wo=rn(0.02, H, nq * d), wg=rn(0.02, I, H), wu=rn(0.02, I, H), wd=rn(0.02, H, I))
        for _ in range(L)])
    eng = Gemma3LRP(cfg, W, dtype=dtype, device=dev, max_seq=S4)
    del W, emb
    return eng, g, V


def config4_probe(ops, dev, dtype, peak, steps=3, B4=4, S4=2048, image=True):
    """BASELINE config 4's text tower through the fused Gemma-3 driver (lxt_amd.engine_gemma3.Gemma3LRP), AFTER and OUTSIDE the headline
    timed region: Gemma-3-4B shape (34 layers, H 2560, 8 / 4 heads of d = 256, I 10240, sliding window 1024 on 5 of 6 layers, tied
    262208-token head), random init on the device, seq = 2048, 4 prompts per step."""
    eng, g, V = config4_text_engine(dev, dtype, S4)
    ids = torch.randint(0, V, (B4 * (steps + 1), S4), generator=torch.Generator().manual_seed(99)).to(dev)
    R = eng.explain(ids[:B4])["R_tok"]
    torch.cuda.synchronize()
    timer = ops.KernelTimer()
    ops.GEMM_TIMER = timer
    t0 = time.perf_counter()
    for i in range(steps):
        R = eng.explain(ids[(i + 1) * B4: (i + 2) * B4])["R_tok"]
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ops.GEMM_TIMER = None
    n_launch, flops, secs = timer.summary()
    assert torch.isfinite(R).all()
    text = {"workload": f"Gemma-3-4B text tower shape, lxt.efficient rule placement, seq={S4}, {B4} prompts per step, {steps} steps after the "
                        "headline region (fused driver engine_gemma3.Gemma3LRP)",
            "value": B4 * steps / el, "unit": "explanations/s", "ms_per_step": el / steps * 1e3,
            "gemm_TFLOPs": flops / secs / 1e12, "gemm_frac_of_peak": flops / secs / 1e12 / peak, "gemm_time_frac_of_step": secs / el}
    mm = None
    if image:
        mm = config4_image_probe(eng, ops, dev, dtype, peak, g, steps=steps, B4=B4, S4=S4)
    eng.release()
    return text, mm


def config4_image_probe(text_eng, ops, dev, dtype, peak, g, steps=3, B4=4, S4=2048):
    """BASELINE config 4 as named: Gemma-3-4B-it IMAGE + TEXT.  One 896 x 896 image per prompt (SigLIP-So400m shape: 27 layers, H 1152, 16
    heads of d = 72, I 4304, 4096 patches -> 256 image tokens through the projector) inside a seq = 2048 prompt, relevance of the text tokens
    and of the 4096 ViT patches, through the fused driver engine_gemma3_mm.Gemma3MMLRP; random init on the device."""
    from lxt_amd.engine_gemma3_mm import Gemma3MMLRP, SiglipLRP
    Lv, Hv, Iv, nh, img, pt, T = 27, 1152, 4304, 16, 896, 14, 256
    Ht, V = text_eng.cfg["hidden"], text_eng.cfg["vocab"]
    rn = lambda sd, *s: (torch.randn(*s, generator=g, device=dev) * sd).to(dtype)  # noqa: E731
    P = (img // pt) ** 2
    W = dict(patch_w=rn(0.02, Hv, 3, pt, pt), patch_b=rn(0.02, Hv), pos=rn(0.02, P, Hv), post_w=1 + rn(0.1, Hv), post_b=rn(0.1, Hv),
             proj_norm=rn(0.1, Hv), proj_w=rn(0.03, Hv, Ht), layers=[
        dict(ln1_w=1 + rn(0.1, Hv), ln1_b=rn(0.1, Hv), ln2_w=1 + rn(0.1, Hv), ln2_b=rn(0.1, Hv), wq=rn(0.02, Hv, Hv), bq=rn(0.02, Hv),
             wk=rn(0.02, Hv, Hv), bk=rn(0.02, Hv), wv=rn(0.02, Hv, Hv), bv=rn(0.02, Hv), wo=rn(0.02, Hv, Hv), bo=rn(0.02, Hv),
             w1=rn(0.02, Iv, Hv), b1=rn(0.02, Iv), w2=rn(0.02, Hv, Iv), b2=rn(0.02, Hv)) for _ in range(Lv)])
    vcfg = dict(hidden=Hv, inter=Iv, n_layers=Lv, n_heads=nh, image=img, patch=pt, channels=3, ln_eps=1e-6, act="gelu_tanh",
                tokens_per_image=T, text_hidden=Ht, image_token_id=V - 1)
    vis = SiglipLRP(vcfg, W, dtype=dtype, device=dev, vision_attn_rule=True)
    del W
    eng = Gemma3MMLRP(text_eng, vis)
    ids = torch.randint(0, V - 8, (B4 * (steps + 1), S4), generator=torch.Generator().manual_seed(98))
    ids[:, 64: 64 + T] = V - 1                                                 # the image's 256 tokens inside the prompt
    pix = torch.randn(B4 * (steps + 1), 3, img, img, generator=g, device=dev).to(dtype)
    r = eng.explain(ids[:B4], pix[:B4])
    torch.cuda.synchronize()
    timer = ops.KernelTimer()
    ops.GEMM_TIMER = timer
    t0 = time.perf_counter()
    for i in range(steps):
        r = eng.explain(ids[(i + 1) * B4: (i + 2) * B4], pix[(i + 1) * B4: (i + 2) * B4])
    t_issue = time.perf_counter() - t0                                         # host time to ISSUE the steps (no arena / hipGraph in this driver)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ops.GEMM_TIMER = None
    n_launch, flops, secs = timer.summary()
    assert torch.isfinite(r["R_tok"]).all() and torch.isfinite(r["R_patch"]).all()
    return {"workload": f"Gemma-3-4B-it shape, image + text: one 896x896 image (SigLIP tower 27 layers, 4096 patches -> 256 image tokens) inside a "
                        f"seq={S4} prompt, {B4} prompts per step, {steps} steps; relevance of text tokens and ViT patches (fused driver "
                        "engine_gemma3_mm.Gemma3MMLRP, lxt.efficient placement, tower attention under the AttnLRP rule = the reference with sdpa)",
            "value": B4 * steps / el, "unit": "explanations/s", "ms_per_step": el / steps * 1e3,
            "gemm_TFLOPs_timed_launches": flops / max(secs, 1e-9) / 1e12, "gemm_time_frac_of_step": secs / el, "host_issue_frac_of_step": t_issue / el}


def dropin_probe(dev, S=2048, B=4, steps=3):
    """The DROP-IN path at the headline shape, after and outside the timed region: a HuggingFace LlamaForCausalLM at the Llama-3-8B dimensions
    (32 layers, random init on the device, bf16) under `lxt_amd.efficient.monkey_patch(modeling_llama)`, driven by autograd exactly as the
    reference's quickstart drives lxt.efficient (docs/source/quickstart.rst:120-141: inputs_embeds.requires_grad_(), logits[.., -1, idx]
    .backward(), (e * e.grad).sum(-1)); 4 prompts per step as one batch.  Round 6: every decoder layer of the adopted bf16 model is ONE autograd
    node on the engine's fused launch sequence (lxt_amd.efficient.patches.decoder_layer_forward / DecoderLayerFn); what the drop-in adds is HF's
    module graph, autograd bookkeeping, the final norm / LM head as separate modules and the torch allocator instead of the engine's arena."""
    import warnings
    from transformers import LlamaConfig, LlamaForCausalLM
    from transformers.models.llama import modeling_llama
    from lxt_amd.efficient import monkey_patch
    kw = dict(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8, vocab_size=128256,
              rms_norm_eps=1e-5, max_position_embeddings=8192, tie_word_embeddings=False, attn_implementation="sdpa")
    try:
        hcfg = LlamaConfig(rope_parameters=dict(rope_type="default", rope_theta=500000.0), **kw)
    except TypeError:
        hcfg = LlamaConfig(rope_theta=500000.0, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        monkey_patch(modeling_llama)
        torch.manual_seed(0)
        with torch.device(dev):
            model = LlamaForCausalLM(hcfg).to(torch.bfloat16).eval()
    for p_ in model.parameters():
        p_.requires_grad_(False)
    ids = torch.randint(0, 128256, (B * (steps + 1), S), generator=torch.Generator().manual_seed(77)).to(dev)
    rows = torch.arange(B, device=dev)

    def run(chunk):
        e = model.get_input_embeddings()(chunk).detach().requires_grad_()
        last = model(inputs_embeds=e, use_cache=False, logits_to_keep=1).logits[:, -1]
        last[rows, last.argmax(-1)].sum().backward()
        return (e * e.grad).float().sum(-1)
    R = run(ids[:B])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        R = run(ids[(i + 1) * B: (i + 2) * B])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    assert torch.isfinite(R).all()
    del model
    torch.cuda.empty_cache()
    return {"workload": f"HF LlamaForCausalLM (Llama-3-8B dims, 32 layers, bf16, random init) under lxt_amd.efficient.monkey_patch, autograd-driven "
                        f"(the reference's own protocol), seq={S}, {B} prompts per step, {steps} steps",
            "value": B * steps / el, "unit": "explanations/s", "ms_per_step": el / steps * 1e3}


def dry_run(args):
    """the N-rank control flow of main() with the explanation replaced by a pure function of the ids (no engine, no device):
    what torch.distributed.run + this script must get right before any kernel matters"""
    import lxt_amd.dist as D
    import torch.distributed as dist
    rank, world, local = D.init(backend="gloo")
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run"
    host = pin_host(local, world)
    B, S = args.batch, min(args.seq, 64)
    n_total = world * B
    ids_all = torch.randint(0, 1000, (n_total * (args.steps + args.warmup), S), generator=torch.Generator().manual_seed(1234))
    fake = lambda x: x.float().cumsum(1)                                    # noqa: E731

    def step(i):
        chunk = ids_all[i * n_total: (i + 1) * n_total]
        lo, hi = D.shard_range(n_total, rank, world)
        return D.gather_relevance(fake(chunk[lo:hi]), n_total)
    # the same start-up self-checks as the real run: zero the non-source replicas, broadcast, compare checksums; gather order
    flat = torch.arange(4096, dtype=torch.float32).to(torch.bfloat16) * (1.0 if rank == 0 else 0.0)
    D.broadcast_weights([flat], src=0)
    sums = D.check_replicas([flat])
    assert len(sums) == world and float(flat.float().abs().sum()) > 0.0
    D.check_gather_order(n_total, S, "cpu")
    for i in range(args.warmup):
        R = step(i)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        R = step(args.warmup + i)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    last = ids_all[(args.warmup + args.steps - 1) * n_total: (args.warmup + args.steps) * n_total]
    assert R.shape == (n_total, S) and torch.equal(R, fake(last)), "gathered relevance is not in global prompt order"
    per_rank = None
    if world > 1:
        mine = torch.tensor([elapsed, 0.0, float(host["threads"])], dtype=torch.float64)       # the same per-rank gather as the real run
        allr = torch.empty(world * 3, dtype=torch.float64)
        dist.all_gather_into_tensor(allr, mine)
        per_rank = [{"rank": r, "ms_per_step": e / args.steps * 1e3, "host_issue_frac": h / max(e, 1e-12), "host_threads": int(t)}
                    for r, (e, h, t) in enumerate(allr.view(-1, 3).tolist())]
        tmax = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax[0])
    if rank == 0:
        print(json.dumps({"metric": "explanations/sec (full AttnLRP backward) Llama-3-8B seq=2048", "value": None, "unit": "explanations/s",
                          "host": host, "per_rank": per_rank,
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
                          "dry_run": True, "config": {"workload": "dry run: control flow only, no kernels", "global_batch": n_total,
                                                      "parallelism": f"dp{world}"}}), flush=True)
    if world > 1:
        dist.destroy_process_group()


DUMP_BYTES = 63 << 20          # --dump-outputs: 64 MB in all, with room for the .npy headers


def dump_outputs(out_dir, out, n_total, write):
    """--dump-outputs: what explain() returned in the last timed step (R_tok, idx, logit, logits), every rank's prompts in global order (one
    all-gather per array, after the timed region), written by rank 0 as out_dir/<name>.npy -- float32, idx as float64 -- so that two builds
    can be compared output for output on the same seeded inputs.  An array beyond its share of DUMP_BYTES is replaced by a fixed, seeded
    sample of its elements (flattened, in index order)."""
    import numpy as np
    import lxt_amd.dist as D
    arrs = {}
    for name in ("R_tok", "idx", "logit", "logits"):
        a = out[name]
        a = D.gather_relevance(a.reshape(a.shape[0], -1).contiguous(), n_total).reshape(n_total, *a.shape[1:])
        arrs[name] = a.cpu().to(torch.float64 if name == "idx" else torch.float32)
    if not write:
        return
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_BYTES
    for i, (name, a) in enumerate(sorted(arrs.items(), key=lambda kv: kv[1].numel())):
        share = budget // (len(arrs) - i)
        if a.numel() * a.element_size() > share:
            pick = torch.randint(a.numel(), (share // a.element_size(),), generator=torch.Generator().manual_seed(0)).sort().values
            a = a.reshape(-1)[pick]
        np.save(os.path.join(out_dir, f"{name}.npy"), a.numpy())
        budget -= a.numel() * a.element_size()


def self_launch(n):
    """`python bench.py --gpus N` started bare (no RANK / WORLD_SIZE in the environment): become the launcher -- the same command the driver
    issues for N > 1, `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <argv>`,
    one rank per GPU over RCCL -- and hand its exit code back.  Rank 0's JSON line reaches this process's stdout unchanged."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    rc = subprocess.run(cmd, env=env).returncode
    if rc != 0:
        sys.exit(rc)


EXTRAS = ("cpu_baseline", "config5", "config4", "config4_image", "dropin", "extra_modes", "smallm")      # each has a --no-<name> option


def parse_args(argv=None):
    """the command line -> args.  Without --full every part of EXTRAS is switched off (args.no_<name> = True): a plain run sets up, warms
    up, times the steps and prints the line.  With --full each runs unless its own --no-<name> option drops it."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything else the benchmark knows, each in runs of its own and under a key of its "
                         "own in the result line: the small-M Linear tables, seq=4096, the explicit placement and 4 / 1 prompts per step, the "
                         "Gemma-3-4B probes, the HF model under monkey_patch, the CPU baseline (the --no-... options below drop one of them "
                         "each).  Off by default: a plain run does only what the headline value needs")
    ap.add_argument("--single-rank-collectives", action="store_true",
                    help="dev, 1 GPU: run the N > 1 code path (RCCL broadcast / self-checks / all-gather / barriers) with a one-rank process group")
    ap.add_argument("--per-step", action="store_true", help="dev: print per-step wall times to stderr (adds a full sync per step)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4, help="prompts per step per GPU (8 measures the same per prompt in one process -- 369.0 ms per 8 vs "
                                                            "183.9 ms per 4, round 6 -- so the headline keeps the configuration of rounds 1-5)")
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--mode", default="efficient", choices=["efficient", "explicit"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-config5", action="store_true", help="skip the seq=4096 probe that follows the headline region")
    ap.add_argument("--no-config4", action="store_true", help="skip the Gemma-3-4B text-tower probe that follows the headline region")
    ap.add_argument("--no-config4-image", action="store_true", help="skip the image + text part of the Gemma-3-4B probe")
    ap.add_argument("--no-dropin", action="store_true", help="skip the HF-model-under-monkey_patch probe that follows the headline region")
    ap.add_argument("--no-extra-modes", action="store_true", help="skip the explicit-mode and one-prompt-per-step probes that follow the headline region")
    ap.add_argument("--no-smallm", action="store_true", help="skip the small-M Linear tables that follow the headline region (profiling: their "
                    "launches carry the same kernel names as the step's GEMMs and would dilute the per-kernel averages)")
    ap.add_argument("--dense-top", action="store_true", help="disable the top-layer sparsity (A/B knob)")
    ap.add_argument("--unfused-gated", action="store_true", help="A/B knob: gated-MLP rules as separate kernels (ops.GATED_FUSION = False)")
    ap.add_argument("--no-rope-bwd-fusion", action="store_true", help="A/B knob: stand-alone rope_bwd pass (ops.ROPE_BWD_FUSION = False)")
    ap.add_argument("--no-prep-fusion", action="store_true", help="A/B knob: stand-alone attn_bwd_prep pass (ops.PREP_FUSION = False)")
    ap.add_argument("--norm-fusion-parts", default="", help="A/B knob: comma-separated subset of fwd,bwd_qkv,bwd_gu (ops.NORM_FUSION as a set)")
    ap.add_argument("--no-norm-fusion", action="store_true", help="A/B knob: RMSNorm / residual sums as stand-alone kernels (ops.NORM_FUSION = False)")
    ap.add_argument("--no-pitch-pad", action="store_true", help="A/B knob: no row-pitch padding of the long-K GEMM operands (engine.PITCH_PAD = False)")
    ap.add_argument("--graph", action="store_true", help="replay each step as one hipGraph (LlamaLRP.explain(graph=True)); pays at small batch")
    ap.add_argument("--dry-run", action="store_true",
                    help="plumbing self-test WITHOUT kernels or a GPU (gloo): rank env, sharding, barrier, max-over-ranks, gather, "
                         "one JSON line from rank 0 -- value is null; used by tests/test_dist_cpu.py for the N>1 launch contract")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed step's explain() returned "
                    "(R_tok, idx, logit, logits; all ranks' prompts) as DIR/<name>.npy in float32 / float64, at most 64 MB in all")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        for name in EXTRAS:
            setattr(args, "no_" + name, True)
    return args


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ and not args.single_rank_collectives:
        return self_launch(args.gpus)
    if args.dry_run:
        return dry_run(args)

    import lxt_amd.dist as D
    import lxt_amd.engine as E
    import lxt_amd.ops as ops
    import torch.distributed as dist

    ops.GATED_FUSION = not args.unfused_gated
    E.PITCH_PAD = not args.no_pitch_pad
    ops.PREP_FUSION = not args.no_prep_fusion
    ops.ROPE_BWD_FUSION = not args.no_rope_bwd_fusion
    if args.no_norm_fusion:
        ops.NORM_FUSION = False
    if args.norm_fusion_parts:
        ops.NORM_FUSION = frozenset(x for x in args.norm_fusion_parts.split(",") if x)
    rank, world, local = D.init()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    host = pin_host(local, world)
    # dev (a 1-GPU box): --single-rank-collectives sends the ONE-rank run through the N > 1 code path below -- an `nccl` process group of
    # world size 1, the world == 1 short cuts of lxt_amd.dist switched off: the same RCCL calls, buffers and dtypes as the 8-rank job
    coll = world > 1
    if args.single_rank_collectives and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group(backend="nccl", rank=0, world_size=1)
        D.SINGLE_RANK_COLLECTIVES = True
        coll = True
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    cfg = dict(LLAMA3_8B, n_layers=args.layers)

    W = synth_weights(cfg, dev, dtype, seed=0, allocate_only=(coll and rank != 0))
    eng = E.LlamaLRP(cfg, W, dtype=dtype, device=dev, mode=args.mode, max_seq=max(args.seq, 4096), sparse_top=not args.dense_top)
    del W
    torch.cuda.empty_cache()
    selfcheck = None
    if coll:
        # C1 of SURVEY.md 8e: ONE collective over the engine's flat weight buffer (forward layouts only, 16 GB) -- outside the timed region;
        # the dgrad GEMMs read the stored weights, so nothing is rebuilt (build_transposes only drops cached fp32 transposes).  SELF-CHECKING
        # (VERDICT r3): every rank but 0 ZEROES its replica first, so the ranks can only produce finite, equal results if the broadcast
        # really delivered rank 0's bytes; the per-rank byte checksums are all-gathered and must agree; and the job's all-gather is
        # exercised once with rank-tagged rows before the timed region (global prompt order, right owner)
        if rank != 0:
            eng.flat.zero_()
        t_b = time.perf_counter()
        D.broadcast_weights([eng.flat], src=0)
        torch.cuda.synchronize()
        t_b = time.perf_counter() - t_b
        sums = D.check_replicas([eng.flat])
        D.check_gather_order(world * args.batch * args.steps, args.seq, dev)
        eng.build_transposes()
        nbytes = eng.flat.numel() * eng.flat.element_size()
        selfcheck = {"broadcast_bytes": nbytes, "broadcast_s": t_b, "broadcast_GBps": nbytes / max(t_b, 1e-9) / 1e9,
                     "replica_checksums_equal": True, "checksum": sums[0] & 0xFFFFFFFF, "gather_order_checked": True,
                     "replicas_other_than_rank0": "allocated uninitialised, zeroed, then filled by the broadcast only"}

    B, S = args.batch, args.seq
    n_total = world * B
    gen = torch.Generator().manual_seed(1234)
    ids_all = torch.randint(0, cfg["vocab"], (n_total * (args.steps + args.warmup), S), generator=gen).to(dev)

    last = [None]                                           # explain()'s output of the latest step (--dump-outputs)

    def step(i):
        chunk = ids_all[i * n_total: (i + 1) * n_total]
        lo, hi = D.shard_range(n_total, rank, world)
        last[0] = eng.explain(chunk[lo:hi], graph=args.graph)
        r = last[0]["R_tok"]                                # this rank's shard; the all-gather (C2) is per JOB, below
        return r.clone() if args.graph else r

    for i in range(args.warmup):
        R = step(i)
    torch.cuda.synchronize()
    if coll:
        dist.barrier()
    timer = ops.KernelTimer()
    ops.GEMM_TIMER = timer
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    per_step = []
    done = []                                               # one marker event per step
    shards = []
    host_issue = 0.0                                        # seconds this rank's host thread spent ISSUING (inside explain(): ~1500 launches per step)
    for i in range(args.steps):
        t_i = time.perf_counter()
        shards.append(step(args.warmup + i))
        host_issue += time.perf_counter() - t_i
        ev = torch.cuda.Event()
        ev.record()
        done.append(ev)
        # bounded run-ahead: the host may be at most ONE step ahead of the device.  Unbounded, it queues K steps x ~1500
        # launches (+ two timing events per GEMM) and the HIP runtime's signal pool / queue back-pressure turns into
        # a slow path in some processes (measured: 250 -> 400-650 ms per step, erratic); with the bound the device
        # never idles (the next step is already queued) and the step time is reproducible.
        if i >= 1:
            done[i - 1].synchronize()
            timer.drain()                                   # fold the finished step's GEMM spans, re-use their events (ops.KernelTimer)
        if args.per_step:                                   # dev: per-step wall times (adds a full sync per step)
            torch.cuda.synchronize()
            per_step.append(time.perf_counter() - t0)
    # C2: ONE all-gather of the job's [steps * prompts_per_rank, S] fp32 token relevances, inside the timed region
    R = D.gather_relevance(torch.cat(shards, 0), n_total * args.steps)
    torch.cuda.synchronize()
    if coll:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    ops.GEMM_TIMER = None
    assert R.shape[0] == n_total * args.steps and torch.isfinite(R).all()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last[0], n_total, write=rank == 0)
    per_rank = None
    if coll:
        # per-rank diagnostics for the first real N > 1 run: every rank's own wall time over the timed region and the share
        # of it its host thread spent issuing launches (8 ranks share the box's host cores: the survey's predicted bottleneck)
        mine = torch.tensor([elapsed, host_issue, float(host["threads"])], device=dev, dtype=torch.float64)
        allr = torch.empty(dist.get_world_size() * 3, device=dev, dtype=torch.float64)
        dist.all_gather_into_tensor(allr, mine)
        per_rank = [{"rank": r, "ms_per_step": e / args.steps * 1e3, "host_issue_frac": h / max(e, 1e-12), "host_threads": int(t)}
                    for r, (e, h, t) in enumerate(allr.view(-1, 3).tolist())]
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax[0])

    if rank == 0 and per_step:
        print("per-step ms:", [round((b - a) * 1e3, 1) for a, b in zip([0.0] + per_step[:-1], per_step)], file=sys.stderr)
    if rank == 0:
        # dominant kernel = the plain instantiations of the ping-pong GEMM; the two launches per layer that carry a gated-MLP rule in
        # their epilogue are different kernels (other template instantiations, separate rows in the rocprof summary) and are reported
        # beside it: their duration includes the rule's own HBM traffic (gu read + Agu written: 0.94 GB per down-dgrad launch)
        n_launch, flops, secs = timer.summary(("plain", "plain_norm"))
        n_norm, flops_norm, secs_norm = timer.summary("plain_norm")
        n_all, flops_all, secs_all = timer.summary()
        traffic, traffic_note = pmc_traffic()
        peak = 2500.0 if dtype == torch.bfloat16 else 157.3
        if secs <= 0.0:       # --graph: the launches are replayed by the graph, no per-launch events exist (dev option; the judged run is eager)
            flops, secs, n_launch = 0.0, float("nan"), 0
            flops_all, secs_all, n_all = 0.0, float("nan"), 0
        achieved = flops / secs / 1e12
        fused = {}
        for tag in ("gated_fwd", "gated_bwd", "splitk", "plain_norm"):
            n_t, f_t, s_t = timer.summary(tag)
            if n_t and s_t > 0.0:
                fused[tag] = {"launches": n_t, "avg_launch_us": s_t / n_t * 1e6, "gemm_TFLOPs_incl_rule": f_t / s_t / 1e12}
        line = {
            "metric": "explanations/sec (full AttnLRP backward) Llama-3-8B seq=2048",
            "value": n_total * args.steps / elapsed, "unit": "explanations/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"Llama-3-8B shape ({cfg['n_layers']} layers, H4096, I14336, 32/8 heads, V128256), "
                                   f"random init, lxt.{args.mode} rule placement, seq={S}, causal, last-position arg-max logit",
                       "seq_len": S, "prompts_per_gpu_per_step": B, "global_batch": n_total, "mode": args.mode,
                       "activation_policy": "stash: every Linear output z, q/k before and after RoPE, o, lse and the residual sums are kept in HBM "
                                            "by the forward (~0.3 GB per layer and prompt); the backward recomputes no GEMM (DESIGN.md section 3)",
                       "parallelism": f"dp{world} (prompt sharding, no data-path collective)"},
            "roofline": {"bound": "mfma", "kernel": "gemm_pp_kernel<bf16, NT | NN, EPI 0 | 3 | 4 | 5> (8-wave ping-pong GEMM: Linear forward z = x W^T and "
                                                    "eps-rule dgrad c = s W from the stored weight), 6 launches per layer"
                                                    + (f"; {n_norm} of the {n_launch} launches carry a K1n epilogue (RMSNorm's row scale / residual add / "
                                                       "row sums of squares: +67 MB per launch)" if n_norm else ""),
                         "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                         "launches": n_launch, "avg_launch_us": secs / max(n_launch, 1) * 1e6,
                         "gemm_time_frac_of_step": secs_all / elapsed, "traffic": traffic, "traffic_note": traffic_note,
                         # every GEMM launch of the step (plain + the two per layer that carry a gated-MLP rule in their epilogue + split-K):
                         # the figure that is comparable across rounds (r01/r02 counted all launches)
                         "frac_all_gemm_launches": flops_all / secs_all / 1e12 / peak,
                         "with_fused_epilogue_launches": {"launches": n_all, "TFLOPs": flops_all / secs_all / 1e12,
                                                          "frac": flops_all / secs_all / 1e12 / peak, **fused}},
        }
        line["host"] = dict(host, host_issue_frac_of_step=host_issue / max(elapsed, 1e-12))
        if selfcheck is not None:
            line["multi_gpu_selfcheck"] = selfcheck
        if per_rank is not None:
            line["per_rank"] = per_rank
        if not args.no_smallm:
            line["roofline_linear_eps_smallm"] = smallm_roofline(ops, dtype, dev, cfg, B)
        if not args.no_config5 and args.layers == 32 and dtype == torch.bfloat16 and world == 1:
            line["config5_seq4096"] = config5_probe(eng, ops, cfg, dev, peak)
        if not args.no_extra_modes and args.layers == 32 and dtype == torch.bfloat16 and world == 1 and args.mode == "efficient":
            line.update(mode_batch_probes(eng, ops, cfg, dev, peak, S, B=B))
        if not args.no_config4 and args.layers == 32 and dtype == torch.bfloat16 and world == 1:
            eng.release()
            line["config4_gemma3_4b_text"], mm_line = config4_probe(ops, dev, dtype, peak, image=not args.no_config4_image)
            if mm_line is not None:
                line["config4_gemma3_4b_image_text"] = mm_line
        if not args.no_dropin and args.layers == 32 and dtype == torch.bfloat16 and world == 1:
            eng.release()
            try:
                line["dropin_monkey_patch"] = dropin_probe(dev, S=S, B=args.batch)
            except Exception as exc:  # noqa: BLE001  (a transformers API drift must not take the headline line down with it)
                line["dropin_monkey_patch"] = {"error": repr(exc)[:300]}
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(cfg, S)
            # the ratio to quote: against the REAL lxt.efficient's CPU number, not against the bf16 port above (torch's CPU bf16
            # matmuls make the port slower than the reference on 16x the cores)
            line["cpu_baseline"]["gpu_over_reference_cpu"] = line["value"] / line["cpu_baseline"]["reference_measured_in_build_container"]["value"]
        print(json.dumps(line), flush=True)
    if coll:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
