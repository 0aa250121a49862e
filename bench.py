#!/usr/bin/env python3
"""bench.py -- denoiser-steps/sec of the captured reverse-diffusion step on MI355X.

    python bench.py --gpus 1 --steps 50 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one `p_sample` iteration of the reference's sampling loop: denoiser
forward over [B, L, E] + nearest-embedding rounding + clamp + posterior mean + truncated-normal
noise (top_p = 1) + anchoring, i.e. one replay of the hipGraph built by
musediffusion_amd.models.diffusion._ReverseLoop.  Workload = BASELINE.json configs[1]
(seq_len 512, batch 64 per GPU, d_model 512, 12 layers, 8 heads, ffn 2048, E 128, vocab 729,
T = 2000 sqrt schedule), synthetic ComMU-shaped generation batch, torch-default random weights
(seed 0), bf16 compute with fp32 accumulation and fp32 latents.  With N > 1 every rank samples its
own batch of 64 (weak scaling; the reference shards whole batches over ranks, run/sample.py:169);
rank 0 builds the weights and ONE RCCL broadcast of the packed arena distributes them.

Prints ONE JSON line (rank 0) with the driver's contract: a plain run sets up, warms up, times exactly --steps steps and reports
them (`value`, `ms_per_step`).  `--full` adds what is measured beside the headline: `roofline` (the kernel with the largest time
share - the bf16 MFMA GEMM with the LayerNorm epilogue - timed live with HIP events on the launch streams), `kernels`, the repeated
timed regions of `config.repeats`, and at N = 1 `cpu_baseline` (the oracle = a torch-CPU fp32 port of the reference path, timed on
the host cores on a bounded sample) and `secondary` / `parity_mode` (training step, other precisions and widths, token agreement).
`--dump-outputs DIR` writes what the timed path computed in its last step as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

WORKLOADS = {
    # BASELINE.json configs[1]
    "c2": dict(L=512, B=64, E=128, H=512, nL=12, nh=8, F=2048, V=729, Tt=128, T=2000),
    # the reference-true BERT-base denoiser at the same batch (network.py:44)
    "c2-bertbase": dict(L=512, B=64, E=128, H=768, nL=12, nh=12, F=3072, V=729, Tt=128, T=2000),
    # the configuration the reference itself ships (config/train.py: seq_len 2096, hidden_dim 500 -> README.md:534 "embedding dim 500"; bert-base
    # encoder, network.py:44-46) at about config 2's token count: 16 sequences x 2096 = 33 536 tokens per step
    "ref-default": dict(L=2096, B=16, E=500, H=768, nL=12, nh=12, F=3072, V=729, Tt=128, T=2000),
    # BASELINE.json configs[0] shape (plumbing)
    "c1": dict(L=128, B=8, E=128, H=128, nL=2, nh=4, F=512, V=729, Tt=128, T=2000),
    # BASELINE.json configs[2]: modification (run/sample.py:109-114, :195-197): 200 DDIM steps (gap 10), strength 0.75 -> 150 iterations
    "c3": dict(L=512, B=64, E=128, H=512, nL=12, nh=8, F=2048, V=729, Tt=128, T=2000, ddim_steps=200, strength=0.75),
    # BASELINE.json configs[3]: generation, 64 sequences per GPU (512 on 8), through sampling.generate
    "c4": dict(L=512, B=64, E=128, H=512, nL=12, nh=8, F=2048, V=729, Tt=128, T=2000),
    # BASELINE.json configs[4]: training_losses, seq_len 1024, global batch 256 = 32 per GPU x 8 (DDP, RCCL all-reduce)
    "train": dict(L=1024, B=32, E=128, H=512, nL=12, nh=8, F=2048, V=729, Tt=128, T=2000),
}
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}   # dense peaks, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0                                 # HBM3E spec (6.3 TB/s achievable with a float4 copy, same guide)
DUMP_BYTES = 60 * 10**6                               # --dump-outputs: array data over all files (64 MB with room for the headers)


def dump_outputs(dirname, arrays):
    """`--dump-outputs DIR`: the arrays {name: tensor} a caller of the timed path receives from its last step, as DIR/<name>.npy.
    Floating point is written as float32 (float64 stays float64), integers (tokens) as float64, which holds them exactly.  Should the
    arrays exceed DUMP_BYTES together, each keeps the same fraction of its elements: a fixed sample (seed 0, sorted flat indices)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        t = t.detach()
        t = t.double() if (t.dtype == torch.float64 or not t.is_floating_point()) else t.float()
        host[name] = t.cpu().numpy()
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > DUMP_BYTES:
            keep = max(1, int(a.size * DUMP_BYTES // total))
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(dirname, name + ".npy"), a)


def step_flops(c):
    """Algorithmic flops of one reverse step, 2 flops per MAC."""
    N, H, F, L, E, V, Tt, B = c["B"] * c["L"], c["H"], c["F"], c["L"], c["E"], c["V"], c["Tt"], c["B"]
    proj = 4 * (E * H + H * H) if E != H else 0
    per_tok = c["nL"] * (2 * (4 * H * H + 2 * H * F) + 4 * L * H) + proj + 2 * V * E
    return N * per_tok + 2 * B * (4 * Tt * Tt + 4 * Tt * H)


def build(c, dtype, device, seed=0):
    from musediffusion_amd.models.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    from musediffusion_amd.models.network import TransformerNetModel
    torch.manual_seed(seed)
    model = TransformerNetModel(c["E"], c["E"], c["Tt"], c["V"], c["L"], dropout=0.1, bert_hidden=c["H"],
                                bert_layers=c["nL"], bert_heads=c["nh"], bert_ffn=c["F"], compute_dtype=dtype)
    model.eval().requires_grad_(False).to(device)
    diff = SpacedDiffusion(use_timesteps=space_timesteps(c["T"], [c["T"]]),
                           betas=get_named_beta_schedule("sqrt", c["T"]), rescale_timesteps=True, predict_xstart=True)
    return model, diff


def time_dominant_kernel(c, dtype, device, reps, branches=1):
    """Average launch duration of the step's dominant kernel (largest time share in profiles/), measured with HIP events
    on the launch streams, launched the way the step launches it.

    bf16 with d_model in {128, 256, 512}: the full-row GEMM with the bias + residual + LayerNorm epilogue
    (gemm_big_kernel<Row tile, EPI=3>), two launches per encoder layer and graph branch: attention-output dense
    (K = d_model) and FFN output dense (K = ffn), both N = d_model, on a branch's batch slice.  With two graph
    branches the step runs two of them side by side, so the timing loop does too (one stream per branch):
    `avg_launch_ms` = wall time of the region / launches (what the chip sustains), `launch_latency_ms` = the span one
    launch occupies on its own stream while it shares the chip with the other branch's (what rocprofv3 lists per kernel).  Otherwise (fp32 parity mode, d_model 768): the FFN intermediate dense with its GELU epilogue."""
    from musediffusion_amd import _lib, ops
    code = ops.dtype_code(dtype)
    td = ops.TORCH_DTYPE[code]
    panel = 1 if code == _lib.MH_BF16 else 0
    N_tok, H, F = (c["B"] // branches) * c["L"], c["H"], c["F"]
    lib = _lib.lib()
    fused = bool(panel and lib.mh_gemm_bias_res_ln_supported(H) and lib.mh_denoiser_get_fuse_ln())
    streams = [torch.cuda.Stream() for _ in range(branches)]
    bufs = []
    for _ in range(branches):
        bufs.append(dict(X=torch.randn(N_tok * H, device=device).to(td), Y=torch.empty(N_tok * H, device=device, dtype=td),
                         Fb=torch.randn(N_tok * F, device=device).to(td), Wa=(torch.randn(H * H, device=device) / 32).to(td),
                         W1=(torch.randn(F * H, device=device) / 32).to(td), W2=(torch.randn(F * H, device=device) / 32).to(td),
                         bias=torch.zeros(max(F, H), device=device), g=torch.ones(H, device=device)))

    def one_pass(bf, st):
        for _ in range(c["nL"]):
            if fused:
                for (A, W, K) in ((bf["X"], bf["Wa"], H), (bf["Fb"], bf["W2"], F)):
                    _lib.check(lib.mh_gemm_bias_res_ln(A.data_ptr(), N_tok, 1, W.data_ptr(), H, 1, bf["bias"].data_ptr(), bf["X"].data_ptr(),
                                                       N_tok, 1, bf["g"].data_ptr(), bf["bias"].data_ptr(), 1e-12, bf["Y"].data_ptr(), N_tok, 1,
                                                       N_tok, H, K, st))
            else:
                _lib.check(lib.mh_gemm_bias_act_ex(bf["X"].data_ptr(), N_tok if panel else H, panel, bf["W1"].data_ptr(), F if panel else H,
                                                   panel, bf["bias"].data_ptr(), None, 0, 0, bf["Fb"].data_ptr(), N_tok if panel else F, panel,
                                                   0, N_tok, F, H, 2, code, st))
    for bf, stream in zip(bufs, streams):
        one_pass(bf, stream.cuda_stream)
    torch.cuda.synchronize()
    # wall time of the whole region (all branches' launches running side by side) and each stream's own span
    cur = torch.cuda.current_stream()
    w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0.record(cur)
    evs = []
    for bf, stream in zip(bufs, streams):
        stream.wait_event(w0)
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                one_pass(bf, stream.cuda_stream)
            e1.record(stream)
            evs.append((e0, e1))
    for _, e1 in evs:
        cur.wait_event(e1)
    w1.record(cur)
    torch.cuda.synchronize()
    per_pass = c["nL"] * (2 if fused else 1)
    latency_ms = sum(a.elapsed_time(b) for a, b in evs) / len(evs) / (reps * per_pass)   # one launch, as its stream sees it
    avg_ms = w0.elapsed_time(w1) / (reps * per_pass * branches)                           # wall time per launch
    if fused:
        flops = (2.0 * N_tok * H * H + 2.0 * N_tok * H * F) / 2
        name = ("gemm_big_kernel<128x512 full-row tile, EPI=bias+residual+LayerNorm> bf16: attention-output dense [%d x %d x %d] and FFN "
                "output dense [%d x %d x %d], %d launches/step on %d concurrent stream(s)" % (N_tok, H, H, N_tok, H, F, per_pass * branches, branches))
    else:
        flops = 2.0 * N_tok * F * H
        name = "%s: FFN intermediate dense + GELU [%d x %d x %d], %d launches/step" % (
            "gemm_big_kernel<EPI=0, ACT=gelu> bf16" if panel else "gemm_kernel<float, EPI=0>", N_tok, F, H, per_pass * branches)
    return avg_ms, flops, name, latency_ms


def classify_launch(kernel, note, c, branches):
    """kernel symbol + launch note (csrc: mh_prof_note) -> (class name, bound, algorithmic work per launch, unit of work).
    Work is ALGORITHMIC: 2 M N K flops for the MFMA GEMMs, 4 L dh flops per (query, head) for attention, and for the HBM-bound
    kernels the bytes they must move at least once."""
    kv = dict(t.split("=", 1) for t in note.split() if "=" in t)
    N_tok = (c["B"] // branches) * c["L"]
    H, F, E, L = c["H"], c["F"], c["E"], c["L"]
    Ep = (E + 63) // 64 * 64
    if "split_gemm" in kernel:      # split precision (csrc/split.hip): ALGORITHMIC flops 2 M N K; the kernel issues three times that on the matrix pipe
        M, N, K, act = int(kv["M"]), int(kv["N"]), int(kv["K"].split("x")[-1]), int(kv.get("act", 0))
        role = "dense+residual+LayerNorm" if "ln_kernel" in kernel else ("dense+GELU (FFN1)" if act == 2 else "dense+tanh" if act == 1 else "dense")
        return "split_gemm<%s> %s [%d x %d x %d], 3 products per reference product" % (kv.get("tile", "?"), role, M, N, K), "mfma", 2.0 * M * N * K, "flop"
    if "split_attn" in kernel:
        bh, dh = int(kv.get("B", 0)) * int(kv.get("nh", 0)), int(kv.get("dh", 0))
        return "split_attn_kernel<dh=%d> [B*nh=%d, L=%d], 3 products per reference product" % (dh, bh, L), "valu+mfma", 4.0 * L * dh * bh * L, "flop"
    if "split_ln_kernel" in kernel:
        return "split_ln_kernel (fp32 rows -> split panels)", "hbm", float(2 * N_tok * H * 4), "B"
    if "gemm_strip_kernel" in kernel:      # round 6: dense + bias + GELU of K32 panels on the column-strip kernel (csrc/gemm_strip.h)
        M, N, K = int(kv["M"]), int(kv["N"]), int(kv["K"])
        return "gemm_strip_kernel<256x128 strips, mfma_32x32x16> bf16 dense+GELU (FFN1) [%d x %d x %d]" % (M, N, K), "mfma", 2.0 * M * N * K, "flop"
    if "gemm_big_kernel" in kernel or "gemm_kernel<bf16" in kernel:
        M, N, K, epi, act = int(kv["M"]), int(kv["N"]), int(kv["K"]), int(kv["epi"]), int(kv["act"])
        role = {3: "dense+bias+residual+LayerNorm", 1: "QKV projection + head scatter"}.get(epi) or (
            "dense+GELU (FFN1)" if act == 2 else "dense+tanh" if act == 1 else "dense")
        return "gemm_big_kernel<%s, EPI=%d> bf16 %s [%d x %d x %d]" % (kv.get("tile", "?"), epi, role, M, N, K), "mfma", 2.0 * M * N * K, "flop"
    if "gemm_kernel<float" in kernel:
        M, N, K = int(kv["M"]), int(kv["N"]), int(kv["K"])
        role = "rounding scores" if N == c["V"] else "dense (fp32 parity mode)"
        return "gemm_kernel<float> exact-fp32 MFMA, %s [%d x %d x %d]" % (role, M, N, K), "mfma_f32", 2.0 * M * N * K, "flop"
    if "gemm_tn_kernel" in kernel:      # weight gradient dW [M x N] = dY^T X over K tokens (note: gemm_dw M N K splits)
        M, N, K = int(kv["M"]), int(kv["N"]), int(kv["K"])
        return "gemm_tn_kernel weight gradient [%d x %d over %d tokens, %s slices]" % (M, N, K, kv.get("splits", "?")), "mfma", 2.0 * M * N * K, "flop"
    if "attn_bwd_dkv" in kernel or "attn_bwd_dq" in kernel:
        bh, dh = int(kv.get("B*nh", 0)), int(kv.get("dh", 0))
        nmm = 4 if "dkv" in kernel else 3     # S, dP, dV, dK  /  S, dP, dQ: 2 L^2 dh flops each per (batch, head)
        return "%s [B*nh=%d, L=%d] (%d products)" % ("attn_bwd_dkv_kernel" if nmm == 4 else "attn_bwd_dq_kernel", bh, L, nmm), "valu+mfma", nmm * 2.0 * L * L * dh * bh, "flop"
    if "attn_f32_kernel" in kernel:       # fp32 parity mode: tiled attention on the exact-fp32 MFMA / VALU
        bh, dh = (c["B"] // branches) * c["nh"], H // c["nh"]
        return "attn_f32_kernel<dh=%d> [B*nh=%d, L=%d]" % (dh, bh, L), "mfma_f32", 4.0 * L * dh * bh * L, "flop"
    if kernel == "kern" or "attn_" in kernel:
        bh, dh = int(kv.get("B*nh", 0)), int(kv.get("dh", 0))
        return "attn_stream_bf16_kernel<dh=%d> [B*nh=%d, L=%d]" % (dh, bh, L), "valu+mfma", 4.0 * L * dh * bh * L, "flop"
    b = None
    if "ln_panel_kernel" in kernel or "ln_panel4_kernel" in kernel:
        b = 2 * N_tok * H * 2 + (N_tok * H * 2 if E != H else 0) * 0                        # read [N,H] bf16, write [N,H] bf16
    elif "pack_panel" in kernel:
        b = N_tok * E * 4 + N_tok * Ep * 2
    elif "unpack_panel" in kernel:
        b = N_tok * H * 2 + N_tok * E * 4
    elif "step_epilogue" in kernel:
        b = N_tok * E * 4 * 5 + N_tok * 4        # model_out (or round idx + rows), x_t, noise, x_start in; sample + pred out; mask
    elif "trunc_normal" in kernel:
        b = int(kv.get("n", c["B"] * L * E)) * 4   # (one draw for the whole batch, or one per decoupled batch slice)
    elif "row_sqnorm_f32" in kernel:
        b = N_tok * E * 4
    elif "argbest_reduce" in kernel:
        b = N_tok * 12 * 8
    elif "adamw_ema_kernel" in kernel:
        b = c.get("n_params", 0) * 4 * (7 + 2 * int(kv.get("n_ema", 0)))       # p, m, v read + written, g read, each EMA copy read + written
    elif "sumsq_chunks" in kernel:
        b = c.get("n_params", 0) * 4
    elif "sum_slices" in kernel:
        b = (int(kv.get("slices", 0)) + 1) * int(kv.get("n", 0)) * 4
    elif "ln_bwd_kernel" in kernel:
        b = 3 * N_tok * H * 2
    elif "head_transpose" in kernel:
        b = 2 * N_tok * H * 2
    elif "dropout_bits_kernel" in kernel:
        b = (c["B"] // branches) * c["nh"] * L * L // 8
    if b is not None:
        return kernel.strip("()"), "hbm", float(b), "B"
    return kernel.strip("()"), "latency", 0.0, ""


def collect_launches(run, n_steps, with_stream=False):
    """Runs `run()` n_steps times with the library's per-launch HIP events on -> [(kernel, note, ms)] (with_stream: + the stream handle)"""
    import ctypes
    from musediffusion_amd import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    _lib.check(lib.mh_profile_start(), "mh_profile_start")
    for _ in range(n_steps):
        run()
    buf = ctypes.create_string_buffer(1 << 24)
    need = lib.mh_profile_stop(buf, len(buf))
    assert 0 < need <= len(buf), need
    recs = []
    for line in buf.value.decode().splitlines():
        kernel, note, grid, block, stream, ms = line.split("\t")
        if float(ms) >= 0:
            recs.append((kernel, note, float(ms), stream) if with_stream else (kernel, note, float(ms)))
    return recs


def main_stream_launches(recs4):
    """[(kernel, note, ms, stream)] -> ([(kernel, note, ms)] of the stream that carries most of the time, [(kernel, ms)] of the others)"""
    by_stream = {}
    for _, _, ms, st in recs4:
        by_stream[st] = by_stream.get(st, 0.0) + ms
    main = max(by_stream, key=by_stream.get)
    return [(k, n, ms) for k, n, ms, st in recs4 if st == main], [(k, ms) for k, n, ms, st in recs4 if st != main]


def kernel_rows(recs, c, branches, n_steps, ms_per_step):
    """Per-launch records -> per-class rows with in-step duration, rate and roofline fraction (see profile_step)."""
    classes, total = {}, 0.0
    for kernel, note, ms in recs:
        name, bound, work, unit = classify_launch(kernel, note, c, branches)
        e = classes.setdefault(name, dict(bound=bound, unit=unit, work=0.0, span_ms=0.0, launches=0))
        e["work"] += work
        e["span_ms"] += ms
        e["launches"] += 1
        total += ms
    rows = []
    for name, e in classes.items():
        share = e["span_ms"] / total
        per_step = e["launches"] / n_steps
        instep_ms = share * ms_per_step / per_step
        work = e["work"] / e["launches"]
        row = {"kernel": name, "bound": e["bound"], "launches_per_step": round(per_step, 2), "share": round(share, 4),
               "avg_launch_ms": round(instep_ms, 5), "stream_span_ms": round(e["span_ms"] / e["launches"], 5)}
        if e["unit"] == "flop" and work > 0:
            tf = work / (instep_ms * 1e-3) / 1e12
            peak = MFMA_PEAK_TFLOPS["fp32" if e["bound"] == "mfma_f32" else "bf16"]
            row.update(achieved=round(tf, 1), unit="TFLOP/s", frac=round(tf / peak, 4), work_per_launch=work)
        elif e["unit"] == "B" and work > 0:
            gbs = work / (instep_ms * 1e-3) / 1e9
            row.update(achieved=round(gbs, 1), unit="GB/s", frac=round(gbs / HBM_PEAK_GBS, 4), work_per_launch=work)
        rows.append(row)
    rows.sort(key=lambda r: -r["share"])
    return rows, total / n_steps


def roofline_from_rows(rows, span_sum, ms_per_step, dtype, workload, branches, n_prof, what="step"):
    """The dominant kernel = the kernel SYMBOL with the largest share (its launches of different shapes pooled):
    achieved = mean algorithmic flops per launch / mean in-step duration per launch."""
    sym = lambda r: r["kernel"].split(" [")[0]
    pools = {}
    for r in rows:
        if r["bound"] in ("mfma", "mfma_f32") and r.get("work_per_launch"):
            pools.setdefault(sym(r), []).append(r)
    dom = max(pools.values(), key=lambda rs: sum(r["share"] for r in rs))
    n_l = sum(r["launches_per_step"] for r in dom)
    share = sum(r["share"] for r in dom)
    fpl = sum(r["work_per_launch"] * r["launches_per_step"] for r in dom) / n_l
    avg_ms = share * ms_per_step / n_l
    ach = fpl / (avg_ms * 1e-3) / 1e12
    peak = MFMA_PEAK_TFLOPS["fp32" if dom[0]["bound"] == "mfma_f32" else "bf16"]
    variant = sym(dom[0])
    return {"bound": "mfma", "kernel": variant + ": " + "; ".join(r["kernel"].split(" [")[1].rstrip("]") if " [" in r["kernel"] else "" for r in dom),
            "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "traffic": pmc_traffic(workload, dtype, branches, variant),
            "traffic_source": "profiles/pmc_traffic.json - HBM bytes per launch from the builder's separate rocprofv3 --pmc passes of this command "
                              "(2 x FETCH_SIZE + WRITE_SIZE, MI355X_MICROARCH.md), keyed by workload and kernel variant; replayed here, NOT measured "
                              "in this run (null when the recorded variant is not the one that ran)",
            "avg_launch_ms": round(avg_ms, 5), "launches_per_step": n_l, "share_of_step": round(share, 4),
            "how": "in-%s: HIP events around every launch of the eager %s on its own stream (%d repetitions); share = spans of this kernel / "
                   "all spans (sum %.3f ms per %s on %d concurrent stream(s) vs %.3f ms wall); avg_launch_ms = share x ms_per_step / launches"
                   % (what, what, n_prof, span_sum, what, branches, ms_per_step),
            "concurrent_streams": branches,
            "stream_span_ms": round(sum(r["stream_span_ms"] * r["launches_per_step"] for r in dom) / n_l, 5),
            "flops_per_launch": fpl}


def profile_step(loop, c, first_k, n_steps, ms_per_step):
    """Per-kernel time INSIDE the step: the step's launch sequence run eagerly on the same streams (same branches) with every
    launch bracketed by HIP events on its stream (mh_profile_start / _stop).  With two branches sharing the chip a launch's span
    on its stream is longer than its share of the wall time, so spans are turned into shares: share = sum of the class's spans /
    sum of all spans, in-step duration per launch = share x ms_per_step / launches per step."""
    was = loop.diff.use_graph
    loop.diff.use_graph = False
    try:
        with torch.no_grad():
            loop.advance(first_k)                                  # eager warm-up
            k = [first_k]

            def one():
                k[0] += 1
                loop.advance(k[0])
            recs = collect_launches(one, n_steps)
    finally:
        loop.diff.use_graph = was
    return kernel_rows(recs, c, int(loop.nsplit), n_steps, ms_per_step)


def dist_evidence(world, device, local_rank):
    """What proves (or disproves) that RCCL carried `world` ranks on `world` different GPUs: the process group's backend, the rank
    count as the backend reports it (0 unless it is nccl = RCCL), and every rank's device as the runtime names it."""
    import torch.distributed as dist
    backend = dist.get_backend() if (world > 1 and dist.is_initialized()) else "none (single process)"
    props = torch.cuda.get_device_properties(device)
    mine = "rank %d: cuda:%d %s uuid=%s" % (int(os.environ.get("RANK", "0")), local_rank, props.name, getattr(props, "uuid", "?"))
    names = [mine]
    if world > 1:
        names = [None] * world
        dist.all_gather_object(names, mine)
    return {"backend": backend, "rccl_ranks": dist.get_world_size() if backend == "nccl" else 0, "devices": names,
            "distinct_devices": len({n.split("uuid=")[-1] for n in names})}


def pmc_traffic(workload, dtype, branches, variant):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes (FETCH_SIZE doubled as
    MI355X_MICROARCH.md prescribes for gfx950, + WRITE_SIZE).  Entries are keyed by workload AND kernel variant (the tile /
    epilogue signature bench.py reports): None when no pass was recorded for the variant that runs now (a stale entry never matches)."""
    try:
        with open(os.path.join(REPO, "profiles", "pmc_traffic.json")) as f:
            rec = json.load(f).get("%s/%s/b%d" % (workload, dtype, branches))
        if rec is None or rec.get("variant") != variant:
            return None
        return float(rec["traffic_bytes_per_launch"])
    except (OSError, ValueError, KeyError):
        return None


def host_description():
    """CPU model, physical cores and hardware threads of the box (BASELINE.md section 3 asks for them beside the CPU number)."""
    model, phys = "?", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                pid = v
            elif k == "core id":
                cid = v
            elif not k and pid is not None:
                phys.add((pid, cid)); pid = cid = None
    except OSError:
        pass
    return {"cpu_model": model, "physical_cores": len(phys) or None, "hardware_threads": os.cpu_count()}


def best_thread_count(fn):
    """torch's CPU GEMMs are far from optimal on all hardware threads of a many-core host: take the thread count that runs fn() fastest"""
    hw = os.cpu_count() or 1
    best, cores = None, hw
    for n in sorted({min(hw, k) for k in (8, 16, 32, 64, 128, hw)}):
        torch.set_num_threads(n)
        fn()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, cores = dt, n
    torch.set_num_threads(cores)
    return cores


def cpu_baseline(c, kind="p", seconds_budget=40.0):
    """The oracle (torch-CPU fp32 port of the reference path) on the same workload: the FULL batch, one warm-up step, then >= 3 timed
    steps (SURVEY.md 8d / BASELINE.md section 3) unless a step takes so long that the budget ends the loop earlier (never below 2)."""
    from musediffusion_amd import synthetic
    from oracle import denoiser as odn, sampling as osa, schedule as osc
    B = c["B"]
    sd = odn.random_state_dict(c["E"], c["H"], c["F"], c["nL"], c["V"], c["L"], c["Tt"], seed=0)
    probe_x, probe_t = torch.randn(min(B, 8), c["L"], c["E"]), torch.full((min(B, 8),), 10.0)

    def probe():
        with torch.no_grad():
            odn.forward(sd, probe_x, probe_t, c["nh"])
    cores = best_thread_count(probe)
    d = osc.make_diffusion(diffusion_steps=c["T"])
    batch = synthetic.generation_batch(B, c["L"], seed=1)
    emb_w = sd["word_embedding.weight"]
    x_start = emb_w[batch["input_ids"].long()]
    mask3 = torch.broadcast_to(batch["input_mask"].unsqueeze(-1), x_start.shape)
    torch.manual_seed(105)
    x = osa.start_latent_generation(x_start, mask3)
    fn = lambda xx, ts: odn.forward(sd, xx, ts, c["nh"])

    def step(i, x):
        t = torch.tensor([i] * B)
        with torch.no_grad():
            if kind == "ddim":
                return osa.ddim_sample(d, fn, x, t, True, emb_w, mask=mask3, x_start=x_start)["sample"]
            return osa.p_sample(d, fn, x, t, True, emb_w, top_p=1, mask=mask3, x_start=x_start)["sample"]
    x = step(c["T"] - 1, x)  # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        x = step(c["T"] - 2 - n, x)
        n += 1
        el = time.perf_counter() - t0
        if n >= 3 and (el > seconds_budget / 2 or n >= 10):
            break
        if n >= 2 and el > seconds_budget:
            break
    out = {"value": n / el, "unit": "denoiser-steps/s", "cores": cores, "kind": "port",
           "sample": "oracle %s step (torch CPU fp32, %d threads = the fastest of 8 / 16 / 32 / 64 / 128 / all on this host) on the FULL batch of "
                     "%d sequences x seq_len %d: %d timed steps in %.1f s after 1 warm-up step (%.2f s per step)"
                     % ("ddim_sample" if kind == "ddim" else "p_sample", cores, B, c["L"], n, el, el / n)}
    out.update(host_description())
    return out


def cpu_baseline_train(c, n_seq=2, seconds_budget=40.0):
    """The oracle's training_losses (with-corruption variant) forward + backward over ALL parameters on n_seq of the micro-batch's
    sequences (fp32, eval-mode arithmetic: the oracle's dropout needs explicit masks), scaled to one micro-batch of c['B'] sequences."""
    from musediffusion_amd import synthetic
    from oracle import denoiser as odn, losses as olo, schedule as osc
    sd = odn.random_state_dict(c["E"], c["H"], c["F"], c["nL"], c["V"], c["L"], c["Tt"], seed=0)
    for k, v in sd.items():
        if v.is_floating_point() and k != "lm_head.weight":
            v.requires_grad_(True)
    sd["lm_head.weight"] = sd["word_embedding.weight"]
    d = osc.make_diffusion(diffusion_steps=c["T"])
    b = synthetic.training_batch(n_seq, c["L"], seed=1)
    t = torch.tensor([(17 + 613 * i) % c["T"] for i in range(n_seq)])

    def step():
        for v in sd.values():
            v.grad = None
        terms = olo.training_losses(d, lambda x, ts: odn.forward(sd, x, ts, c["nh"]), lambda ids: odn.get_embeds(sd, ids),
                                    lambda h: odn.get_logits(sd, h), t, b["input_ids"], b["input_mask"], correct_ids=b["correct_ids"])
        terms["loss"].mean().backward()
    cores = best_thread_count(step)
    step()
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        el = time.perf_counter() - t0
        if (n >= 3 and el > seconds_budget / 2) or n >= 10 or (n >= 2 and el > seconds_budget):
            break
    per_micro = el / n * c["B"] / n_seq
    out = {"value": 1.0 / per_micro, "unit": "micro-batches/s (training_losses fwd+bwd, %d x %d tokens)" % (c["B"], c["L"]), "cores": cores,
           "kind": "port", "sample": "oracle training_losses_seq2seq_with_corruption forward + backward (torch CPU fp32 autograd, %d threads) on %d "
                                     "of the %d sequences of a micro-batch, seq_len %d: %d timed repetitions in %.1f s after warm-up; value = "
                                     "measured rate x %d/%d (cost is linear in the batch); the optimizer step is not included"
                                     % (cores, n_seq, c["B"], c["L"], n, el, n_seq, c["B"])}
    out.update(host_description())
    return out


def make_sampler(name, diff):
    """`uniform` (the reference's fallback, train_util.py:84) or `lossaware` (its DEFAULT, config/train.py:38-39, scripts/run_train.sh:12).
    The factory refuses lossaware without a process group like the reference's (step_sample.py:23-24); a single-GPU bench line builds
    the class directly - the update path is the same minus the all-gather."""
    from musediffusion_amd.models.step_sample import LossSecondMomentResampler, UniformSampler
    return LossSecondMomentResampler(diff) if name == "lossaware" else UniformSampler(diff)


def train_main(args, world, rank, local_rank, device):
    """`--workload train` (BASELINE.json configs[4]): one step = ONE OPTIMIZER STEP of the reference's TrainLoop
    (utils/train_util.py:170-172): `--accum` micro-batches of 32 sequences x seq_len 1024 per GPU through training_losses
    forward + backward in train mode (dropout 0.1 at the reference's three sites), DDP gradient all-reduce over RCCL on the
    last micro-batch only (`no_sync` before it), then the fused AdamW + 3 x EMA step.  Reported separately from the headline
    sampling metric."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from musediffusion_amd import sharding, synthetic
    from musediffusion_amd.train_step import TrainStep
    c = WORKLOADS["train"]
    model, diff = build(c, args.dtype, device, seed=rank)
    model.train().requires_grad_(True)
    ddp = None
    if world > 1:
        sharding.broadcast_weights(model, src=0)                    # utils/dist_util.py:141-152 as one flat broadcast
        ddp = DDP(model, device_ids=[local_rank], broadcast_buffers=False, bucket_cap_mb=128, find_unused_parameters=False)
    loop = TrainStep(model, diff, microbatch=c["B"], lr=1e-4, weight_decay=0.0, ema_rate=(0.5, 0.9, 0.99), learning_steps=320000,
                     ddp_model=ddp, schedule_sampler=make_sampler(args.sampler, diff))
    import numpy as np
    np.random.seed(7 + rank)                                         # the schedule sampler draws with np.random (step_sample.py:45-63)
    cond = synthetic.training_batch(c["B"] * args.accum, c["L"], seed=1 + rank)

    for _ in range(args.warmup):
        loop.run_step(cond)

    def timed():
        for _ in range(args.steps):
            losses, gn = loop.run_step(cond)
        return losses, gn
    elapsed, (losses, gn) = timed_region(timed, world, device)
    assert bool(torch.isfinite(losses["loss"])) and bool(torch.isfinite(gn).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict({"losses_" + k: v for k, v in losses.items()}, grad_norm=gn))
    # the gradient all-reduce's EXPOSED time (--full): the same steps with DDP's all-reduce suppressed on every micro-batch (no_sync) -
    # the difference is what the collective adds to a step after its overlap with the backward (0 by construction at N = 1)
    nosync_ms = None
    if world > 1 and args.full:
        def timed_nosync():
            for _ in range(args.steps):
                with ddp.no_sync():
                    loop.forward_backward(cond)
                loop.optimize()
                loop.step += 1
        nosync_ms = timed_region(timed_nosync, world, device)[0] / args.steps * 1e3
    ev = dist_evidence(world, device, local_rank)
    n_params = sum(p.numel() for p in model.parameters())
    ms_per_step = elapsed / args.steps * 1e3
    out = None
    if rank == 0:
        N = c["B"] * c["L"] * args.accum
        fwd = (step_flops(dict(c)) - 2 * c["B"] * c["L"] * c["V"] * c["E"] + 2 * 2 * c["B"] * c["L"] * c["V"] * c["E"]) * args.accum
        out = {"metric": "training-steps/sec (optimizer steps: %d x training_losses fwd+bwd at seq_len=%d, batch=%d/GPU, + AdamW/EMA)"
                         % (args.accum, c["L"], c["B"]),
               "value": round(args.steps / elapsed, 3), "unit": "optimizer steps/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": "TrainLoop.run_step: training_losses_seq2seq_with_corruption fwd+bwd (train mode, dropout %.2f) "
                                      "x %d micro-batches, %s schedule sampler, DDP all-reduce on the last, fused AdamW + 3 EMA; seq_len=%d microbatch=%d/GPU "
                                      "d_model=%d layers=%d" % (model.dropout.p, args.accum, args.sampler, c["L"], c["B"], c["H"], c["nL"]),
                          "global_batch": c["B"] * args.accum * world, "seq_len": c["L"], "parallelism": "ddp x%d" % world,
                          "backend": ev["backend"], "rccl_ranks": ev["rccl_ranks"], "devices": ev["devices"],
                          "distinct_devices": ev["distinct_devices"], "microbatches_per_step": args.accum,
                          "ms_per_microbatch": round(elapsed / args.steps / args.accum * 1e3, 3),
                          "tokens_per_s": round(world * args.steps * N / elapsed, 1),
                          "approx_tflops": round(3 * fwd / (elapsed / args.steps) / 1e12, 2),
                          "gradient_bytes_all_reduced_per_step": n_params * 4,
                          "ms_per_step_without_all_reduce": None if nosync_ms is None else round(nosync_ms, 3),
                          "all_reduce_exposed_ms": None if nosync_ms is None else round(ms_per_step - nosync_ms, 3),
                          "loss": round(float(losses["loss"]), 4), "grad_norm": round(float(gn), 4)}}
    if not args.no_kernel_timing:
        # every launch of one optimizer step bracketed by HIP events (all ranks run it: the step holds a collective)
        recs4 = collect_launches(lambda: loop.run_step(cond), 2, with_stream=True)
        # the step's kernels run on ONE stream; what runs beside them on the model's side stream (the gradient folds of the panel layers'
        # backward, the attention keep bits at the head of the forward) overlaps them and must not dilute their shares of the wall time
        recs, side = main_stream_launches(recs4)
        if rank == 0:
            cc = dict(c, n_params=n_params)
            rows, span_sum = kernel_rows(recs, cc, 1, 2, ms_per_step)
            out["roofline"] = roofline_from_rows(rows, span_sum, ms_per_step, args.dtype, "train", 1, 2, what="optimizer step")
            out["roofline"]["side_stream"] = {"launches_per_step": len(side) / 2, "span_ms_per_step": round(sum(ms for _, ms in side) / 2, 3),
                                              "note": "launches on the model's side stream (split-K / LayerNorm gradient folds, attention keep bits): they "
                                                      "overlap the main stream's kernels and are left out of the shares above"}
            out["kernels"] = [{k: v for k, v in r.items() if k != "work_per_launch"} for r in rows if r["share"] >= 0.004]
    if rank == 0:
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline_train(c)
            out["cpu_baseline"]["value"] = round(out["cpu_baseline"]["value"], 6)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n, argv):
    """`python bench.py --gpus N` with no launcher around it: start N fresh ranks (one per GPU) the way the reference's own
    launcher does (utils/dist_run.py:13-51: `python -m torch.distributed.run`), as a CHILD process of this one, which has
    not touched the GPU (importing torch does not), and exit with the child's code.  Never an exec of a GPU process."""
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))       # dist_run.py:31
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    raise SystemExit(subprocess.call(cmd, env=env))


def init_ranks(args):
    """Rank bookkeeping shared by every workload: WORLD_SIZE must equal --gpus (also when it is 1), one process per GPU, RCCL."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # MUSE_BENCH_SHARE_GPU=1 (tests/test_multirank_gpu.py on a one-GPU box only): every rank on cuda:0, collectives over gloo -
    # the launcher, the rank logic and the collectives' call sites are exercised end to end; the numbers mean nothing
    share = os.environ.get("MUSE_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: process group has %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus))
    return world, rank, local_rank, device


def timed_region(fn, world, device):
    """barrier + synchronize on both sides of fn(); returns the MAX elapsed seconds over ranks."""
    import torch.distributed as dist
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    return float(el.item()), out


def assert_same_on_all_ranks(value, what, world, device):
    """Every rank must hold the same int64 scalar (weight checksum, token checksum)."""
    import torch.distributed as dist
    if world == 1:
        return
    t = torch.tensor([int(value)], device=device, dtype=torch.int64)
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t)
    vals = [int(p.item()) for p in parts]
    if len(set(vals)) != 1:
        raise SystemExit("bench.py: %s differs across ranks: %s" % (what, vals))


def make_loop(model, diff, c, kind, device, rank, need):
    """The captured reverse step of the workload as a _ReverseLoop over `need` iterations: `kind` "p" = p_sample with rounding, clamp
    and top_p = 1 (BASELINE configs[1], [3]); "ddim" = ddim_sample with rounding (configs[2])."""
    from functools import partial
    from musediffusion_amd import synthetic
    from musediffusion_amd.models.diffusion import _ReverseLoop
    from musediffusion_amd.models.rounding import denoised_fn_round
    batch = synthetic.generation_batch(c["B"], c["L"], seed=1 + rank)
    ids, mask = batch["input_ids"].to(device), batch["input_mask"].to(device)
    x_start = model.get_embeds(ids)
    mask3 = torch.broadcast_to(mask.unsqueeze(-1), x_start.shape)
    torch.manual_seed(105)
    x_noised = torch.where(mask3 == 0, x_start, torch.randn_like(x_start))
    model_emb = torch.nn.Embedding(c["V"], c["E"], _weight=model.word_embedding.weight.clone()).eval().requires_grad_(False)
    fn = partial(denoised_fn_round, model_emb, dist=None)
    indices = (list(range(c["T"]))[::-1] * (need // c["T"] + 1))[:need]     # (a timed region longer than T steps wraps around)
    loop = _ReverseLoop.try_build(diff, kind, model, x_noised, True, fn, 1 if kind == "p" else None, mask3, x_start, 0.0, indices,
                                  lambda i: fn, False)
    assert loop is not None, "fused reverse loop unavailable"
    return loop


def step_tables(loop, c, args, ms_per_step, first_k, n_prof=4):
    """`roofline` + `kernels` of a captured step from its eager, per-launch-timed twin (profile_step)."""
    rows, span_sum = profile_step(loop, c, first_k, n_prof, ms_per_step)
    roof = roofline_from_rows(rows, span_sum, ms_per_step, args.dtype, args.workload, int(loop.nsplit), n_prof)
    return roof, [{k: v for k, v in r.items() if k != "work_per_launch"} for r in rows if r["share"] >= 0.002]


def sampling_main(args, world, rank, local_rank, device):
    """`--workload c3 | c4`: the reference's sampling block (run/sample.py:185-220) end to end through
    musediffusion_amd.sampling: rank 0 owns the weights -> ONE packed RCCL broadcast -> every rank samples its contiguous
    shard of the global batch -> ONE token all-gather.  c4 = generation (BASELINE configs[3]: 64 sequences per GPU, p_sample
    loop), c3 = modification (configs[2]: 200 DDIM steps x strength 0.75 = q_sample to t = 149, then 150 iterations)."""
    import torch.distributed as dist
    from musediffusion_amd import sampling, sharding, synthetic
    c = WORKLOADS[args.workload]
    model, diff = build(c, args.dtype, device, seed=rank)          # different weights per rank until the broadcast
    sharding.broadcast_weights(model, src=0, packed=True)
    arena_sum = sharding.weights_checksum(model)
    assert_same_on_all_ranks(arena_sum, "weight arena checksum after the broadcast", world, device)
    ev = dist_evidence(world, device, local_rank)
    diff.rng_mode, diff.rng_seed, diff.rng_stream = args.rng, 105, rank
    diff.use_graph = not args.no_graph
    Bg = c["B"] * world
    torch.manual_seed(105 + rank)
    if args.workload == "c4":
        cond = synthetic.generation_batch(Bg, c["L"], seed=1)
        steps = args.steps
        run = lambda n: sampling.generate(model, diff, cond, t_enc=n, sharded=True)
        what = "sampling.generate (p_sample_loop, first %d of T=%d iterations)" % (steps, c["T"])
    else:
        tb = synthetic.training_batch(Bg, c["L"], seed=1)
        cond = {"input_ids": tb["input_ids"], "input_mask": tb["input_mask"]}
        steps = int(c["ddim_steps"] * c["strength"])
        run = lambda n: sampling.modify(model, diff, cond, step=c["ddim_steps"], strength=c["strength"], sharded=True)
        what = "sampling.modify (q_sample to t=%d, %d ddim iterations, gap %d)" % (steps - 1, steps, c["T"] // c["ddim_steps"])
    if args.warmup > 0:
        run(min(args.warmup, steps))
    elapsed, tokens = timed_region(lambda: run(steps), world, device)
    assert tokens.shape == (Bg, c["L"]) and tokens.dtype == torch.int64
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"tokens": tokens})
    assert_same_on_all_ranks(int(tokens.sum().item()) * 1000003 + int((tokens * torch.arange(1, c["L"] + 1, device=tokens.device)).sum().item()),
                             "gathered token checksum", world, device)
    if rank == 0:
        flops = step_flops(c)
        ms = elapsed / steps * 1e3
        out = {"metric": "denoiser-steps/sec (seq_len=%d, batch=%d)" % (c["L"], c["B"]), "value": round(world * steps / elapsed, 3),
               "unit": "denoiser-steps/s", "n_gpus": world, "steps": steps, "warmup": args.warmup, "ms_per_step": round(ms, 4),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": "%s: %s; seq_len=%d batch=%d/GPU (global %d) d_model=%d layers=%d; timed region = the whole call: "
                                      "embed + start latent + loop set-up (graph capture) + loop + logits argmax + token all-gather"
                                      % (args.workload, what, c["L"], c["B"], Bg, c["H"], c["nL"]),
                          "global_batch": Bg, "seq_len": c["L"], "parallelism": "batch-sharded x%d" % world,
                          "backend": ev["backend"], "rccl_ranks": ev["rccl_ranks"], "devices": ev["devices"], "distinct_devices": ev["distinct_devices"],
                          "weights": "one packed-arena broadcast from rank 0 (%.1f MB)" % (model.engine().arena_bytes() / 1e6),
                          "arena_checksum_after_broadcast": int(arena_sum),
                          "rng": args.rng, "hipgraph": not args.no_graph,
                          "step_tflops_achieved": round(flops / (ms * 1e-3) / 1e12, 2)}}
        if not args.no_kernel_timing:
            # the same captured step as a stand-alone loop (this rank's shard), every launch timed: whole-call ms_per_step is the scale
            ploop = make_loop(model, diff, c, "p" if args.workload == "c4" else "ddim", device, rank, 16)
            with torch.no_grad():
                ploop.begin()
                ploop.advance(0)
            out["roofline"], out["kernels"] = step_tables(ploop, c, args, ms, 1)
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(c, kind="p" if args.workload == "c4" else "ddim")
            out["cpu_baseline"]["value"] = round(out["cpu_baseline"]["value"], 5)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _time_loop(c, dtype, device, steps, warmup):
    """steps/s of the captured p_sample step of config `c` in compute mode `dtype` (the headline's procedure on a short region)"""
    model, diff = build(c, dtype, device, seed=0)
    diff.rng_mode, diff.rng_seed, diff.rng_stream, diff.use_graph = "philox", 105, 0, True
    loop = make_loop(model, diff, c, "p", device, 0, warmup + steps + 2)
    with torch.no_grad():
        loop.begin()
        for k in range(warmup):
            loop.advance(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(warmup, warmup + steps):
            loop.advance(k)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        loop.finish()
    assert bool(torch.isfinite(loop.x).all())
    ms = el / steps * 1e3
    return {"value": round(steps / el, 3), "unit": "denoiser-steps/s", "ms_per_step": round(ms, 4), "steps": steps, "warmup": warmup, "dtype": dtype,
            "step_tflops_achieved": round(step_flops(c) / (ms * 1e-3) / 1e12, 2), "graph_branches": int(loop.nsplit)}


def _time_train(device, steps, warmup, sampler="uniform"):
    """ms per optimizer step of `--workload train` (one micro-batch of 32 x 1024 tokens, train mode, dropout 0.1, fused AdamW + 3 EMA) and
    the dominant kernel's roofline fraction inside it"""
    import numpy as np
    from musediffusion_amd import synthetic
    from musediffusion_amd.train_step import TrainStep
    c = WORKLOADS["train"]
    model, diff = build(c, "bf16", device, seed=0)
    model.train().requires_grad_(True)
    loop = TrainStep(model, diff, microbatch=c["B"], lr=1e-4, weight_decay=0.0, ema_rate=(0.5, 0.9, 0.99), learning_steps=320000,
                     schedule_sampler=make_sampler(sampler, diff))
    np.random.seed(7)
    cond = synthetic.training_batch(c["B"], c["L"], seed=1)
    for _ in range(warmup):
        loop.run_step(cond)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses, gn = loop.run_step(cond)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    assert bool(torch.isfinite(losses["loss"])) and bool(torch.isfinite(gn).all())
    ms = el / steps * 1e3
    n_params = sum(p.numel() for p in model.parameters())
    fwd = step_flops(dict(c)) + 2 * c["B"] * c["L"] * c["V"] * c["E"]
    out = {"value": round(steps / el, 3), "unit": "optimizer steps/s", "ms_per_step": round(ms, 3), "steps": steps, "warmup": warmup, "dtype": "bf16",
           "tokens_per_s": round(steps * c["B"] * c["L"] / el, 1), "approx_tflops": round(3 * fwd / (ms * 1e-3) / 1e12, 2),
           "workload": "TrainLoop.run_step: training_losses (with corruption) fwd+bwd, train mode, dropout 0.1, 32 x 1024 tokens, %s sampler, fused AdamW + 3 EMA" % sampler}
    if sampler != "uniform":
        return out
    recs = main_stream_launches(collect_launches(lambda: loop.run_step(cond), 2, with_stream=True))[0]
    rows, span_sum = kernel_rows(recs, dict(c, n_params=n_params), 1, 2, ms)
    roof = roofline_from_rows(rows, span_sum, ms, "bf16", "train", 1, 2, what="optimizer step")
    out["roofline"] = {k: roof[k] for k in ("kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms", "launches_per_step", "share_of_step")}
    return out


def secondary_block(device, budget_note="short timed regions: <= 60 s in total"):
    """What the headline line does not show, measured by the same process right after it (N = 1 only): the training step, the
    token-exact fp32 mode, the reference-true width, and how many tokens the fast mode changes.  Each entry stands alone: a failure is
    recorded under `error` and the headline fields are untouched."""
    import gc
    import importlib.util
    sec = {"note": budget_note}

    def guarded(name, fn):
        t0 = time.perf_counter()
        try:
            sec[name] = fn()
        except Exception as e:     # noqa: BLE001 - a secondary measurement must never take the headline down
            sec[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        sec[name]["seconds_spent"] = round(time.perf_counter() - t0, 1)
        gc.collect()
        torch.cuda.empty_cache()
    guarded("train", lambda: _time_train(device, steps=10, warmup=4))
    guarded("train_lossaware", lambda: dict(_time_train(device, steps=10, warmup=4, sampler="lossaware"),
                                            note="the reference's default schedule sampler (config/train.py:38-39): its per-micro-batch update is a "
                                                 "device -> pinned-host copy applied when the next draw reads the state, no host sync between forward and backward"))
    guarded("c2_fp32", lambda: dict(_time_loop(WORKLOADS["c2"], "fp32", device, steps=20, warmup=3),
                                    note="compute_dtype='fp32': the mode whose final tokens equal the reference's bit for bit (tests/test_diffusion_gpu.py)"))
    for mode in ("bf16x3", "f16x3"):
        guarded("c2_" + mode, lambda mode=mode: dict(_time_loop(WORKLOADS["c2"], mode, device, steps=20, warmup=3),
                                                     note="compute_dtype=%r: split precision (csrc/split.hip) - every value as hi + lo 16-bit parts, three matrix-pipe products "
                                                          "per reference product, fp32 sums; the golden loops end on the reference's tokens bit for bit in this mode too" % mode))
    guarded("c2_bertbase", lambda: dict(_time_loop(WORKLOADS["c2-bertbase"], "bf16", device, steps=60, warmup=5),
                                        note="the reference-true width (network.py:44: d_model 768, 12 heads, ffn 3072), same batch"))
    guarded("ref_default", lambda: dict(_time_loop(WORKLOADS["ref-default"], "bf16", device, steps=30, warmup=3),
                                        note="the reference's own shipped shape: seq_len 2096, embedding dim 500, bert-base encoder; 16 sequences (33 536 tokens per step)"))

    def agreement():
        spec = importlib.util.spec_from_file_location("drift_c2", os.path.join(REPO, "tools", "drift_c2.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        rs = mod.run(steps=2000, batch=64, segment="first", modes=("bf16", "bf16x3", "f16x3"), light=True)
        r = rs["bf16"]
        out = {"value": round(r["final_token_agreement"], 5), "unit": "share of generated positions whose final argmax token equals the fp32 mode's",
               "steps": 2000, "agreement_min_over_steps": round(r["agreement_min"], 5), "free_positions": r["free_positions"],
               "final_tokens_differing": r["final_tokens_differing"],
               "how": "tools/drift_c2.py: config 2 at full size, same weights, same start latent, same Philox noise, ALL 2000 p_sample iterations "
                      "(t = 1999 .. 0) in bf16 (and bf16x3, f16x3) and in fp32 mode; random-init weights put many positions on near-ties, "
                      "trained ones would not (the released checkpoints are unreachable from here)"}
        for mode in ("bf16x3", "f16x3"):
            out[mode] = {"value": round(rs[mode]["final_token_agreement"], 6), "final_tokens_differing": rs[mode]["final_tokens_differing"],
                         "agreement_min_over_steps": round(rs[mode]["agreement_min"], 6), "first_step_with_a_differing_token": rs[mode]["first_step_with_a_differing_token"]}
        return out
    guarded("bf16_token_agreement", agreement)
    return sec


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 200: 0.8 s of replay; train: 10; c3: fixed by the config)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16x3", "f16x3"])
    ap.add_argument("--rng", default="philox", choices=["philox", "torch"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--sampler", default="uniform", choices=["uniform", "lossaware"], help="train: the timestep sampler (lossaware = the reference's default)")
    ap.add_argument("--full", action="store_true", help="also what is measured beside the headline: roofline + kernels, cpu_baseline, secondary + parity_mode "
                                                        "(N = 1 config 2), repeated timed regions, the all-reduce's exposed time (train, N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--repeats", type=int, default=None, help="sampling workloads: further back-to-back repetitions of the timed region, reported in config.repeats (value = the median region; default 4 with --full, else 0)")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the `secondary` object (train / fp32 / bertbase / token agreement) of the N = 1 config-2 line")
    ap.add_argument("--accum", type=int, default=1, help="train: micro-batches per optimizer step (the reference's batch_size // microbatch)")
    ap.add_argument("--split", type=int, default=None, help="batch slices run as concurrent graph branches (default: the library's choice)")
    ap.add_argument("--gemm", type=int, default=None, help="bf16 GEMM kernel variant 0 / 2 / 4 (see mh_gemm_set_variant)")
    ap.add_argument("--no-fuse-ln", action="store_true", help="A/B: separate GEMM and LayerNorm kernels")
    ap.add_argument("--defer-ln", type=int, default=None, help="A/B: deferred LayerNorm 0 never / 1 where no fused epilogue exists (default) / 2 always")
    ap.add_argument("--no-stream-attn", action="store_true", help="A/B: LDS-resident attention instead of the streaming kernel")
    ap.add_argument("--no-decouple", action="store_true", help="A/B: one graph per step with a fork / join of the batch slices instead of one free-running graph per slice (the default where the fused step boundary runs)")
    ap.add_argument("--decouple", action="store_true", help="A/B: force the free-running graphs (widths without the fused boundary default to the fork / join)")
    ap.add_argument("--skew-us", type=int, default=None, help="phase lag between the decoupled batch-slice chains in microseconds (default: half a step)")
    args = ap.parse_args(argv)
    if args.steps is None:
        args.steps = {"train": 10}.get(args.workload, 200)
    if not args.full:      # a plain run does what its headline needs and nothing else
        args.no_cpu_baseline = args.no_kernel_timing = args.no_secondary = True
    if args.repeats is None:
        args.repeats = 4 if args.full else 0
    return args


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus, sys.argv[1:])          # does not return
    world, rank, local_rank, device = init_ranks(args)
    import torch.distributed as dist

    if args.workload == "train":
        return train_main(args, world, rank, local_rank, device)
    if args.workload in ("c3", "c4"):
        return sampling_main(args, world, rank, local_rank, device)
    from functools import partial
    from musediffusion_amd import _lib, sharding, synthetic
    from musediffusion_amd.models.diffusion import _ReverseLoop
    from musediffusion_amd.models.rounding import denoised_fn_round

    if args.gemm is not None or args.no_fuse_ln or args.defer_ln is not None or args.no_stream_attn:
        _lib.use_debug_library()      # an A/B flag: the switches exist in libmusehip_dbg.so only (include/musehip_dbg.h); the default run is the production library
    if args.gemm is not None:
        _lib.lib().mh_gemm_set_variant(args.gemm)
    if args.no_fuse_ln:
        _lib.lib().mh_denoiser_set_fuse_ln(0)
    if args.defer_ln is not None:
        _lib.lib().mh_denoiser_set_defer_ln(args.defer_ln)
    if args.no_stream_attn:
        _lib.lib().mh_attention_set_stream(0)
    c = WORKLOADS[args.workload]
    model, diff = build(c, args.dtype, device, seed=rank)     # different weights per rank until the broadcast
    arena_sum = None
    if world > 1:
        sharding.broadcast_weights(model, src=0, packed=True)   # ONE RCCL broadcast of the packed arena
        arena_sum = sharding.weights_checksum(model)
        assert_same_on_all_ranks(arena_sum, "weight arena checksum after the broadcast", world, device)
    ev = dist_evidence(world, device, local_rank)
    diff.rng_mode, diff.rng_seed, diff.rng_stream = args.rng, 105, rank
    diff.use_graph = not args.no_graph
    if args.split is not None:
        diff.batch_split = args.split
    if args.no_decouple:
        diff.decouple_branches = False
    if args.decouple:
        diff.decouple_branches = True
    if args.skew_us is not None:
        diff.branch_skew_us = args.skew_us

    total = args.warmup + args.steps
    PROF_STEPS = 4
    # `repeats`: the same K-step region timed again, back to back in the same loop, so that the line carries its own spread (boxes of the
    # pool differ by several percent and a 20-step region is 72 ms; `value` is the MEDIAN region - each region is exactly K steps between a barrier + synchronize pair, as the contract times them)
    reps = max(0, min(args.repeats, (c["T"] - 16 - total - PROF_STEPS) // max(1, args.steps)))
    loop = make_loop(model, diff, c, "p", device, rank, total + reps * args.steps + PROF_STEPS + 2)
    rep_ms = []
    with torch.no_grad():
        loop.begin()
        for k in range(args.warmup):
            loop.advance(k)

        def timed():
            for k in range(args.warmup, total):
                loop.advance(k)
        elapsed, _ = timed_region(timed, world, device)
        for r in range(reps):
            k0 = total + r * args.steps

            def again():
                for k in range(k0, k0 + args.steps):
                    loop.advance(k)
            el, _ = timed_region(again, world, device)
            rep_ms.append(el / args.steps * 1e3)
        total += reps * args.steps
        loop.finish()
    tokens = model.argmax_tokens(loop.x)       # the loop's product: discrete tokens (run/sample.py:219-220)
    assert tokens.shape == (c["B"], c["L"]) and bool(torch.isfinite(loop.x).all())
    all_tokens = sharding.gather_rows(tokens, c["B"] * world)      # one token all-gather (run/sample.py:288-291)
    assert all_tokens.shape == (c["B"] * world, c["L"])
    assert_same_on_all_ranks(int(all_tokens.sum().item()), "gathered token checksum", world, device)
    if args.dump_outputs and rank == 0:
        # what the loop hands its caller (_ReverseLoop.run: sample, pred_xstart of this rank's batch) and the tokens made of it
        dump_outputs(args.dump_outputs, {"sample": loop.x, "pred_xstart": loop.pred, "tokens": all_tokens})

    if rank == 0:
        first_ms = elapsed / args.steps * 1e3
        # `value` = the MEDIAN of the back-to-back K-step regions (each bracketed by the barrier + synchronize of timed_region and reduced
        # with MAX over ranks): the first region alone was a sample of one inside a 1 - 2 % run-to-run spread.  Every region's
        # own figure stays in config.repeats
        regions = sorted([first_ms] + rep_ms)
        ms_per_step = regions[len(regions) // 2] if len(regions) % 2 else 0.5 * (regions[len(regions) // 2 - 1] + regions[len(regions) // 2])
        value = world * 1e3 / ms_per_step
        flops = step_flops(c)
        out = {
            "metric": "denoiser-steps/sec (seq_len=%d, batch=%d)" % (c["L"], c["B"]),
            "value": round(value, 3), "unit": "denoiser-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "p_sample_loop step, %s: seq_len=%d batch=%d/GPU d_model=%d layers=%d heads=%d "
                                   "ffn=%d E=%d vocab=%d T=%d, rounding+clamp+top_p=1 every step"
                                   % (args.workload, c["L"], c["B"], c["H"], c["nL"], c["nh"], c["F"], c["E"], c["V"], c["T"]),
                       "global_batch": c["B"] * world, "seq_len": c["L"], "parallelism": "batch-sharded x%d" % world,
                       "backend": ev["backend"], "rccl_ranks": ev["rccl_ranks"], "devices": ev["devices"], "distinct_devices": ev["distinct_devices"],
                       "arena_checksum_after_broadcast": None if arena_sum is None else int(arena_sum),
                       "rng": args.rng, "hipgraph": not args.no_graph, "graph_branches": int(loop.nsplit),
                       "decoupled_branches": bool(loop.decoupled), "branch_skew_us": int(getattr(loop, "skew_us", 0)),
                       "host_launches_per_step": int(loop.nsplit) if not args.no_graph else None,
                       "host_launches_note": "hipGraphLaunch calls per reverse step and process (one captured graph per batch slice); nothing else is "
                                             "enqueued from the host inside the timed region",
                       "repeats": {"regions": 1 + len(rep_ms), "steps_each": args.steps,
                                   "ms_per_step": [round(first_ms, 4)] + [round(v, 4) for v in rep_ms],
                                   "median_ms": round(ms_per_step, 4), "first_region_ms": round(first_ms, 4),
                                   "min_ms": round(min([first_ms] + rep_ms), 4), "max_ms": round(max([first_ms] + rep_ms), 4),
                                   "note": "the K-step timed region repeated back to back in the same loop; value / ms_per_step = the MEDIAN region"},
                       "step_tflop": round(flops / 1e12, 4),
                       "step_tflops_achieved": round(flops / (ms_per_step * 1e-3) / 1e12, 2),
                       "sequences_steps_per_s": round(value * c["B"], 1)},
        }
        run_secondary = world == 1 and args.workload == "c2" and args.dtype == "bf16" and not args.no_secondary and not args.no_graph
        if run_secondary:
            # right after the headline's timed region (its two-chain loops choose their streams by an overlap probe: DESIGN section 5,
            # "Streams are not queues")
            secondary = secondary_block(device)
        if not args.no_kernel_timing:
            out["roofline"], out["kernels"] = step_tables(loop, c, args, ms_per_step, total, PROF_STEPS)
            if args.dtype in ("bf16", "fp32"):
                iso_ms, iso_f, _, _ = time_dominant_kernel(c, args.dtype, device, reps=5, branches=int(loop.nsplit))
                out["roofline"]["isolated"] = {"avg_launch_ms": round(iso_ms, 5), "achieved": round(iso_f / (iso_ms * 1e-3) / 1e12, 2),
                                               "note": "secondary: the full-row GEMM + LayerNorm kernel alone in a loop on fresh operands"}
        if not args.no_cpu_baseline and world == 1:     # the host baseline is a rank-0, N = 1 measurement
            out["cpu_baseline"] = cpu_baseline(c)
            out["cpu_baseline"]["value"] = round(out["cpu_baseline"]["value"], 5)
        if run_secondary:
            out["secondary"] = secondary
            # The headline dtype (bf16: what BASELINE.json configs[1] names) is NOT token-exact: first class next to it, the fastest mode
            # whose final tokens equal the fp32 mode's - the north_star's "bit-exact for the final argmax / clamp token rounding"
            pm, agree = secondary.get("c2_f16x3", {}), secondary.get("bf16_token_agreement", {})
            if "value" in pm:
                differing = agree.get("f16x3", {}).get("final_tokens_differing")
                out["parity_mode"] = {"dtype": "f16x3", "value": pm["value"], "unit": pm["unit"], "ms_per_step": pm["ms_per_step"],
                                      "tokens_exact": None if differing is None else differing == 0,
                                      "final_tokens_differing_from_fp32_mode": differing, "checked_over_steps": agree.get("steps"),
                                      "headline_dtype_final_tokens_differing": None if "value" not in agree else
                                      int(round((1.0 - agree["value"]) * agree.get("free_positions", 0))),
                                      "note": "compute_dtype='f16x3' (split fp16 hi + lo, three matrix-pipe products per product, fp32 sums): same workload, "
                                              "same procedure as `value` on a 20-step region; the golden loops of tests/test_diffusion_gpu.py end on the "
                                              "reference's tokens bit for bit in this mode, the bf16 headline mode does not (bf16_token_agreement)"}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
