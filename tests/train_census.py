"""Shared helpers of the training-kernel census and parity matrix (imported by test modules; not a conftest).

* `FAMILY`: every `__global__` kernel of csrc/train.hip, read from the source.
* `census_key`: (kernel text, launch note) -> census key.  The recorder's kernel text carries the template arguments as launched
  (`ln_bwd_kernel<bf16, 1, true>`, `colsum8_partial_kernel<float>`); where a kernel's path depends on a runtime argument the text does not
  show, the launch note does and the key takes the class of it that selects the path: the LayerNorm backward's second-output form, the head
  permutes' mode, whether the partial fold's unrolled loop runs (P > 48) and whether it accumulates, the scatter's chunk form and column
  passes, the squared error's vector or scalar loop, the number of EMA copies of the optimizer step (`chunks=%d n_ema=%d`: it selects one of
  the five adamw_ema_chunk<NEMA> instantiations, `ADAM_KEYS`).
* `record`: tests/gemm_census.py's recorder for this family -> [(key, note, grid)].
* `WORKLOADS`: the GEMM census' training runs, the seq_len 128 run again in fp32 (the only place the `float` instantiations are launched),
  and one optimizer step (clip + AdamW / EMA + gradient norm), all eager."""
import os
import re

import gemm_census as gc

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musediffusion_amd", "csrc", "train.hip")
with open(_SRC) as _f:
    FAMILY = tuple(sorted(set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", _f.read()))))


def fields(note):
    return dict(t.split("=", 1) for t in note.split() if "=" in t)


def fold_key(P, acc):
    return "colsum_final_kernel | P%s48 acc=%d" % (">" if int(P) > 48 else "<=", int(acc))


def ln_key(T, lnch, drop_build, panel=0, always=0, drop=0):
    """T: "bf16" / "float"; drop_build: the instantiation that writes the second output"""
    if not drop_build:
        return "ln_bwd_kernel<%s, %d>" % (T, lnch)
    return "ln_bwd_kernel<%s, %d, true> | panel=%d always=%d drop=%d" % (T, lnch, panel, always, drop)


def scatter_key(chunks, E):
    return "scatter_rows_partial_kernel | chunks%s32 passes=%d" % ("=" if int(chunks) == 32 else "<", (int(E) + 255) // 256)


def adam_key(n_ema):
    return "adamw_ema_kernel | n_ema=%d" % int(n_ema)


# the five instantiations of adamw_ema_chunk<NEMA> the kernel's switch selects from mh_opt_hparams.n_ema
ADAM_KEYS = tuple(adam_key(k) for k in range(5))


def census_key(kernel, note):
    """(kernel text, launch note) -> census key, or None for a kernel outside csrc/train.hip"""
    name = " ".join(kernel.strip().strip("()").split())
    base = name.split("<")[0].strip()
    if base not in FAMILY:
        return None
    kv = fields(note)
    if base == "ln_bwd_kernel" and name.endswith("true>"):
        return "%s | panel=%s always=%s drop=%s" % (name, kv.get("panel", "?"), kv.get("always", "?"), kv.get("drop", "?"))
    if base in ("head_permute_kernel", "head_permute8_kernel", "head_transpose_kernel"):
        return "%s | mode=%s" % (name, kv.get("mode", "?"))
    if base == "colsum_final_kernel":
        return fold_key(kv.get("P", -1), kv.get("acc", -1)) if "P" in kv else name + " | P=? acc=?"
    if base == "scatter_rows_partial_kernel":
        return scatter_key(kv["chunks"], kv["E"]) if "chunks" in kv else name + " | chunks=? passes=?"
    if base == "sqdiff_mean_kernel":
        return "%s | vec=%s" % (name, kv.get("vec", "?"))
    if base == "adamw_ema_kernel":
        return "%s | n_ema=%s" % (name, kv.get("n_ema", "?"))
    return name


def record(fn):
    """fn() with the per-launch recorder on -> [(key, note, grid)] of its train.hip launches, in launch order"""
    return gc.record_family(fn, census_key)


def keys_of(fn):
    return [k for k, _, _ in record(fn)]


def _with(run):
    return lambda dev: run(dev, record)


def _train_fp32(dev):
    """the `c1` micro-step (op-per-node tape) with compute_dtype "fp32" """
    import torch
    from musediffusion_amd import synthetic
    bench = gc._bench()
    c = dict(bench.WORKLOADS["c1"])
    model, diff = bench.build(c, "fp32", dev, seed=0)
    model.dropout.p = 0.1
    model.bert_hidden_dropout = model.bert_attention_dropout = 0.1
    model.train().requires_grad_(True)
    batch = {k: v.to(dev) for k, v in synthetic.training_batch(c["B"], c["L"], seed=1).items()}
    t = torch.randint(0, c["T"], (c["B"],), generator=torch.Generator().manual_seed(7)).to(dev)

    def step():
        model.zero_grad(set_to_none=True)
        diff.training_losses(model, t, model_kwargs=batch)["loss"].mean().backward()
    step()
    return record(step)


def _optimizer_step(dev):
    """clip + step + gradient norm of FusedAdamWEMA on the `c1` model after one backward"""
    import torch
    from musediffusion_amd import synthetic
    from musediffusion_amd.optim import FusedAdamWEMA
    bench = gc._bench()
    c = dict(bench.WORKLOADS["c1"])
    model, diff = bench.build(c, "bf16", dev, seed=0)
    model.train().requires_grad_(True)
    batch = {k: v.to(dev) for k, v in synthetic.training_batch(c["B"], c["L"], seed=1).items()}
    t = torch.randint(0, c["T"], (c["B"],), generator=torch.Generator().manual_seed(7)).to(dev)
    opt = FusedAdamWEMA(model.parameters(), lr=1e-4, weight_decay=0.01, ema_rates=(0.9999,))
    diff.training_losses(model, t, model_kwargs=batch)["loss"].mean().backward()

    def step():
        opt.clip_grad_norm(1.0)
        opt.step()
        opt.grad_norm()
    return record(step)


TRAINING = ("train 32x1024 dropout 0.1", "train 32x1024 dropout 0", "train 8x128 (op-per-node tape)")
# name -> run(device) -> [(key, note, grid)]
WORKLOADS = {name: _with(gc.WORKLOADS[name]) for name in TRAINING}
WORKLOADS["train 8x128 fp32"] = _train_fp32
WORKLOADS["optimizer step"] = _optimizer_step
