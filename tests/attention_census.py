"""Shared helpers of the attention census and parity matrix (imported by test modules; not a conftest).

* `census_key`: (kernel text, launch note) -> census key of an attention-family launch.  Every instantiation of the streaming forward is
  launched through one function pointer, so the recorder's kernel text is `kern` for all of them: the key is built from the note's
  `key=value` fields, which name the instantiation (csrc/attention_stream.hip: stream_fwd_impl; csrc/attention_bwd.hip: launch_bwd).
* `record`: tests/gemm_census.py's recorder for this family -> [(key, note, grid)].
* `fwd_key` / `bwd_keys`: the keys of a streaming variant, as the matrix and PARITY spell them.
* `WORKLOADS`: the GEMM census' eager runs plus one forward at the reference's own shape (seq_len 2096: the key-bound forward)."""
import gemm_census as gc

FWD_FIELDS = ("dh", "nw", "sk", "dropv", "full", "kvnt", "pre")
BWD_FIELDS = ("dh", "drop", "full", "opanel", "dpanel")
BWD_KERNELS = ("attn_bwd_dq_kernel", "attn_bwd_dkv_kernel")
SMALL_KERNELS = ("attn_bf16_kernel", "attn_res_bf16_kernel", "attn_f32_kernel")
OTHER_KERNELS = ("attn_bwd_rowdot_kernel", "attn_stream2_kernel", "split_attn_kernel")


def fields(note):
    return dict(t.split("=", 1) for t in note.split() if "=" in t)


def _fmt(kv, names):
    return " ".join("%s=%s" % (n, kv.get(n, "?")) for n in names)


def census_key(kernel, note):
    """(kernel text, launch note) -> census key, or None for a kernel outside the attention family"""
    name = " ".join(kernel.strip().strip("()").split())
    base = name.split("<")[0].strip()
    kv = fields(note)
    if name == "kern" and note.startswith("attn_stream "):
        return "attn_stream_bf16_kernel | " + _fmt(kv, FWD_FIELDS)
    if base in BWD_KERNELS:
        return "%s | %s" % (base, _fmt(kv, BWD_FIELDS))
    if base in SMALL_KERNELS:
        return "%s | kind=%s dh=%s" % (name, kv.get("kind", "?"), kv.get("dh", "?"))
    if base in OTHER_KERNELS:
        return name
    return None


def fwd_key(dh, nw=16, sk=256, dropv=0, full=0, kvnt=0, pre=0):
    return "attn_stream_bf16_kernel | " + _fmt(dict(dh=dh, nw=nw, sk=sk, dropv=dropv, full=int(full), kvnt=int(kvnt), pre=int(pre)), FWD_FIELDS)


def bwd_keys(dh, drop, full, panel):
    kv = dict(dh=dh, drop=int(drop), full=int(full), opanel=int(panel), dpanel=int(panel))
    return ["%s | %s" % (k, _fmt(kv, BWD_FIELDS)) for k in BWD_KERNELS]


def record(fn):
    """fn() with the per-launch recorder on -> [(key, note, grid)] of its attention-family launches, in launch order"""
    return gc.record_family(fn, census_key)


def items(note):
    """the `items=` field of a streaming launch's note: (batch, head, query or key block) work items the persistent blocks walk"""
    return int(fields(note)["items"])


def _with(run):
    return lambda dev: run(dev, record)


# name -> run(device) -> [(key, note, grid)]
WORKLOADS = {name: _with(run) for name, run in gc.WORKLOADS.items()}
WORKLOADS["fwd ref-default bf16"] = _with(gc._forward("ref-default", "bf16"))

# the workloads bench.py times in the persistent multi-item regime: more items than blocks in every streaming launch
MULTI_ITEM = ("fwd c2 bf16", "fwd ref-default bf16", "train 32x1024 dropout 0.1")
# the op-per-node tape at seq_len 128 with dropout materialises P (batched GEMMs + row softmax + the bit mask): no attention kernel
NO_ATTENTION_KERNEL = ("train 8x128 (op-per-node tape)",)
