"""ctypes binding of libmusehip.so.  The C ABI is the headers under include/ that HEADERS names: musehip.h for the model side and one
header per entry-point family beside it, each with a prefix of its own (mhd_, mhe_, ...) and exported by both libraries; the
extension families of EXTENSION_HEADERS (prefixes of two letters: mhac_, ...) are read and bound the same way.

There is no fallback: `lib()` raises if the shared library is absent or does not export the
symbols the headers declare.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C musediffusion_amd/csrc`.
"""
import collections
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree build.  Another build is taken ONLY under the explicit A/B switch of tools/ab_lib.sh
# (MUSEHIP_AB=1 MUSEHIP_LIB=<path>): a stray MUSEHIP_LIB alone changes nothing
LIB_PATH = os.path.join(_HERE, "csrc", "libmusehip.so")
if os.environ.get("MUSEHIP_AB") == "1" and os.environ.get("MUSEHIP_LIB"):
    LIB_PATH = os.environ["MUSEHIP_LIB"]

# The headers both libraries export, in load order: musehip.h, whose types the others use, then one per entry-point family.  A new
# family is one more name here ("Adding an entry-point family")
HEADERS = ("musehip.h", "musehip_data.h", "musehip_eval.h", "musehip_stats.h", "musehip_infill.h", "musehip_harmony.h", "musehip_grammar.h",
           "musehip_region.h", "musehip_solver.h", "musehip_structure.h", "musehip_arrange.h")
# The headers are the single source of the ABI: signatures, struct layouts and enum values are read from them (_abi.py), not restated here.
# header name -> its .protos (name -> (restype, argtypes); a pointer argument is c_void_p, char*: c_char_p), .structs and .enums
_H = _abi.load(HEADERS[0])
ABI = {HEADERS[0]: _H, **{name: _abi.load(name, _H) for name in HEADERS[1:]}}


def _merged(tables):
    out = {}
    for protos in tables:
        twice = set(out) & set(protos)
        if twice:
            raise _abi.AbiError("declared by two headers: %s" % ", ".join(sorted(twice)))
        out.update(protos)
    return out


# every symbol libmusehip.so exports
PRODUCT_SIGNATURES = _merged(h.protos for h in ABI.values())
# every symbol include/musehip.h declares
SIGNATURES = _H.protos
# The EXTENSION families: headers of entry points that both libraries export as well, under prefixes of two letters (mhac_, ...), read
# by the same _abi.load and bound by the same _load.  They stand in a tuple and a table of their own: HEADERS, the number of prototypes
# per header and PRODUCT_SIGNATURES are pinned by tests/test_abi_cpu.py and tests/test_host_cpu.py, whose export pattern (mh_ and at
# most one letter more) does not claim a two-letter prefix.  A new family is one more name HERE ("Adding an entry-point
# family")
EXTENSION_HEADERS = ("musehip_choose.h",)
EXTENSION_ABI = {name: _abi.load(name, _H) for name in EXTENSION_HEADERS}
EXTENSION_SIGNATURES = _merged(h.protos for h in EXTENSION_ABI.values())
_merged((PRODUCT_SIGNATURES, EXTENSION_SIGNATURES))          # raises on a name that stands in both tables
# include/musehip_dbg.h: exported by libmusehip_dbg.so only (A/B switches, ablation knobs, diagnostics)
DBG_SIGNATURES = _abi.load("musehip_dbg.h", _H).protos

MH_ERR_INVALID, MH_ERR_HIP, MH_ERR_UNSUPPORTED = (_H.enums["MH_ERR_" + n] for n in ("INVALID", "HIP", "UNSUPPORTED"))
MH_F32, MH_BF16, MH_BF16X3, MH_F16X3 = (_H.enums["MH_" + n] for n in ("F32", "BF16", "BF16X3", "F16X3"))
ACT_NONE, ACT_TANH, ACT_GELU_ERF, ACT_SILU, ACT_DERIV = (_H.enums["MH_ACT_" + n] for n in ("NONE", "TANH", "GELU_ERF", "SILU", "DERIV"))

StepCoef = _H.structs["mh_step_coef"]
LoopState = _H.structs["mh_loop_state"]
OptHParams = _H.structs["mh_opt_hparams"]
Dropout = _H.structs["mh_dropout"]
StepRng = _H.structs["mh_step_rng"]
StepUpdate = _H.structs["mh_step_update"]
WPrepItem = _H.structs["mh_wprep_item"]
GemmDesc = _H.structs["mh_gemm_desc"]
TrainLayer = _H.structs["mh_train_layer"]
LayerWeights = _H.structs["mh_layer_weights"]
LnDefer = _H.structs["mh_ln_defer"]
Denoiser = _H.structs["mh_denoiser"]
GrammarClasses = ABI["musehip_grammar.h"].structs["mhg_classes"]
SolverCoef = ABI["musehip_solver.h"].structs["mhv_solver_coef"]

_lib = None
_handles = {}


class MuseHipError(RuntimeError):
    pass


DBG_LIB_PATH = os.path.join(_HERE, "csrc", "libmusehip_dbg.so")


def _load(path, signatures, what):
    if path in _handles:
        return _handles[path]
    if not os.path.exists(path):
        raise MuseHipError(
            "%s not found at %s: the HIP kernels are the only compute path "
            "(build with `make -C musediffusion_amd/csrc` or __graft_entry__.build())" % (what, path))
    # PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Import torch
    # FIRST so the library's DT_NEEDED entry resolves to that already-loaded runtime: two HIP
    # runtimes in one process do not share devices, streams or allocations.
    import torch  # noqa: F401
    handle = C.CDLL(path)
    for name, (res, args) in {**signatures, **EXTENSION_SIGNATURES}.items():   # both libraries export the extension families
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise MuseHipError("%s does not export %s (stale build?)" % (what, name))
        fn.restype = res
        fn.argtypes = args
    _handles[path] = handle
    return handle


def lib():
    """The loaded library (cached).  Raises MuseHipError when it cannot be loaded.  This is the production build unless the caller
    switched to the debug build (use_debug_library / debug_library)."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, PRODUCT_SIGNATURES, "libmusehip.so")
    return _lib


def use_debug_library(on=True):
    """Route every later call of this process through libmusehip_dbg.so (-DMH_ABLATE: the same kernels plus the switches of
    include/musehip_dbg.h) or back to the production library.  For tools/, bench.py's A/B flags and tests that compare kernel forms;
    the product never calls this.  Each library has its own switch state; objects made under one (captured graphs, engines' arenas)
    are plain HIP objects and stay valid under the other."""
    global _lib
    _lib = (_load(DBG_LIB_PATH, _merged((PRODUCT_SIGNATURES, DBG_SIGNATURES)), "libmusehip_dbg.so") if on else
            _load(LIB_PATH, PRODUCT_SIGNATURES, "libmusehip.so"))
    return _lib


class debug_library:
    """`with _lib.debug_library(): ...` - the debug build for the duration of the block."""

    def __enter__(self):
        self.prev = _lib
        return use_debug_library(True)

    def __exit__(self, *a):
        global _lib
        _lib = self.prev


def check(rc, what=""):
    if rc != 0:
        msg = lib().mh_last_error()
        raise MuseHipError("%s failed (%d): %s" % (what or "libmusehip call", rc, msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


LaunchRecord = collections.namedtuple("LaunchRecord", "kernel detail grid block stream ms")


def record_launches(fn):
    """fn() between mh_profile_start and mh_profile_stop -> one LaunchRecord per kernel the library launched meanwhile, in launch order.
    The fields are those of the report line (include/musehip.h): kernel text as launched, detail, blocks and threads in x, stream, and
    milliseconds between the two events around the launch.  The recorder's events cannot be captured, so this refuses inside a graph
    capture; it measures and tests, the product never calls it."""
    import torch
    L = lib()
    if torch.cuda.is_current_stream_capturing():
        raise MuseHipError("the launch recorder must not run inside a graph capture")
    torch.cuda.synchronize()
    check(L.mh_profile_start(), "mh_profile_start")
    try:
        fn()
    finally:
        # mh_profile_stop keeps its records until the next start and returns the bytes the whole report needs, whatever it was given: the
        # first call stops the recorder and asks, the second fetches - no size to guess for the longest run
        need = L.mh_profile_stop(None, 0)
        buf = C.create_string_buffer(max(need, 1))
        got = L.mh_profile_stop(buf, len(buf))
    if not 0 < need == got:
        raise MuseHipError("mh_profile_stop failed (%d, then %d)" % (need, got))
    out = []
    for line in buf.value.decode().splitlines():
        kernel, detail, grid, block, stream, ms = line.split("\t")
        out.append(LaunchRecord(kernel, detail, int(grid), int(block), stream, float(ms)))
    return out


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MuseHipError("musediffusion_amd runs on the GPU only: got a %s tensor "
                               "(move the model and inputs to cuda; there is no CPU path)" % t.device)
