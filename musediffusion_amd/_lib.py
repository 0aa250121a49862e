"""ctypes binding of libmusehip.so (C ABI: include/musehip.h, include/musehip_data.h for the dataset loader and
include/musehip_eval.h for the evaluation of sampled batches, include/musehip_stats.h for the pair statistics of a set,
include/musehip_infill.h for the infill mask and splice, include/musehip_harmony.h for the chord-fit counts,
include/musehip_grammar.h for the grammar-constrained rounding, include/musehip_region.h for the rounding of infill regions,
include/musehip_solver.h for the multistep DPM-Solver++ reverse step, include/musehip_structure.h for the structure counts,
include/musehip_arrange.h for the interplay counts of the tracks of a song).

There is no fallback: `lib()` raises if the shared library is absent or does not export the
symbols the header declares.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C musediffusion_amd/csrc`.
"""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree build.  Another build is taken ONLY under the explicit A/B switch of tools/ab_lib.sh
# (MUSEHIP_AB=1 MUSEHIP_LIB=<path>): a stray MUSEHIP_LIB alone changes nothing
LIB_PATH = os.path.join(_HERE, "csrc", "libmusehip.so")
if os.environ.get("MUSEHIP_AB") == "1" and os.environ.get("MUSEHIP_LIB"):
    LIB_PATH = os.environ["MUSEHIP_LIB"]

# The header is the single source of the ABI: signatures, struct layouts and enum values are read from it (_abi.py), not restated here
_H = _abi.load("musehip.h")
_DBG_H = _abi.load("musehip_dbg.h", _H)
_DATA_H = _abi.load("musehip_data.h", _H)
_EVAL_H = _abi.load("musehip_eval.h", _H)
_STATS_H = _abi.load("musehip_stats.h", _H)
_INFILL_H = _abi.load("musehip_infill.h", _H)
_HARMONY_H = _abi.load("musehip_harmony.h", _H)
_GRAMMAR_H = _abi.load("musehip_grammar.h", _H)
_REGION_H = _abi.load("musehip_region.h", _H)
_SOLVER_H = _abi.load("musehip_solver.h", _H)
_STRUCTURE_H = _abi.load("musehip_structure.h", _H)
_ARRANGE_H = _abi.load("musehip_arrange.h", _H)

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

# name -> (restype, argtypes): every symbol include/musehip.h declares; a pointer argument is c_void_p (char*: c_char_p)
SIGNATURES = _H.protos
# include/musehip_dbg.h: exported by libmusehip_dbg.so only (A/B switches, ablation knobs, diagnostics)
DBG_SIGNATURES = _DBG_H.protos
# include/musehip_data.h: the dataset loader's mhd_* entry points and their status enums, exported by both libraries
DATA_SIGNATURES = _DATA_H.protos
DATA_ENUMS = _DATA_H.enums
# include/musehip_eval.h: the mhe_* entry points (fused MSIM nearest neighbour), exported by both libraries
EVAL_SIGNATURES = _EVAL_H.protos
EVAL_ENUMS = _EVAL_H.enums
# include/musehip_stats.h: the mhs_* entry points (pair statistics under MSIM), exported by both libraries
STATS_SIGNATURES = _STATS_H.protos
# include/musehip_infill.h: the mhi_* entry points (infill mask and splice) and enum mhi_status, exported by both libraries
INFILL_SIGNATURES = _INFILL_H.protos
INFILL_ENUMS = _INFILL_H.enums
# include/musehip_harmony.h: the mhh_* entry point (chord-fit counts of decoded rows) and enum mhh_status, exported by both libraries
HARMONY_SIGNATURES = _HARMONY_H.protos
HARMONY_ENUMS = _HARMONY_H.enums
# include/musehip_grammar.h: the mhg_* entry points (class winners, row Viterbi), struct mhg_classes and its enums, exported by both libraries
GRAMMAR_SIGNATURES = _GRAMMAR_H.protos
GRAMMAR_ENUMS = _GRAMMAR_H.enums
GrammarClasses = _GRAMMAR_H.structs["mhg_classes"]
# include/musehip_region.h: the mhr_* entry point (whole-note rounding of an infill plan's regions) and enum mhr_status, exported by both libraries
REGION_SIGNATURES = _REGION_H.protos
REGION_ENUMS = _REGION_H.enums
# include/musehip_solver.h: the mhv_* entry point (DPM-Solver++(2M) update of a reverse step) and struct mhv_solver_coef, exported by both libraries
SOLVER_SIGNATURES = _SOLVER_H.protos
SolverCoef = _SOLVER_H.structs["mhv_solver_coef"]
# include/musehip_structure.h: the mhm_* entry point (per-bar pitch-class entropy and groove counts of decoded rows) and enum mhm_status, exported by both libraries
STRUCTURE_SIGNATURES = _STRUCTURE_H.protos
STRUCTURE_ENUMS = _STRUCTURE_H.enums
# include/musehip_arrange.h: the mha_* entry points (interplay counts of the rows of a song, the tile they are staged in) and enum mha_status, exported by both libraries
ARRANGE_SIGNATURES = _ARRANGE_H.protos
ARRANGE_ENUMS = _ARRANGE_H.enums

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
    for name, (res, args) in signatures.items():
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
        _lib = _load(LIB_PATH, {**SIGNATURES, **DATA_SIGNATURES, **EVAL_SIGNATURES, **STATS_SIGNATURES, **INFILL_SIGNATURES, **HARMONY_SIGNATURES, **GRAMMAR_SIGNATURES, **REGION_SIGNATURES, **SOLVER_SIGNATURES, **STRUCTURE_SIGNATURES, **ARRANGE_SIGNATURES}, "libmusehip.so")
    return _lib


def use_debug_library(on=True):
    """Route every later call of this process through libmusehip_dbg.so (-DMH_ABLATE: the same kernels plus the switches of
    include/musehip_dbg.h) or back to the production library.  For tools/, bench.py's A/B flags and tests that compare kernel forms;
    the product never calls this.  Each library has its own switch state; objects made under one (captured graphs, engines' arenas)
    are plain HIP objects and stay valid under the other."""
    global _lib
    _lib = (_load(DBG_LIB_PATH, {**SIGNATURES, **DATA_SIGNATURES, **EVAL_SIGNATURES, **STATS_SIGNATURES, **INFILL_SIGNATURES, **HARMONY_SIGNATURES, **GRAMMAR_SIGNATURES, **REGION_SIGNATURES, **SOLVER_SIGNATURES, **STRUCTURE_SIGNATURES, **ARRANGE_SIGNATURES, **DBG_SIGNATURES}, "libmusehip_dbg.so") if on else
            _load(LIB_PATH, {**SIGNATURES, **DATA_SIGNATURES, **EVAL_SIGNATURES, **STATS_SIGNATURES, **INFILL_SIGNATURES, **HARMONY_SIGNATURES, **GRAMMAR_SIGNATURES, **REGION_SIGNATURES, **SOLVER_SIGNATURES, **STRUCTURE_SIGNATURES, **ARRANGE_SIGNATURES}, "libmusehip.so"))
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


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MuseHipError("musediffusion_amd runs on the GPU only: got a %s tensor "
                               "(move the model and inputs to cuda; there is no CPU path)" % t.device)
