"""The ctypes binding is derived from the headers under include/ by musediffusion_amd/_abi.py: musehip.h and the entry-point families
beside it (_lib.HEADERS), and musehip_dbg.h.  A parser cannot vouch for itself, so the compiler does: every derived struct layout, every
derived signature and every derived enum value is turned into a static_assert over the real headers, and a wrong table fails the same
translation unit.  FACTS pins, per header, what its entry points are.  Also: what the reader cannot parse raises instead of being guessed
or skipped, the tables are disjoint and both loaded libraries carry them, and optim.py's numpy images of the optimizer's device tables
have the layouts of mh_opt_chunk / mh_opt_tensor."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import REPO

from musediffusion_amd import _abi, _lib

PRELUDE = """
#include <cstddef>
#include <tuple>
#include <type_traits>
#include "musehip.h"
#include "musehip_dbg.h"
// class of a type (1 pointer, 2 floating, 3 signed integer, 4 unsigned integer; 0 anything else) * 100 + its size
template <class T> constexpr int cls() {
  return (std::is_pointer<T>::value ? 1 : std::is_floating_point<T>::value ? 2 : !std::is_integral<T>::value ? 0 :
          std::is_signed<T>::value ? 3 : 4) * 100 + int(sizeof(T));
}
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
  static constexpr int arity = sizeof...(A);
  static constexpr int ret = cls<R>();
  template <int I> static constexpr int arg = cls<std::tuple_element_t<I, std::tuple<A...>>>();
};
"""


def cls(ct):
    """the class * 100 + size code of PRELUDE's cls<T>() for a ctypes scalar or pointer type"""
    code = getattr(ct, "_type_", None)
    if not isinstance(code, str):
        assert issubclass(ct, C._Pointer), ct
        kind = 1
    else:
        kind = 1 if code in "Pz" else 2 if code in "fd" else 3 if code in "bhilq" else 4 if code in "BHILQ" else 0
    assert kind, ct
    return kind * 100 + C.sizeof(ct)


def translation_unit(structs, protos):
    out = [PRELUDE]
    for name, st in structs.items():
        out.append('static_assert(sizeof(%s) == %d, "sizeof %s");' % (name, C.sizeof(st), name))
        for fname, ft in st._fields_:
            f = getattr(st, fname)
            out.append('static_assert(offsetof(%s, %s) == %d && sizeof(%s::%s) == %d, "%s.%s: offset / size");'
                       % (name, fname, f.offset, name, fname, f.size, name, fname))
            if not issubclass(ft, (C.Array, C.Structure)):
                out.append('static_assert(cls<decltype(%s::%s)>() == %d, "%s.%s: class");' % (name, fname, cls(ft), name, fname))
    for name, (res, args) in protos.items():
        s = "sig<decltype(&%s)>" % name
        out.append('static_assert(%s::arity == %d, "%s: arity");' % (s, len(args), name))
        out.append('static_assert(%s::ret == %d, "%s: return type");' % (s, cls(res), name))
        for i, a in enumerate(args):
            out.append('static_assert(%s::arg<%d> == %d, "%s: argument %d");' % (s, i, cls(a), name, i))
    return "\n".join(out) + "\n"


def compile_check(source, path):
    """host-only syntax pass with the compiler the Makefile uses; a missing compiler is a failure, not a skip"""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: it built the library, so it must be here"
    path.write_text(source)
    return subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-fsyntax-only", "-ferror-limit=0", "-I", os.path.join(REPO, "include"), str(path)],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def derived():
    h = _abi.load("musehip.h")
    return h, _abi.load("musehip_dbg.h", h)


def test_lib_serves_the_derived_tables(derived):
    h, dbg = derived
    assert len(h.protos) == 157 and len(dbg.protos) == 20 and len(h.structs) == 14 and not dbg.structs
    for tab, ref in ((_lib.SIGNATURES, h.protos), (_lib.DBG_SIGNATURES, dbg.protos)):
        assert list(tab) == list(ref)
        assert all(tab[n][0] is ref[n][0] and tab[n][1] == ref[n][1] for n in ref)
    for py, c in (("StepCoef", "mh_step_coef"), ("LoopState", "mh_loop_state"), ("OptHParams", "mh_opt_hparams"), ("Dropout", "mh_dropout"),
                  ("StepRng", "mh_step_rng"), ("StepUpdate", "mh_step_update"), ("WPrepItem", "mh_wprep_item"), ("GemmDesc", "mh_gemm_desc"),
                  ("TrainLayer", "mh_train_layer"), ("LayerWeights", "mh_layer_weights"), ("LnDefer", "mh_ln_defer"), ("Denoiser", "mh_denoiser")):
        assert [(n, getattr(getattr(_lib, py), n).offset) for n, _ in getattr(_lib, py)._fields_] == \
            [(n, getattr(h.structs[c], n).offset) for n, _ in h.structs[c]._fields_]
    S = _lib
    assert (C.sizeof(S.TrainLayer), C.sizeof(S.GemmDesc), C.sizeof(S.Denoiser)) == (416, 184, 184)
    # type rules: a field that points to a known struct is POINTER(struct), every other pointer c_void_p; arguments c_void_p / c_char_p
    assert S.StepUpdate.rng.size == 8 and dict(S.StepUpdate._fields_)["rng"] is C.POINTER(S.StepRng)
    assert dict(S.GemmDesc._fields_)["drop"] is C.POINTER(S.Dropout) and dict(S.Denoiser._fields_)["layers"] is C.POINTER(S.LayerWeights)
    assert dict(S.StepUpdate._fields_)["coef"] is C.c_void_p and _abi.DEVICE_STRUCT_FIELDS == {("mh_step_update", "coef")}   # a device table
    assert dict(S.TrainLayer._fields_)["drop_ao"] is S.Dropout and dict(S.OptHParams._fields_)["ema_rate"] is C.c_float * 4
    assert dict(h.structs["mh_opt_tensor"]._fields_)["ema"] is C.c_void_p * 4 and dict(S.TrainLayer._fields_)["side_stream"] is C.c_void_p
    assert S.SIGNATURES["mh_last_error"] == (C.c_char_p, []) and S.SIGNATURES["mh_device_name"] == (C.c_int, [C.c_int, C.c_char_p, C.c_int])
    assert S.SIGNATURES["mh_train_layer_fwd"] == (C.c_int, [C.c_void_p, C.c_void_p]) and S.SIGNATURES["mh_stream_delay"][1][0] is C.c_uint
    assert S.SIGNATURES["mh_train_layer_grad_floats"][0] is C.c_int64 and S.SIGNATURES["mh_round_workspace_bytes"][0] is C.c_size_t
    assert S.SIGNATURES["mh_graph_end_capture"][1] == [C.c_void_p, C.c_void_p]
    # enum values come from the header
    assert (S.MH_F32, S.MH_BF16, S.MH_BF16X3, S.MH_F16X3) == (0, 1, 2, 3) and (S.MH_ERR_INVALID, S.MH_ERR_HIP, S.MH_ERR_UNSUPPORTED) == (-1, -2, -3)
    assert (S.ACT_NONE, S.ACT_TANH, S.ACT_GELU_ERF, S.ACT_SILU, S.ACT_DERIV) == (0, 1, 2, 3, 4)
    assert h.enums["MH_DECODE_OVERFLOW"] == 7 and h.enums["MH_ENCODE_OVERFLOW"] == 5 and len(h.enums) == 27
    from musediffusion_amd import ops, training
    assert training.ACT_DERIV is S.ACT_DERIV and ops.ACT == {None: 0, "none": 0, "tanh": 1, "gelu": 2, "silu": 3}


def test_compiler_agrees_with_every_derived_layout_and_signature(derived, tmp_path):
    h, dbg = derived
    r = compile_check(translation_unit(h.structs, {**h.protos, **dbg.protos}), tmp_path / "abi_check.cpp")
    assert r.returncode == 0, r.stderr[-4000:]


def test_compiler_check_catches_a_wrong_table(derived, tmp_path):
    """the control of the test above: the mistakes the hand-written tables could hide each fail the same translation unit"""
    h, _ = derived
    protos = copy.deepcopy({n: h.protos[n] for n in ("mh_repack_panel", "mh_split_attention", "mh_train_layer_grad_floats", "mh_trunc_normal")})
    assert protos["mh_repack_panel"][1][1] is C.c_int64
    protos["mh_repack_panel"][1][1] = C.c_int                  # an INT where the header says int64_t
    del protos["mh_split_attention"][1][12]                    # a dropped argument far down a long list
    protos["mh_train_layer_grad_floats"] = (C.c_int, protos["mh_train_layer_grad_floats"][1])
    protos["mh_trunc_normal"][1][3] = C.c_int64                # signed for uint64_t
    tl = h.structs["mh_train_layer"]
    short = type("mh_train_layer", (C.Structure,), {"_fields_": [f for f in tl._fields_ if f[0] != "bits_in"]})   # a field not mirrored
    sr = h.structs["mh_step_rng"]
    swapped = type("mh_step_rng", (C.Structure,), {"_fields_": [(n, C.c_uint32 if n == "bound" else t) for n, t in sr._fields_]})
    r = compile_check(translation_unit({"mh_train_layer": short, "mh_step_rng": swapped}, protos), tmp_path / "abi_wrong.cpp")
    assert r.returncode != 0
    for msg in ("mh_repack_panel: argument 1", "mh_split_attention: arity", "mh_train_layer_grad_floats: return type",
                "mh_trunc_normal: argument 3", "sizeof mh_train_layer", "mh_train_layer.y_panel: offset / size", "mh_step_rng.bound: class"):
        assert msg in r.stderr, msg
    assert "mh_repack_panel: argument 0" not in r.stderr and "mh_step_rng.seed" not in r.stderr


# ------------------------------------------------------------------------------------------------------------------ every header
P, I, I64, Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
# One row per header of _lib.HEADERS - a new entry-point family adds its row.  prefix: what every name of the header starts with;
# protos: the names in the header's order (musehip.h: their number); enums: every enumerator; structs: the struct names; pins:
# signatures spelled out.  The controls of the compiler pass: mutate = (function, argument, a type of another class or size, the text
# of the neighbour that must NOT be named); arity = (function, None: one int more | k: argument k dropped); enum = (enumerator, a wrong
# value); lines = further static_asserts that hold with the header included
FACTS = {
    "musehip.h": dict(prefix="mh_", protos=157),
    "musehip_data.h": dict(
        prefix="mhd_", protos=["mhd_gather_offsets", "mhd_gather_rows", "mhd_select_rows", "mhd_augment_rows"], structs=[],
        enums={"MHD_GATHER_OK": 0, "MHD_GATHER_BAD_INDEX": 1, "MHD_GATHER_OVERFLOW": 2, "MHD_AUGMENT_OK": 0, "MHD_AUGMENT_NOT_ORIGIN": 1,
               "MHD_AUGMENT_PITCH_RANGE": 2, "MHD_AUGMENT_BAD_ROW": 3},
        pins={"mhd_gather_offsets": (I, [P, I64, P, P, P, P, I, I64, P])},
        mutate=("mhd_gather_rows", 2, C.c_int, "mhd_select_rows"), arity=("mhd_augment_rows", 5)),
    "musehip_eval.h": dict(
        prefix="mhe_", protos=["mhe_msim_nearest", "mhe_nearest_key_tile"], structs=[], enums={},
        pins={"mhe_msim_nearest": (I, [P, I64, P, I64, P, P, I, P, P, P, P]), "mhe_nearest_key_tile": (I, [])},
        mutate=("mhe_msim_nearest", 1, C.c_int, "mhe_msim_nearest: argument 0"), arity=("mhe_nearest_key_tile", None)),
    "musehip_stats.h": dict(
        prefix="mhs_", protos=["mhs_msim_pair_stats", "mhs_pair_key_tile"], structs=[], enums={},
        pins={"mhs_msim_pair_stats": (I, [P, I64, P, I64, P, P, P, P, I, C.c_float, P, P, P, P, P]), "mhs_pair_key_tile": (I, [])},
        mutate=("mhs_msim_pair_stats", 9, C.c_double, "mhs_msim_pair_stats: argument 8"),       # the threshold is a float
        arity=("mhs_pair_key_tile", None)),
    "musehip_infill.h": dict(
        prefix="mhi_", protos=["mhi_infill_plan", "mhi_infill_splice"], structs=[],
        enums={"MHI_OK": 0, "MHI_NO_EOS": 1, "MHI_BAD_MASK": 2, "MHI_BAD_RANGE": 3, "MHI_OVERFLOW": 4},
        pins={"mhi_infill_plan": (I, [P, P, P, P, I, I, P, P, P, P, I, I, P]), "mhi_infill_splice": (I, [P, P, P, P, I, P, P, I, I, P])},
        mutate=("mhi_infill_plan", 4, I64, "mhi_infill_plan: argument 5"),                      # room is an int
        arity=("mhi_infill_splice", None), enum=("MHI_OVERFLOW", 3)),
    "musehip_harmony.h": dict(
        prefix="mhh_", protos=["mhh_harmony_counts"], structs=[], enums={"MHH_OK": 0, "MHH_MASKED": 1, "MHH_BAD_META": 2, "MHH_BAD_COUNTS": 3},
        pins={"mhh_harmony_counts": (I, [P] * 9 + [I] * 4 + [P])},
        mutate=("mhh_harmony_counts", 9, I64, "mhh_harmony_counts: argument 8"),                # B is an int
        arity=("mhh_harmony_counts", None), enum=("MHH_BAD_COUNTS", 2)),
    "musehip_grammar.h": dict(
        prefix="mhg_", protos=["mhg_note_classes", "mhg_class_argmax", "mhg_constrain_workspace_bytes", "mhg_constrain_rows"],
        structs=["mhg_classes"],
        enums={"MHG_PAD": 0, "MHG_EOS": 1, "MHG_BAR": 2, "MHG_PITCH": 3, "MHG_VELOCITY": 4, "MHG_DURATION": 5, "MHG_POSITION": 6,
               "MHG_ANY": 7, "MHG_BARS_EXACT": 0, "MHG_BARS_DECODABLE": 1, "MHG_OK": 0, "MHG_BAD_MASK": 1, "MHG_NO_CHORDS": 2,
               "MHG_TOO_MANY_BARS": 3, "MHG_BAD_BOUNDS": 4, "MHG_NO_ROOM": 5, "MHG_NONFINITE": 6},
        pins={"mhg_note_classes": (I, [P]), "mhg_class_argmax": (I, [P] * 6 + [I64, I, I, I, P]),
              "mhg_constrain_workspace_bytes": (Z, [I, I]), "mhg_constrain_rows": (I, [P] * 6 + [I] + [P] * 5 + [Z, I, I, P])},
        mutate=("mhg_class_argmax", 6, I, "mhg_class_argmax: argument 5"),                      # n_tokens is an int64
        arity=("mhg_constrain_rows", None), enum=("MHG_NONFINITE", 5)),
    "musehip_region.h": dict(
        prefix="mhr_", protos=["mhr_constrain_regions"], structs=[],
        enums={"MHR_OK": 0, "MHR_NOT_PLANNED": 1, "MHR_BAD_PLAN": 2, "MHR_NONFINITE": 3, "MHR_NO_ROOM": 4},
        pins={"mhr_constrain_regions": (I, [P] * 5 + [I] + [P] * 4 + [I, I, P])},
        mutate=("mhr_constrain_regions", 5, I64, "mhr_constrain_regions: argument 4"),          # fields is an int
        arity=("mhr_constrain_regions", None), enum=("MHR_NO_ROOM", 3),
        lines=['static_assert(MHG_ANY == 7, "the header brings enum mhg_class with it");']),
    "musehip_solver.h": dict(
        prefix="mhv_", protos=["mhv_dpmpp_epilogue"], structs=["mhv_solver_coef"], enums={},
        pins={"mhv_dpmpp_epilogue": (I, [P] * 6 + [I, P, P, I, I, P, I, P, P, P, I, I64, I, P])},
        mutate=("mhv_dpmpp_epilogue", 17, I, "mhv_dpmpp_epilogue: argument 16"),                # per_batch is an int64_t
        arity=("mhv_dpmpp_epilogue", None)),
    "musehip_structure.h": dict(
        prefix="mhm_", protos=["mhm_structure_counts"], structs=[], enums={"MHM_OK": 0, "MHM_MASKED": 1, "MHM_BAD_META": 2, "MHM_BAD_COUNTS": 3},
        pins={"mhm_structure_counts": (I, [P] * 9 + [I] * 3 + [P])},
        mutate=("mhm_structure_counts", 9, I64, "mhm_structure_counts: argument 8"),            # B is an int
        arity=("mhm_structure_counts", None), enum=("MHM_BAD_COUNTS", 2)),
    "musehip_arrange.h": dict(
        prefix="mha_", protos=["mha_interplay_counts", "mha_key_tile"], structs=[],
        enums={"MHA_OK": 0, "MHA_MASKED": 1, "MHA_BAD_COUNTS": 2, "MHA_BAD_SHIFT": 3, "MHA_MIXED": 4},
        pins={"mha_interplay_counts": (I, [P] * 10 + [I] * 2 + [P]), "mha_key_tile": (I, [])},
        mutate=("mha_interplay_counts", 10, I64, "mha_interplay_counts: argument 9"),           # B is an int
        arity=("mha_interplay_counts", None), enum=("MHA_MIXED", 3)),
}
FAMILIES = _lib.HEADERS[1:]


def header_unit(name, structs, protos, enums=None, lines=()):
    """translation_unit with the header included and one static_assert per enumerator"""
    checks = ['static_assert(%s == %d, "%s");' % (k, v, k) for k, v in (enums or {}).items()]
    return '#include "%s"\n' % name + "\n".join(checks + list(lines)) + "\n" + translation_unit(structs, protos)


def test_every_header_has_its_row_and_the_mapping_is_what_the_reader_gives(derived):
    assert list(FACTS) == list(_lib.HEADERS) and _lib.HEADERS[0] == "musehip.h" and "musehip_dbg.h" not in _lib.HEADERS
    base = derived[0]
    for name in _lib.HEADERS:
        got, ref = _lib.ABI[name], _abi.load(name, base if name != "musehip.h" else None)
        assert list(got.protos) == list(ref.protos) and got.enums == ref.enums and list(got.structs) == list(ref.structs), name
        assert all(got.protos[n][0] is ref.protos[n][0] and got.protos[n][1] == ref.protos[n][1] for n in ref.protos), name
        for s in ref.structs:
            assert [(n, getattr(got.structs[s], n).offset) for n, _ in got.structs[s]._fields_] == \
                [(n, getattr(ref.structs[s], n).offset) for n, _ in ref.structs[s]._fields_], s
    assert _lib.SIGNATURES is _lib.ABI["musehip.h"].protos
    assert _lib.GrammarClasses is _lib.ABI["musehip_grammar.h"].structs["mhg_classes"] and C.sizeof(_lib.GrammarClasses) == 56
    assert _lib.SolverCoef is _lib.ABI["musehip_solver.h"].structs["mhv_solver_coef"]


def test_tables_are_disjoint_and_counted():
    """the number of entry points of every header, pinned once; no name in two tables; a header's names carry its prefix alone"""
    counts = {name: len(_lib.ABI[name].protos) for name in _lib.HEADERS}
    assert counts == {"musehip.h": 157, "musehip_data.h": 4, "musehip_eval.h": 2, "musehip_stats.h": 2, "musehip_infill.h": 2,
                      "musehip_harmony.h": 1, "musehip_grammar.h": 4, "musehip_region.h": 1, "musehip_solver.h": 1,
                      "musehip_structure.h": 1, "musehip_arrange.h": 2}
    assert len(_lib.DBG_SIGNATURES) == 20
    tables = [_lib.ABI[name].protos for name in _lib.HEADERS] + [_lib.DBG_SIGNATURES]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    assert len(_lib.PRODUCT_SIGNATURES) == sum(counts.values()) == 177
    assert list(_lib.PRODUCT_SIGNATURES) == [n for name in _lib.HEADERS for n in _lib.ABI[name].protos]
    assert all(_lib.PRODUCT_SIGNATURES[n] is _lib.ABI[name].protos[n] for name in _lib.HEADERS for n in _lib.ABI[name].protos)
    prefixes = [FACTS[name]["prefix"] for name in _lib.HEADERS]
    assert len(set(prefixes)) == len(prefixes)
    for name in _lib.HEADERS:
        assert all(n.startswith(FACTS[name]["prefix"]) for n in _lib.ABI[name].protos), name
    assert all(n.startswith("mh_") for n in _lib.DBG_SIGNATURES)
    with pytest.raises(_abi.AbiError, match="mh_twice"):                 # the merge refuses a name that two headers declare
        _lib._merged(({"mh_once": 1, "mh_twice": 2}, {"mh_twice": 3}))


@pytest.mark.parametrize("name", FAMILIES)
def test_header_declares_what_is_pinned(name):
    d, f = _lib.ABI[name], FACTS[name]
    assert list(d.protos) == f["protos"] and d.enums == f["enums"] and list(d.structs) == f["structs"]
    for fn, sig in f["pins"].items():
        assert d.protos[fn] == sig, fn


@pytest.mark.parametrize("name", _lib.HEADERS)
def test_compiler_agrees_with_the_header(name, tmp_path):
    d, f = _lib.ABI[name], FACTS[name]
    assert len(d.protos) == (f["protos"] if name == "musehip.h" else len(f["protos"]))
    r = compile_check(header_unit(name, d.structs, d.protos, d.enums, f.get("lines", ())), tmp_path / "abi.cpp")
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("name", FAMILIES)
def test_compiler_check_catches_a_wrong_table_of_the_header(name, tmp_path):
    """the controls of the test above: a wrong argument class is named and its neighbour is not, a wrong arity and a wrong enumerator fail"""
    d, f = _lib.ABI[name], FACTS[name]
    fn, k, wrong_type, unnamed = f["mutate"]
    assert cls(wrong_type) != cls(d.protos[fn][1][k])
    wrong = {n: (res, list(args)) for n, (res, args) in d.protos.items()}
    wrong[fn][1][k] = wrong_type
    r = compile_check(header_unit(name, {}, wrong), tmp_path / "abi_wrong.cpp")
    assert r.returncode != 0 and "%s: argument %d" % (fn, k) in r.stderr and unnamed not in r.stderr
    fn, k = f["arity"]
    wrong = {n: (res, list(args)) for n, (res, args) in d.protos.items()}
    if k is None:
        wrong[fn][1].append(C.c_int)
    else:
        del wrong[fn][1][k]
    r = compile_check(header_unit(name, {}, wrong), tmp_path / "abi_arity.cpp")
    assert r.returncode != 0 and "%s: arity" % fn in r.stderr and unnamed not in r.stderr
    if "enum" in f:
        enumerator, value = f["enum"]
        assert d.enums[enumerator] != value
        r = compile_check(header_unit(name, {}, {}, {enumerator: value}), tmp_path / "abi_enum_wrong.cpp")
        assert r.returncode != 0 and enumerator in r.stderr
    else:
        assert name in ("musehip_data.h", "musehip_eval.h", "musehip_stats.h", "musehip_solver.h")


def test_what_single_headers_add(derived, tmp_path):
    """grammar and region: the restatements' classes and statuses are the headers' (region's slots are enum mhg_class of the header it
    includes); solver: its coefficient row has the size mh_step_advance copies, and a wrong size fails; stats: a double is legal behind a
    pointer only"""
    import grammar_ref as gr
    import region_ref as rr
    h = derived[0]
    grammar, region = _lib.ABI["musehip_grammar.h"].enums, _lib.ABI["musehip_region.h"].enums
    classes = ("PAD", "EOS", "BAR", "PITCH", "VELOCITY", "DURATION", "POSITION", "ANY")
    assert [getattr(gr, n) for n in gr.STATUS_NAMES] == [grammar["MHG_" + n] for n in gr.STATUS_NAMES]
    assert (gr.PAD, gr.EOS, gr.BAR, gr.PITCH, gr.VELOCITY, gr.DURATION, gr.POSITION, gr.ANY) == tuple(grammar["MHG_" + n] for n in classes)
    assert [getattr(rr, n) for n in rr.STATUS_NAMES] == [region["MHR_" + n] for n in rr.STATUS_NAMES]
    assert (rr.PAD, rr.EOS, rr.BAR, rr.PITCH, rr.VELOCITY, rr.DURATION, rr.POSITION, rr.ANY) == tuple(grammar["MHG_" + n] for n in classes)
    st = _lib.SolverCoef
    assert C.sizeof(st) == 32 == C.sizeof(h.structs["mh_step_coef"])             # mh_step_advance copies a row of either alike
    assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [("a", 0), ("b", 4), ("c", 8), ("reserved", 12)]
    r = compile_check(header_unit("musehip_solver.h", {}, {}, lines=['static_assert(sizeof(mhv_solver_coef) == 16, "mhv_solver_coef");']),
                      tmp_path / "solver_struct_wrong.cpp")
    assert r.returncode != 0 and "mhv_solver_coef" in r.stderr
    with pytest.raises(_abi.AbiError):
        _abi.parse("int mhs_bad(double threshold);", h)


def test_both_loaded_libraries_carry_the_derived_tables():
    """every function of the product tables on the loaded handle has the derived types; the debug library has every product name and
    its own; the tile getters answer alike in both (what the libraries export: tests/test_host_cpu.py)"""
    handle = _lib.lib()
    for fn_name, (res, args) in _lib.PRODUCT_SIGNATURES.items():
        fn = getattr(handle, fn_name)
        assert fn.restype is res and list(fn.argtypes) == args, fn_name
    assert handle.mh_abi_version() == 1
    assert handle.mhe_nearest_key_tile() > 0 and handle.mhe_nearest_key_tile() * 56 * 4 <= 32 << 10
    assert handle.mhs_pair_key_tile() == handle.mhe_nearest_key_tile() and handle.mha_key_tile() == 512
    with _lib.debug_library() as dbg:
        assert dbg is not handle and all(hasattr(dbg, n) for n in _lib.PRODUCT_SIGNATURES) and all(hasattr(dbg, n) for n in _lib.DBG_SIGNATURES)
        for getter in ("mhe_nearest_key_tile", "mhs_pair_key_tile", "mha_key_tile"):
            assert getattr(dbg, getter)() == getattr(handle, getter)(), getter
    assert _lib.lib() is handle


GOOD = "typedef void* mh_stream_t; typedef struct mh_s { int a; const float *p, *q; float r[4]; } mh_s;\n" \
       "enum mh_e { MH_A = 0,\n /* note */ MH_B = -3 };\nsize_t mh_f(const mh_s* s, char* buf,\n  unsigned n, mh_stream_t st); // end\nint mh_g(void);\n"


def test_reader_reads_the_forms_the_headers_use():
    h = _abi.parse('#ifdef __cplusplus\nextern "C" {\n#endif\n' + GOOD + '#ifdef __cplusplus\n}\n#endif\n')
    assert h.enums == {"MH_A": 0, "MH_B": -3} and list(h.structs) == ["mh_s"]
    assert h.structs["mh_s"]._fields_ == [("a", C.c_int), ("p", C.c_void_p), ("q", C.c_void_p), ("r", C.c_float * 4)]
    assert h.protos == {"mh_f": (C.c_size_t, [C.c_void_p, C.c_char_p, C.c_uint, C.c_void_p]), "mh_g": (C.c_int, [])}
    more = _abi.parse("typedef struct mh_t { mh_s s; const mh_s* ps; mh_stream_t st; } mh_t; int mh_h(const mh_t* t);", h)
    assert more.structs["mh_t"]._fields_ == [("s", h.structs["mh_s"]), ("ps", C.POINTER(h.structs["mh_s"])), ("st", C.c_void_p)]
    assert list(more.protos) == ["mh_h"]


@pytest.mark.parametrize("text, names", [
    ("int mh_bad_arg(mh_nothing* x, int n);", ("mh_bad_arg", "mh_nothing")),                       # unknown type name behind a pointer
    ("int mh_bad_val(double x);", ("mh_bad_val", "double")),                                      # ... and by value
    ("typedef struct mh_bad_s { int a; wchar_t c; } mh_bad_s;", ("mh_bad_s", "wchar_t")),         # ... and in a struct
    ("int mh_bad_cb(void (*cb)(int), int n);", ("mh_bad_cb",)),                                   # function-pointer parameter
    ("typedef struct mh_bad_bits { int a : 3; int b; } mh_bad_bits;", ("mh_bad_bits", "a : 3")),  # bit-field
    ("int mh_bad_unnamed(unsigned);", ("mh_bad_unnamed", "unsigned")),                            # would have to guess: type or name?
    ("int mh_bad_value_struct(mh_s s);", ("mh_bad_value_struct", "mh_s")),                        # struct by value
    ("enum mh_bad_e { MH_X, MH_Y = 2 };", ("mh_bad_e", "MH_X")),                                  # implicit enumerator value
    ("int mh_g(void);", ("mh_g", "twice")),                                                       # already declared by the base header
    ("#define MH_N 3\nstatic const int mh_bad_const = 3;", ("mh_bad_const",)),                    # not a declaration kind the ABI has
    ("int mh_bad_open(int a)", ("mh_bad_open",)),                                                 # no terminating semicolon
], ids=["unknown-pointee", "unknown-value", "unknown-field", "function-pointer", "bit-field", "unnamed", "struct-by-value", "implicit-enum",
        "redeclared", "other-declaration", "unterminated"])
def test_reader_raises_on_what_it_cannot_read(text, names):
    base = _abi.parse(GOOD)
    with pytest.raises(_abi.AbiError) as e:
        _abi.parse(text, base)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_optimizer_tables_have_the_header_layouts(derived):
    from musediffusion_amd import optim
    chunk, tensor = derived[0].structs["mh_opt_chunk"], derived[0].structs["mh_opt_tensor"]
    dt = optim.CHUNK_DTYPE
    assert dt.itemsize == C.sizeof(chunk) == 16 and list(dt.names) == [n for n, _ in chunk._fields_]
    for n, _ in chunk._fields_:
        f = getattr(chunk, n)
        assert (dt.fields[n][1], dt.fields[n][0].itemsize, dt.fields[n][0].kind) == (f.offset, f.size, "i"), n
    assert optim.TENSOR_ROW * 8 == C.sizeof(tensor) == 64
    assert [(n, getattr(tensor, n).offset) for n, _ in tensor._fields_] == [("param", 0), ("grad", 8), ("exp_avg", 16), ("exp_avg_sq", 24), ("ema", 32)]
