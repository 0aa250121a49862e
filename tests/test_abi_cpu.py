"""The ctypes binding is derived from include/musehip.h and include/musehip_dbg.h by musediffusion_amd/_abi.py.  A parser cannot vouch
for itself, so the compiler does: every derived struct layout and every derived signature is turned into a static_assert over the real
headers.  Also: what the reader cannot parse raises instead of being guessed or skipped, and optim.py's numpy images of the optimizer's
device tables have the layouts of mh_opt_chunk / mh_opt_tensor."""
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
