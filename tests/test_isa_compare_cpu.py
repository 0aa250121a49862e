"""tools/isa_compare.py: the kernel-by-kernel comparison of two builds' gfx950 machine code.  Two tiny kernels cross-compiled for
gfx950 are `identical` against themselves, a copy with one changed vector operation `differs`, and the `scalar-only` class - the one
that needs a compiler's scheduling to occur - is checked on two canned disassembly texts."""
import importlib.util
import os
import shutil
import subprocess

import pytest

from conftest import REPO

spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(REPO, "tools", "isa_compare.py"))
isa_compare = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_compare)

AXPY = """
#include <hip/hip_runtime.h>
__global__ void axpy_kernel(const float* x, float* y, float a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = a * x[i] %s y[i];
}
"""
FILL = """
#include <hip/hip_runtime.h>
template <typename T> __global__ void fill_kernel(T* y, T v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = v;
}
template __global__ void fill_kernel<float>(float*, float, int);
"""


def compile_objects(directory, axpy_op):
    """axpy.o and fill.o for gfx950, with the compiler the Makefile uses; a missing compiler is a failure, not a skip"""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: it built the library, so it must be here"
    os.makedirs(directory)
    for name, text in (("axpy", AXPY % axpy_op), ("fill", FILL)):
        src = os.path.join(directory, name + ".hip")
        with open(src, "w") as f:
            f.write(text)
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", os.path.join(directory, name + ".o")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    root = tmp_path_factory.mktemp("isa")
    dirs = {"a": str(root / "a"), "same": str(root / "same"), "changed": str(root / "changed")}
    compile_objects(dirs["a"], "+")
    compile_objects(dirs["same"], "+")
    compile_objects(dirs["changed"], "-")   # one vector operation: v_fma -> v_fma with a negated operand / v_sub
    return dirs


def run_tool(capsys, a, b):
    status = isa_compare.main(["isa_compare.py", a, b])
    return status, capsys.readouterr().out.splitlines()


def test_a_build_is_identical_to_itself_and_to_a_second_build_of_the_same_sources(builds, capsys):
    for other in ("a", "same"):
        status, lines = run_tool(capsys, builds["a"], builds[other])
        assert status == 0, lines
        kernel_lines = lines[:-1]
        assert len(kernel_lines) == 2 and all(ln.startswith("identical ") for ln in kernel_lines), lines
        assert any("axpy.o: " in ln and "axpy_kernel(float const*, float*, float, int)" in ln for ln in kernel_lines), lines   # demangled
        assert any("fill.o: " in ln and "fill_kernel<float>" in ln for ln in kernel_lines), lines
        assert lines[-1] == "total: 2 identical, 0 scalar-only, 0 differs; 0 kernel-set differences"


def test_one_changed_vector_operation_differs(builds, capsys):
    status, lines = run_tool(capsys, builds["a"], builds["changed"])
    assert status == 1
    assert [ln.split()[0] for ln in lines[:-1]] == ["differs", "identical"], lines   # axpy.o, fill.o
    assert lines[-1] == "total: 1 identical, 0 scalar-only, 1 differs; 0 kernel-set differences"


def test_a_missing_kernel_or_object_is_a_kernel_set_difference(builds, capsys, tmp_path):
    only_axpy = tmp_path / "only_axpy"
    only_axpy.mkdir()
    shutil.copy(os.path.join(builds["a"], "axpy.o"), only_axpy)
    status, lines = run_tool(capsys, builds["a"], str(only_axpy))
    assert status == 1
    assert any(ln.startswith("object only in ") and ln.endswith("fill.o") for ln in lines), lines
    assert lines[-1] == "total: 1 identical, 0 scalar-only, 0 differs; 1 kernel-set differences"


def test_metadata_of_a_kernel_is_read(builds):
    kernels = isa_compare.load_object(os.path.join(builds["a"], "axpy.o"))
    (meta, text), = kernels.values()
    assert set(meta) == set(isa_compare.META_KEYS)
    assert meta["vgpr_count"] > 0 and meta["sgpr_count"] > 0 and meta["vgpr_spill_count"] == 0 and meta["max_flat_workgroup_size"] == 1024
    assert text[-1] == "s_endpgm" and any(ins.startswith("global_store_dword ") for ins in text)
    assert not any("//" in ins for ins in text)   # no addresses, no encodings


# llvm-objdump -d, as it prints it: the same kernel twice, the scalar prologue in another order and other scalar registers; then with
# one vector instruction changed; then with one instruction more
CANNED_A = """
0000000000001900 <k>:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0                         // 000000001900: C0060080 00000000
\ts_load_dword s4, s[0:1], 0x8                               // 000000001908: C0020100 00000008
\ts_getpc_b64 s[6:7]                                         // 000000001910: BE861C00
\ts_add_u32 s6, s6, 0xffff9e18                               // 000000001914: 8006FF06 FFFF9E18
\ts_addc_u32 s7, s7, -1                                      // 00000000191C: 8207FF07 FFFFFFFF
\tv_lshlrev_b32_e32 v1, 2, v0                                // 000000001924: 24020082
\ts_waitcnt lgkmcnt(0)                                       // 000000001928: BF8CC07F
\tv_add_u32_e32 v2, s4, v1                                   // 00000000192C: 68040204
\ts_cbranch_execz 12                                         // 000000001930: BF88000C <k+0x64>
\tglobal_store_dword v2, v1, s[2:3]                          // 000000001934: DC708000 00020102
\ts_endpgm                                                   // 00000000193C: BF810000
"""
CANNED_SCALAR = """
0000000000002a00 <k>:
\ts_load_dword s8, s[0:1], 0x8                               // 000000002A00: C0020200 00000008
\ts_load_dwordx2 s[4:5], s[0:1], 0x0                         // 000000002A08: C0060100 00000000
\ts_getpc_b64 s[6:7]                                         // 000000002A10: BE861C00
\ts_add_u32 s6, s6, 0xffff8d18                               // 000000002A14: 8006FF06 FFFF8D18
\ts_addc_u32 s7, s7, -1                                      // 000000002A1C: 8207FF07 FFFFFFFF
\tv_lshlrev_b32_e32 v1, 2, v0                                // 000000002A24: 24020082
\ts_waitcnt lgkmcnt(0)                                       // 000000002A28: BF8CC07F
\tv_add_u32_e32 v2, s8, v1                                   // 000000002A2C: 68040208
\ts_cbranch_execz 14                                         // 000000002A30: BF88000E <k+0x6c>
\tglobal_store_dword v2, v1, s[4:5]                          // 000000002A34: DC708000 00040102
\ts_endpgm                                                   // 000000002A3C: BF810000
"""
META = dict.fromkeys(isa_compare.META_KEYS, 0)


def canned(text):
    return META, isa_compare.normalise(text)["k"]


def test_scalar_only_class_on_canned_disassembly():
    a, s = canned(CANNED_A), canned(CANNED_SCALAR)
    assert a[1][3] == "s_add_u32 s6, s6, <pcrel>" and a[1][8] == "s_cbranch_execz <disp>"
    assert isa_compare.classify(a, a)[0] == "identical"
    # the same text at another address, with another pc-relative literal and another branch displacement, is the same text
    moved = canned(CANNED_A.replace("0xffff9e18", "0xffff0018").replace("s_cbranch_execz 12", "s_cbranch_execz 40"))
    assert isa_compare.classify(a, moved)[0] == "identical"
    cls, detail = isa_compare.classify(a, s)
    assert cls == "scalar-only" and detail.startswith("11 instructions, 4 lines differ"), detail
    # a vector instruction that differs in more than a scalar register number
    v = canned(CANNED_SCALAR.replace("v_lshlrev_b32_e32 v1, 2, v0", "v_lshlrev_b32_e32 v1, 3, v0"))
    assert isa_compare.classify(a, v)[0] == "differs"
    v = canned(CANNED_SCALAR.replace("v_add_u32_e32 v2, s8, v1", "v_add_u32_e32 v3, s8, v1"))
    assert isa_compare.classify(a, v)[0] == "differs"
    # one instruction more, scalar or not
    longer = canned(CANNED_SCALAR.replace("\ts_endpgm", "\ts_nop 0                                                    // 000000002A3C: BF800000\n\ts_endpgm"))
    assert isa_compare.classify(a, longer)[0] == "differs"
    # other metadata
    assert isa_compare.classify(a, (dict(META, sgpr_count=2), a[1]))[0] == "differs"
