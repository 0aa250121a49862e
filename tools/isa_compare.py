#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 machine code of two builds (CPU only; the method of profiles/*_isa_and_bench.txt).

    python tools/isa_compare.py <dir A> <dir B>

Every *.o / *.dbg.o of the two directories that carries an offload bundle is taken apart: `llvm-objdump --offloading` extracts the
gfx950 code object, `llvm-readelf --notes` gives each kernel's .amdhsa metadata (vgpr / sgpr counts, both spill counts,
group_segment_fixed_size, private_segment_fixed_size, max_flat_workgroup_size) and `llvm-objdump -d` its text, from which addresses,
encodings, branch displacements and the pc-relative literal behind s_getpc_b64 are removed.  Names are demangled.  Kernels are matched by
(object, name), and per kernel one line says
    identical    metadata and text equal
    scalar-only  metadata equal, the same number of instructions, and the sequence of all instructions that do not begin with s_ equal
                 once scalar register numbers are masked: the scalar instructions differ in order and registers only
    differs      anything else
followed by the kernel-set differences and the totals.  Exit status 1 on any `differs` or kernel-set difference.
The tool compares two builds with each other; it does not look for particular instructions."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

META_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
             "private_segment_fixed_size", "max_flat_workgroup_size")


def llvm_tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    path = shutil.which(name)
    if not path:
        raise SystemExit("isa_compare: %s not found (looked under $ROCM_PATH/llvm/bin and on PATH)" % name)
    return path


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True).stdout


def demangle(co, names):
    """{mangled: demangled} by llvm-objdump's own demangler (it knows __bf16 and _Float16; a binutils c++filt may not): the symbol
    table printed twice, with and without -C, line by line.  A name that does not come out unique stays mangled."""
    sym = re.compile(r"^[0-9a-f]+ .{7} \S+\t[0-9a-f]+ (?:\.\w+ )?(.*)$")
    raw = [m.group(1) for m in map(sym.match, run(llvm_tool("llvm-objdump"), "-t", co).splitlines()) if m]
    nice = [m.group(1) for m in map(sym.match, run(llvm_tool("llvm-objdump"), "-t", "-C", co).splitlines()) if m]
    table = dict(zip(raw, nice)) if len(raw) == len(nice) else {}
    out = {n: table.get(n, n) for n in names}
    return out if len(set(out.values())) == len(out) else {n: n for n in names}


def extract_code_object(obj):
    """the gfx950 code object inside a host object, as a path in a temporary directory (None: the object carries no device code)"""
    tmp = tempfile.mkdtemp(prefix="isa_compare_")
    local = os.path.join(tmp, "obj.o")
    shutil.copy(obj, local)   # (the bundles are written next to the input)
    run(llvm_tool("llvm-objdump"), "--offloading", "obj.o", cwd=tmp)
    found = [f for f in os.listdir(tmp) if "amdgcn" in f and f.endswith("gfx950")]
    return (tmp, os.path.join(tmp, found[0])) if found else (tmp, None)


def parse_metadata(notes):
    """{mangled kernel name: {key: value}} from the YAML that llvm-readelf --notes prints"""
    kernels, cur, inside = {}, None, False
    for line in notes.splitlines():
        if not line.startswith(" "):
            inside = line.startswith("amdhsa.kernels:")
            continue
        m = re.match(r"^  (- |  )\.(\w+):\s*(\S*)\s*$", line)   # an entry's own keys: its .args entries sit deeper
        if not inside or not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if m.group(2) == "name":
            kernels[m.group(3)] = cur
        elif m.group(2) in META_KEYS:
            cur[m.group(2)] = int(m.group(3))
    return kernels


BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch|s_call_b64.*,)\s+-?\d+$")


def normalise(disasm):
    """{mangled symbol: [instruction, ...]} from llvm-objdump -d: no addresses, encodings, branch displacements or pc-relative literals"""
    funcs, cur, after_getpc = {}, None, 0
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = " ".join(line.split("//")[0].split())
        if not ins:
            continue
        if BRANCH.match(ins):
            ins = ins.rsplit(" ", 1)[0] + " <disp>"
        if after_getpc and re.match(r"s_addc?_u32 ", ins):   # s_getpc_b64 + s_add_u32 lo + s_addc_u32 hi: the distance to a symbol
            ins = ins.rsplit(" ", 1)[0] + " <pcrel>"
            after_getpc -= 1
        else:
            after_getpc = 2 if ins.startswith("s_getpc_b64") else 0
        cur.append(ins)
    for text in funcs.values():   # the padding up to the next symbol's alignment is not the function's text
        while text and text[-1] in ("s_nop 0", "s_code_end"):
            text.pop()
    return funcs


def load_object(obj):
    """{demangled kernel name: (metadata, [instructions])} of one object"""
    tmp, co = extract_code_object(obj)
    try:
        if co is None:
            return {}
        meta = parse_metadata(run(llvm_tool("llvm-readelf"), "--notes", co))
        text = normalise(run(llvm_tool("llvm-objdump"), "-d", co))
        names = demangle(co, meta)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {names[k]: (meta[k], text.get(k, [])) for k in meta}


SREG = re.compile(r"\b(s|ttmp)(\d+|\[\d+:\d+\])")


def vector_sequence(text):
    return [SREG.sub(r"\1#", ins) for ins in text if not ins.startswith("s_")]


def classify(a, b):
    """(class, detail) of one kernel given as (metadata, [instructions]) in the two builds"""
    (ma, ta), (mb, tb) = a, b
    if ma != mb:
        return "differs", "metadata " + ", ".join("%s %s -> %s" % (k, ma.get(k), mb.get(k)) for k in META_KEYS if ma.get(k) != mb.get(k))
    if ta == tb:
        return "identical", "%d instructions" % len(ta)
    if len(ta) != len(tb):
        return "differs", "%d -> %d instructions" % (len(ta), len(tb))
    if vector_sequence(ta) == vector_sequence(tb):
        return "scalar-only", "%d instructions, %d lines differ: scalar instructions and scalar register numbers" % (len(ta), sum(x != y for x, y in zip(ta, tb)))
    return "differs", "%d instructions, %d lines differ, non-scalar ones among them" % (len(ta), sum(x != y for x, y in zip(ta, tb)))


def objects(d):
    return sorted(f for f in os.listdir(d) if f.endswith(".o"))


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    da, db = argv[1], argv[2]
    oa, ob = objects(da), objects(db)
    totals = {"identical": 0, "scalar-only": 0, "differs": 0}
    set_diffs = ["object only in %s: %s" % (d, o) for d, o in [(da, o) for o in oa if o not in ob] + [(db, o) for o in ob if o not in oa]]
    for o in [o for o in oa if o in ob]:
        ka, kb = load_object(os.path.join(da, o)), load_object(os.path.join(db, o))
        for name in sorted(set(ka) | set(kb)):
            if name not in ka or name not in kb:
                set_diffs.append("kernel only in %s: %s: %s" % (db if name in kb else da, o, name))
                continue
            cls, detail = classify(ka[name], kb[name])
            totals[cls] += 1
            print("%-11s %s: %s  (%s)" % (cls, o, name, detail))
    for line in set_diffs:
        print(line)
    print("total: %d identical, %d scalar-only, %d differs; %d kernel-set differences" %
          (totals["identical"], totals["scalar-only"], totals["differs"], len(set_diffs)))
    return 1 if totals["differs"] or set_diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
