"""The C ABI as ctypes, read from the headers that define it: those _lib.HEADERS names, and include/musehip_dbg.h.

`load(name)` gives the header's enumerators (name -> int), its structs (name -> ctypes.Structure class) and its prototypes
(name -> (restype, argtypes)).  The reader knows the C these headers are written in and nothing more: a declaration it does not
recognise raises AbiError naming it - nothing is guessed and nothing is skipped.  tests/test_abi_cpu.py checks the result against
the compiler.
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
POINTEE_ONLY = {"void", "char", "uint8_t", "double"}     # legal behind a `*`, never by value (double: device float64 buffers)
# A struct field that points to a known struct is POINTER(struct): a host descriptor the caller links with ctypes.pointer().  The C cannot
# say that such a pointer is for DEVICE memory, where the caller stores an address instead; those fields are named here and are c_void_p.
DEVICE_STRUCT_FIELDS = {("mh_step_update", "coef")}

_IDENT = r"[A-Za-z_]\w*"
_TYPEDEF_VOIDP = re.compile(r"typedef void\s*\*\s*(%s)$" % _IDENT)
_ENUM = re.compile(r"enum (%s) ?\{(.*)\}$" % _IDENT)
_ENUMERATOR = re.compile(r"(%s) ?= ?(-?\d+)$" % _IDENT)
_STRUCT = re.compile(r"typedef struct (%s) ?\{(.*)\} ?(%s)$" % (_IDENT, _IDENT))
_FIELD = re.compile(r"(?:const )?(%s)\b(.*)$" % _IDENT)
_DECLARATOR = re.compile(r"(\*+)? ?(%s) ?(?:\[ ?(\d+) ?\])?$" % _IDENT)
_PROTO = re.compile(r"(?:const )?(%s)(?: ?(\*+) ?| )(%s) ?\(([^()]*)\)$" % (_IDENT, _IDENT))
_PARAM = re.compile(r"(?:const )?(%s)(?: ?(\*+) ?| )(%s)$" % (_IDENT, _IDENT))


class AbiError(ValueError):
    pass


def _declarations(text):
    """The header's top-level declarations, one string each, white space squeezed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            out.append(" ".join(text[start:i].split()))
            start = i + 1
    if depth != 0 or text[start:].strip():
        raise AbiError("unterminated declaration: %r" % " ".join(text[start:].split())[:120])
    return out


def load(name, base=None):
    with open(os.path.join(INCLUDE_DIR, name)) as f:
        return parse(f.read(), base)


def parse(text, base=None):
    """Parse one header.  `base`: the result for a header this one includes (its types are known here)."""
    h = SimpleNamespace(enums={}, structs={}, protos={})
    structs = dict(base.structs) if base else {}
    handles = set(base.handles) if base else set()     # typedef void* NAME
    h.handles = handles

    def value_type(t, where):
        if t in SCALARS:
            return SCALARS[t]
        if t in handles:
            return C.c_void_p
        raise AbiError("%s: %s %r" % (where, "struct passed by value:" if t in structs else "unknown type", t))

    def check_pointee(t, where):
        if not (t in SCALARS or t in POINTEE_ONLY or t in handles or t in structs):
            raise AbiError("%s: pointer to unknown type %r" % (where, t))

    def call_type(t, stars, where):
        """return type or parameter"""
        if not stars:
            return value_type(t, where)
        check_pointee(t, where)
        return C.c_char_p if (t, stars) == ("char", "*") else C.c_void_p

    for decl in _declarations(text):
        m = _TYPEDEF_VOIDP.match(decl)
        if m:
            handles.add(m.group(1))
            continue
        m = _ENUM.match(decl)
        if m:
            for item in filter(None, (s.strip() for s in m.group(2).split(","))):
                e = _ENUMERATOR.match(item)
                if not e or e.group(1) in h.enums:
                    raise AbiError("enum %s: cannot read enumerator %r" % (m.group(1), item))
                h.enums[e.group(1)] = int(e.group(2))
            continue
        m = _STRUCT.match(decl)
        if m:
            sname = m.group(1)
            if m.group(3) != sname or sname in structs:
                raise AbiError("struct %s: tag and typedef name differ, or declared twice" % sname)
            fields = []
            for fdecl in filter(None, (s.strip() for s in m.group(2).split(";"))):
                where = "struct %s, field %r" % (sname, fdecl)
                f = _FIELD.match(fdecl)
                if not f:
                    raise AbiError("%s: cannot read" % where)
                t = f.group(1)
                for d in f.group(2).split(","):
                    dm = _DECLARATOR.match(d.strip())
                    if not dm:
                        raise AbiError("%s: cannot read declarator %r" % (where, d.strip()))
                    stars, fname, count = dm.groups()
                    if stars:
                        check_pointee(t, where)
                        host_struct = stars == "*" and t in structs and (sname, fname) not in DEVICE_STRUCT_FIELDS
                        ct = C.POINTER(structs[t]) if host_struct else C.c_void_p
                    else:
                        ct = structs[t] if t in structs else value_type(t, where)
                    fields.append((fname, ct * int(count) if count else ct))
            if len({n for n, _ in fields}) != len(fields):
                raise AbiError("struct %s: a field name repeats" % sname)
            structs[sname] = h.structs[sname] = type(sname, (C.Structure,), {"_fields_": fields, "__doc__": sname})
            continue
        m = _PROTO.match(decl)
        if m:
            rtype, rstars, fname, params = m.groups()
            where = "prototype %s" % fname
            if fname in h.protos or (base and fname in base.protos):
                raise AbiError("%s: declared twice" % where)
            args = []
            if params.strip() != "void":
                for p in params.split(","):
                    pm = _PARAM.match(p.strip())
                    if not pm:
                        raise AbiError("%s: cannot read parameter %r" % (where, p.strip()))
                    args.append(call_type(pm.group(1), pm.group(2), "%s, parameter %r" % (where, p.strip())))
            h.protos[fname] = (call_type(rtype, rstars, where + ", return type"), args)
            continue
        raise AbiError("cannot read declaration %r" % decl[:160])
    return h
