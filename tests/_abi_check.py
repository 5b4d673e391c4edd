"""What the ABI tests share, each stated once and driven by _abi.HEADERS (header -> its prototype table and its struct mirrors): the library fixture, the header parser,
the rule that says as which ctypes object a C type is bound, the comparator of a header's declarations with a prototype table, and the C compiler's layout of a struct."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from mpc_local_planner_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
MAIN = "mpc_hip.h"                                  # the header every other one includes; _abi.PROTOTYPES / _lib.EXPORTS mirror it alone
SIDE = [h for h in _abi.HEADERS if h != MAIN]


@pytest.fixture(scope="module")
def lib():
    """the C-ABI library: built if stale (where there is a compiler), loaded, every table of _abi.HEADERS bound"""
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    return _lib.load()


def header_text(header):
    return open(os.path.join(INCLUDE, header)).read()


def header_code(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def declarations(text):
    """{name: (return type, [(parameter type, parameter name), ...])} of every `ret name(params);` of the header, types without const"""
    def ctype(words):
        return " ".join(w for w in words if w != "const").replace(" *", "*")
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(mpc_\w+)\s*\(([^)]*)\)\s*;", header_code(text)):
        params = [p.replace("*", " * ").split() for p in params.split(",")]
        out[name] = (ctype(ret.replace("*", " * ").split()), [] if params == [["void"]] else [(ctype(p[:-1]), p[-1]) for p in params])
    return out


# where the binding deviates from the rule of bound() (found by the comparator when a table or a header changes)
VOID_STRUCTS = ("mpc_obstacles",)                                            # const mpc_obstacles* is bound as c_void_p everywhere: callers pass byref() or NULL
EXCEPTIONS = {("mpc_set_parameter_sets", "sets"): C.c_void_p,                # an array of mpc_config, passed as a cast address
              ("mpc_occupancy", "workgroups_per_cu"): C.POINTER(C.c_int32)}  # the one int32_t* that is a byref() scalar and not an array


def bound(header, function, ctype, name=None):
    """THE ctypes object a return value (name None) or a parameter of this C type is bound as: exactly one.  A struct pointer is a pointer to the mirror when the
    struct is the header's own or mpc_hip.h's."""
    if (function, name) in EXCEPTIONS:
        return EXCEPTIONS[function, name]
    if ctype in ("double", "int32_t", "int"):
        return C.c_double if ctype == "double" else C.c_int32      # (c_int32 is c_int here: one object)
    if name is None:
        return {"void": None, "char*": C.c_char_p}[ctype]
    assert ctype.endswith("*"), ctype
    base, mirrors = ctype[:-1], {**_abi.HEADERS[MAIN][1], **_abi.HEADERS[header][1]}
    if base in mirrors and base not in VOID_STRUCTS:
        return C.POINTER(mirrors[base])
    return {"mpc_solver*": C.POINTER(C.c_void_p), "float": C.POINTER(C.c_float), "int64_t": C.POINTER(C.c_int64)}.get(base, C.c_void_p)


def mismatches(header, table):
    """what differs between the header's declarations and a prototype table: a function of the two (and of the mirrors _abi.HEADERS gives the header)"""
    decl = declarations(header_text(header))
    bad = [f"{n}: declared, not in the table" for n in sorted(set(decl) - set(table))] + [f"{n}: in the table, not declared" for n in sorted(set(table) - set(decl))]
    for name in sorted(set(decl) & set(table)):
        (ret, params), (restype, argtypes) = decl[name], table[name]
        if restype is not bound(header, name, ret):
            bad.append(f"{name}: returns {ret}, bound as {restype}")
        if len(params) != len(argtypes):
            bad.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} bound")
            continue
        bad += [f"{name}: parameter {i} is {t} {p}, bound as {a}" for i, ((t, p), a) in enumerate(zip(params, argtypes)) if a is not bound(header, name, t, p)]
    return bad


def struct_fields(header, struct):
    """the field names of `typedef struct <struct> {...} <struct>;` in header order; `double Q[3], R[2]` -> Q, R"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header_code(header_text(header)), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]


def c_layout(header, struct, fields, enumerators, tmp_path):
    """[sizeof(struct), offsetof(struct, f) for every field, the value of every enumerator] as gcc has them, the header compiled as C"""
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){\nprintf("%%zu\\n", sizeof(%s));\n' % (header, struct) +
                   "".join('printf("%%zu\\n", offsetof(%s,%s));\n' % (struct, f) for f in fields) + "".join('printf("%%d\\n", %s);\n' % e for e in enumerators) + 'return 0;}\n')
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
