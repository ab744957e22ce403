# coding=utf-8
"""The one copy of the C-ABI test scaffolding: a parser of the headers under include/, the rule that says which ctypes binding a
declared parameter accepts, and the gcc / nm / refusal helpers the per-header test files share (no GPU needed)."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}


def source(header):
    """A header's text without comments: `header` is a file name under include/, or C text itself (anything with a newline)."""
    text = header if "\n" in header else open(os.path.join(INCLUDE, header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _ctype_of(text, named):
    """("val" | "ptr", base type) of a return type or of one parameter (whose last word is then its name); const is dropped."""
    words = [w for w in re.findall(r"\w+|\*", text) if w not in ("const", "struct")]
    if named and len(words) > 1 and words[-1] != "*":
        words.pop()
    assert words and words[0] != "*" and len([w for w in words if w != "*"]) == 1, "cannot read the type of {!r}".format(text)
    depth = words.count("*")
    return ("ptr" if depth else "val"), (words[0] if depth < 2 else "void")


def declarations(header):
    """name -> (return type, [parameter types]) of every tfgx_* function a header declares, each type as _ctype_of gives it."""
    src = re.sub(r"^[ \t]*#.*$", "", source(header).replace("\\\n", " "), flags=re.M)      # preprocessor lines
    src = re.sub(r"\{[^{}]*\}", "", re.sub(r'extern\s+"C"\s*\{', "", src))                  # struct and enum bodies
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(tfgx_\w+)\s*\(([^()]*)\)\s*;", src):
        assert name not in out, "{} is declared twice".format(name)
        out[name] = (_ctype_of(ret, False), [_ctype_of(p, True) for p in params.split(",") if p.strip() != "void"])
    return out


def accepts(declared, bound, structs):
    """THE RULE.  A value is bound as exactly its ctypes scalar (tfgx_stream_t: c_void_p; a void return: None).  A pointer may be
    bound as c_void_p; as c_char_p only for char*; as POINTER(T) only where T is the ctypes type of the declared pointee or the
    class `structs` registers for the declared struct."""
    kind, base = declared
    if kind == "val":
        return bound is None if base == "void" else bound is (ctypes.c_void_p if base == "tfgx_stream_t" else SCALARS.get(base, 0))
    if bound is ctypes.c_void_p:
        return True
    if bound is ctypes.c_char_p:
        return base == "char"
    pointee = structs.get(base, SCALARS.get(base))
    return pointee is not None and bound is ctypes.POINTER(pointee)


def mismatches(declared, table, structs):
    """Every way a ctypes table {name: (restype, argtypes)} departs from declarations(): [] when the rule holds throughout."""
    bad = ["{}: only in the {}".format(n, "header" if n in declared else "table") for n in sorted(set(declared) ^ set(table))]
    for name in sorted(set(declared) & set(table)):
        (ret, params), (res, args) = declared[name], table[name]
        if not accepts(ret, res, structs):
            bad.append("{}: returns {} but is bound as {}".format(name, ret, res))
        if len(params) != len(args):
            bad.append("{}: {} parameters declared, {} bound".format(name, len(params), len(args)))
            continue
        bad += ["{}: argument {} is {} but is bound as {}".format(name, i, p, a)
                for i, (p, a) in enumerate(zip(params, args)) if not accepts(p, a, structs)]
    return bad


def macro(header, name):
    """The value of an integer #define (decimal or hex, parenthesised or not); None when the header does not define it."""
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))\)?[ \t]*$" % name, source(header), flags=re.M)
    return int(m.group(1), 0) if m else None


def struct_layout(header, c_struct, cls, tmp_path):
    """The ctypes class has the header struct's members, in order, at gcc's offsetof, and its sizeof."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_struct, c_struct), source(header), flags=re.S).group(1)
    fields = [f for f, _ in cls._fields_]
    assert re.findall(r"(\w+)\s*[,;]", body) == fields, c_struct
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "{}"'.format(header), 'int main(void){',
             'printf("%zu\\n", sizeof({}));'.format(c_struct)]
    lines += ['printf("%zu\\n", offsetof({}, {}));'.format(c_struct, f) for f in fields] + ['return 0;}']
    src, exe = tmp_path / (c_struct + ".c"), tmp_path / c_struct
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == ctypes.sizeof(cls), (c_struct, vals[0], ctypes.sizeof(cls))
    for f, off in zip(fields, vals[1:]):
        assert getattr(cls, f).offset == off, (c_struct, f)


def compiles_as_c_and_cxx(header, tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cc")):
        src = tmp_path / "{}.{}".format(header, ext)
        src.write_text('#include "{}"\nint main(void) {{ return 0; }}\n'.format(header))
        subprocess.check_call([compiler, "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def exported_symbols():
    """The tfgx_* text symbols of the loaded library."""
    from tf_geometric_amd import _lib as L
    L.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    return {line.split()[-1] for line in out.splitlines() if re.search(r" T tfgx_\w+$", line)}


def refused(fn, ok, change, word, code=1):
    """Call lib.<fn> with the keyword table `ok` (in the declaration's order) and one change: it returns `code` (1 =
    TFGX_ERR_INVALID_ARG) on the host, before any device work, and tfgx_last_error() names `word` and the function."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    rc = getattr(lib, fn)(*dict(ok, **change).values())
    assert rc == code, (fn, change, rc)
    msg = lib.tfgx_last_error().decode()
    assert word in msg and fn in msg, msg
