# coding=utf-8
"""include/tfgx_normgrad.h (the backward of the GCN normalisation) without a GPU: the header compiles as C and as C++, every
declared symbol is exported and bound by its own ctypes table with the declared argument types (tfgx.h and its version
untouched), the version function returns what _lib binds, and the entry refuses null pointers, a bad mode, negative sizes and
an unweighted list on the host, before any device work."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tfgx_normgrad.h")
ENTRY = "tfgx_gcn_norm_backward_f32"

CTYPE_OF = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
            "float": ctypes.c_float, "tfgx_stream_t": ctypes.c_void_p}


def _declarations():
    """name -> (return ctype, [argument ctypes]) parsed from the header (every pointer is a void pointer in _lib.py)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(tfgx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for a in [a.strip() for a in args.split(",") if a.strip() and a.strip() != "void"]:
            types.append(ctypes.c_void_p if "*" in a else CTYPE_OF[a.replace("const", "").split()[0]])
        out[name] = (CTYPE_OF[ret], types)
    return out


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


@pytest.mark.parametrize("compiler, lang", [("gcc", "c"), ("g++", "c++")])
def test_header_compiles_as_c_and_cxx(compiler, lang, tmp_path):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cc"))
    src.write_text('#include "tfgx_normgrad.h"\nint main(void) { return TFGX_NORMGRAD_ABI_VERSION == 1 && TFGX_NORMGRAD_ALL == '
                   '(TFGX_NORMGRAD_ROW_PASS | TFGX_NORMGRAD_COL_PASS | TFGX_NORMGRAD_EDGE_PASS) ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_symbols_versions_and_signatures():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    decl = _declarations()
    assert sorted(decl) == [ENTRY, "tfgx_normgrad_version"]
    assert set(decl) == set(L.NORMGRAD_SIGNATURES)
    for name, (res, args) in decl.items():
        assert hasattr(lib, name), "libtfgx.so does not export {}".format(name)
        bound_res, bound_args = L.NORMGRAD_SIGNATURES[name]
        assert bound_res is res, name
        assert list(bound_args) == args, "{}: _lib.py binds {} but the header declares {}".format(name, bound_args, args)
        assert getattr(lib, name).argtypes == bound_args
    assert lib.tfgx_normgrad_version() == L.NORMGRAD_ABI_VERSION == int(
        re.search(r"#define\s+TFGX_NORMGRAD_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert (L.NORMGRAD_ROW_PASS, L.NORMGRAD_COL_PASS, L.NORMGRAD_EDGE_PASS, L.NORMGRAD_ALL) == tuple(
        int(re.search(r"#define\s+TFGX_NORMGRAD_" + n + r"\s+(\d+)", open(HEADER).read()).group(1))
        for n in ("ROW_PASS", "COL_PASS", "EDGE_PASS", "ALL"))
    assert lib.tfgx_version() == L.ABI_VERSION == 114                                               # did not move
    assert re.search(r"#define\s+TFGX_ABI_VERSION\s+114\b", open(os.path.join(ROOT, "include", "tfgx.h")).read())


def test_nothing_undeclared_is_exported():
    """Every tfgx_normgrad* / tfgx_gcn_norm_backward* symbol of the library is declared in the header."""
    from tf_geometric_amd import _lib as L
    L.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r"\bT tfgx_(normgrad|gcn_norm_backward)", line)}
    assert exported == set(_declarations())


# non-null pointers are never dereferenced: every refusal happens on the host
OK = dict(row_ptr=8, col=8, w=8, n_rows=5, n_cols=5, t_row_ptr=8, t2d=8, row_deg=8, col_deg=None, mode=0, fill=1.0,
          add_self_loop=1, renorm=1, G=8, S=8, A=8, B=8, t=8, dw=8, passes=7, stream=None)


def _refused(change, word):
    lib = _lib()
    rc = getattr(lib, ENTRY)(*dict(OK, **change).values())
    assert rc == 1, rc
    msg = lib.tfgx_last_error().decode()
    assert word in msg and ENTRY in msg, msg


@pytest.mark.parametrize("change, word", [
    (dict(n_rows=-1), "negative"), (dict(n_cols=-1), "negative"),
    (dict(mode=3), "bad norm mode"), (dict(mode=-1), "bad norm mode"),
    (dict(w=None), "w is null"), (dict(passes=0), "passes"), (dict(passes=8), "passes"), (dict(passes=-1), "passes"),
    (dict(row_ptr=None), "null pointer"), (dict(col=None), "null pointer"), (dict(row_deg=None), "null pointer"),
    (dict(G=None), "null pointer"), (dict(dw=None), "null pointer"), (dict(A=None), "null pointer (A)"),
    (dict(t_row_ptr=None), "t_row_ptr"), (dict(t2d=None), "t_row_ptr"), (dict(B=None), "t_row_ptr"), (dict(t=None), "t_row_ptr"),
    (dict(mode=1, A=None), "null pointer (A)"), (dict(mode=2, t=None), "t_row_ptr"),
    (dict(n_cols=7), "add_self_loop"), (dict(n_cols=7, add_self_loop=0), "symmetric"),
    (dict(mode=2, n_cols=7, add_self_loop=0), "n_cols <= n_rows"),
])
def test_argument_checks_happen_on_the_host(change, word):
    _refused(change, word)


def test_zero_rows_succeed_without_device_work_but_not_without_weights():
    lib = _lib()
    null = dict(row_ptr=None, col=None, t_row_ptr=None, t2d=None, row_deg=None, G=None, S=None, A=None, B=None, t=None, dw=None)
    assert getattr(lib, ENTRY)(*dict(OK, **dict(null, n_rows=0, n_cols=0)).values()) == 0
    _refused(dict(null, n_rows=0, n_cols=0, w=None), "w is null")


def test_gcn_norm_adj_fails_loudly_without_a_gpu():
    import numpy as np
    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd import autograd
    from tf_geometric_amd._lib import TfgxError
    assert callable(autograd.gcn_norm) and callable(autograd.gcn_norm_backward)
    if torch.cuda.is_available():
        return
    w = torch.ones(2, requires_grad=True)
    with pytest.raises(TfgxError):
        tfg.nn.gcn_norm_edge(np.array([[0, 1], [1, 0]], np.int32), 2, w)
