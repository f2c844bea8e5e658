"""ampligraph_amd/_ffi.py's second table, ABI_EXT, against the headers under include/ext/, without a GPU, by the rules
tests/test_abi_host.py holds ABI to the headers directly under include/ with (tests/abi_decl.py has them): every entry point's name,
return type and argument list (count, order, types) as the header declares them and as lib() bound them."""
import os

import pytest

import abi_decl as D
from ampligraph_amd import _ffi

EXT_HEADERS = sorted("ext/" + f for f in os.listdir(os.path.join(D.INCLUDE, "ext")) if f.endswith(".h"))


def test_the_table_names_every_extension_header_and_every_name_once():
    assert set(_ffi.ABI_EXT) == set(EXT_HEADERS) and "ext/amdkge_sparse.h" in _ffi.ABI_EXT
    names = [n for table in _ffi.ABI_EXT.values() for n in table]
    assert len(names) == len(set(names)) and set(_ffi.ABI_EXT["ext/amdkge_sparse.h"]) == {
        "amdkge_step_rows_workspace_bytes", "amdkge_step_rows", "amdkge_opt_step_rows"}
    # nothing is in both tables, and no header directly under include/ knows the extension
    assert not set(names) & {n for table in _ffi.ABI.values() for n in table}
    assert not [h for h in D.HEADERS if "amdkge_sparse" in D.text(h) or "step_rows" in D.text(h)]


@pytest.mark.parametrize("header", list(_ffi.ABI_EXT))
def test_names_and_types_are_the_headers(header):
    table, decls = _ffi.ABI_EXT[header], D.declarations(header)
    assert D.declared_names(header) == set(decls) == set(table), D.declared_names(header) ^ set(table)
    for name, (res, params) in decls.items():
        want_res, want_args = table[name]
        assert D.matches(res, want_res, _ffi), f"{name}: returns {res}, the table says {want_res}"
        assert len(params) == len(want_args), f"{name}: {len(params)} parameters declared, {len(want_args)} in the table"
        for i, ((c_type, pname), ct) in enumerate(zip(params, want_args)):
            assert D.matches(c_type, ct, _ffi), f"{name}: parameter {i} is `{c_type} {pname}`, the table says {ct.__name__}"
        fn = getattr(_ffi.lib(), name)
        assert fn.restype is want_res and list(fn.argtypes) == list(want_args), name


def test_the_header_compiles_as_c_on_its_own(tmp_path):
    import subprocess

    src = tmp_path / "probe.c"
    src.write_text('#include "ext/amdkge_sparse.h"\nint main(void) { return amdkge_step_rows_workspace_bytes(1, 0) < 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", D.INCLUDE, "-c", str(src), "-o", str(tmp_path / "probe.o")], check=True)


# the argument errors of the three entry points, returned before any device work (the pointers that are set are never dereferenced)
def test_argument_errors_without_a_device():
    import ctypes as C

    lib, X = _ffi.lib(), C.c_void_p(4096)
    ws = lib.amdkge_step_rows_workspace_bytes
    assert ws(0, 5) == -1 and ws(1 << 31, 5) == -1 and ws(10, -1) == -1 and ws(10, 1 << 31) == -1 and ws(10, 0) > 0
    sr = lib.amdkge_step_rows
    for args, word in (((0, X, 2, X, 3, X, 7, X, X, None), "bad sizes"), ((10, X, -1, X, 3, X, 7, X, X, None), "bad sizes"),
                       ((10, X, 2, X, -3, X, 7, X, X, None), "bad sizes"), ((10, X, 2, X, 3, X, 6, X, X, None), "cap"),
                       ((5, X, 2, X, 3, X, 4, X, X, None), "cap"), ((10, X, 2, X, 3, None, 7, X, X, None), "NULL"),
                       ((10, X, 2, X, 3, X, 7, None, X, None), "NULL"), ((10, X, 2, X, 3, X, 7, X, None, None), "NULL"),
                       ((10, None, 2, X, 3, X, 7, X, X, None), "NULL"), ((10, X, 2, None, 3, X, 7, X, X, None), "NULL")):
        assert sr(*args) == _ffi.EINVAL and word in lib.amdkge_last_error().decode(), args
    opt = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1, 0, 8)
    osr = lib.amdkge_opt_step_rows
    good = dict(x=X, g=X, s0=X, s1=X, n=10, rows=X, cnt=X, cap=4)
    call = lambda o=opt, **kw: osr(*(lambda a: (C.byref(o) if o is not None else None, a["x"], a["g"], a["s0"], a["s1"], a["n"], a["rows"], a["cnt"], a["cap"], None, None))(dict(good, **kw)))  # noqa: E731
    for kw, word in ((dict(x=None), "NULL"), (dict(g=None), "NULL"), (dict(s0=None), "slot 0"), (dict(s1=None), "slot 1"), (dict(n=-1), ">= 0"),
                     (dict(cap=-1), ">= 0"), (dict(rows=None), "NULL"), (dict(cnt=None), "NULL"), (dict(x=C.c_void_p(4100)), "aligned")):
        assert call(**kw) == _ffi.EINVAL and word in lib.amdkge_last_error().decode(), kw
    for rf in (0, 2, 6, -4):
        bad = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1, 0, rf)
        assert call(bad) == _ffi.EINVAL and "row_floats" in lib.amdkge_last_error().decode()
    assert call(None) == _ffi.EINVAL
    assert call(cap=0, rows=None, cnt=None) == _ffi.OK and call(n=0) == _ffi.OK     # nothing to do
    sgd = _ffi.Opt(_ffi.OPTIMIZERS["sgd"], 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1, 0, 8)
    assert call(sgd, s0=None, s1=None, cap=0) == _ffi.OK                            # SGD keeps no slots
