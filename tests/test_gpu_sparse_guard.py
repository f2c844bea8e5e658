"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the entry points of
include/ext/amdkge_sparse.h are handed: no write outside a buffer, no result that depends on bytes outside one.  amdkge_step_rows gets
exactly amdkge_step_rows_workspace_bytes of workspace, 16 bytes behind a 256-byte boundary, and a row buffer of exactly the cap it asks
for; amdkge_opt_step_rows gets a list whose count is smaller than its cap, and tables whose first and last row are listed."""
import ctypes as C

import numpy as np
import pytest

import sparse_ref as SR
from abi_decl import declared_names
from test_gpu_guard_bands import F32, F64, I32, I64, P, edge_triples, run_case, same_bits

pytestmark = pytest.mark.gpu

EXEMPT = {"amdkge_step_rows_workspace_bytes": "size function: every step_rows case allocates exactly what it returns"}


def case_step_rows(ar, B, n_ids, N):
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    rng = np.random.default_rng(B + n_ids)
    X = edge_triples(3, B, N, 4) if B else np.zeros((0, 3), I32)
    ids = rng.integers(0, N, n_ids).astype(I32)
    if n_ids > 1:
        ids[0], ids[-1] = 0, N - 1
    cap = min(2 * B + n_ids, N)
    tri, idt = ar.put("triples", X), ar.put("ids", ids)
    rows, cnt = ar.out("rows", (cap,), I32, -7), ar.out("n_rows", (1,), I64, -7)
    work = ar.work("work", lib.amdkge_step_rows_workspace_bytes(N, 2 * B + n_ids))
    _ffi.check(lib.amdkge_step_rows(N, P(tri), B, P(idt), n_ids, P(rows), cap, P(cnt), P(work), None))
    want = SR.candidate_rows(X, ids)

    def oracle(o):
        n = int(o["n_rows"][0])
        assert n == want.size and np.array_equal(o["rows"][:n], want) and (o["rows"][n:] == -7).all()

    ar.expects.append(oracle)


def case_opt_step_rows(ar, kind, rf, rows, lam):
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    rng = np.random.default_rng(rows + rf)
    x0 = (rng.normal(size=(rows, rf)) * 0.5).astype(F32)
    g0 = (rng.normal(size=(rows, rf)) * (rng.random(size=(rows, 1)) < 0.7)).astype(F32)
    g0[0], g0[-1] = 1.0, 1.0
    listed = np.unique(np.concatenate([[0, rows - 1], rng.choice(rows, rows // 2, replace=False)])).astype(I32)
    cap = listed.size + 5
    lst = np.concatenate([listed, np.full(5, rows - 1, I32)])           # behind the count: never read (a second wave on the last row would show)
    d = _ffi.Opt(_ffi.OPTIMIZERS[kind], 2, 1e-2, 0.9, 0.999, 1e-7, lam, 1, 0, rf)
    x, g = ar.put("x", x0, "out"), ar.put("grad", g0, "out")
    n_slots = len(_ffi.OPT_SLOTS[kind])
    s0 = ar.put("slot0", (rng.random(size=(rows, rf)) * 0.01 + 0.01).astype(F32), "out") if n_slots >= 1 else None
    s1 = ar.put("slot1", (rng.random(size=(rows, rf)) * 0.01).astype(F32), "out") if n_slots == 2 else None
    rw, cnt = ar.put("rows", lst), ar.put("n_rows", np.array([listed.size], I64))
    reg = ar.out("reg", (1,), F64, 0.0)
    _ffi.check(lib.amdkge_opt_step_rows(C.byref(d), P(x), P(g), P(s0), P(s1), rows, P(rw), P(cnt), cap, P(reg), None))
    ar.loose.add("reg")
    is_listed = np.zeros(rows, bool)
    is_listed[listed] = True
    touched = is_listed & (g0 != 0).any(1)
    want = lam * float((x0[touched].astype(F64) ** 2).sum())

    def oracle(o):
        assert abs(float(o["reg"][0]) - want) <= 1e-5 * want
        assert not o["grad"][is_listed].any() and same_bits(o["grad"][~is_listed], g0[~is_listed])
        assert same_bits(o["x"][~touched], x0[~touched]) and not (o["x"][touched] == x0[touched]).all(1).any()

    ar.expects.append(oracle)


SPARSE_CASES = {
    "amdkge_step_rows": [(case_step_rows, dict(B=37, n_ids=64, N=130)), (case_step_rows, dict(B=1, n_ids=0, N=130)),
                         (case_step_rows, dict(B=0, n_ids=1, N=130)), (case_step_rows, dict(B=300, n_ids=257, N=97)),
                         (case_step_rows, dict(B=1000, n_ids=2097, N=100000))],
    "amdkge_opt_step_rows": [(case_opt_step_rows, dict(kind="adam", rf=12, rows=123, lam=1e-3)),
                             (case_opt_step_rows, dict(kind="sgd", rf=4, rows=7, lam=0.0)),
                             (case_opt_step_rows, dict(kind="adagrad", rf=260, rows=50, lam=1e-3)),
                             (case_opt_step_rows, dict(kind="adamax", rf=2000, rows=33, lam=1e-3))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values()))
                                   for cases in SPARSE_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bitwise the same in all three"""
    run_case(fn, kw)


def test_every_declared_name_has_a_case():
    declared = declared_names("ext/amdkge_sparse.h")
    assert len(declared) == 3 and declared == set(SPARSE_CASES) | set(EXEMPT) and all(SPARSE_CASES.values()) and not set(SPARSE_CASES) & set(EXEMPT)
