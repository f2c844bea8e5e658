"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer amdkge_batch_reg_fwdbwd
(include/amdkge_batch_reg.h) is handed: no write outside a buffer, no result that depends on bytes outside one -- also with the
tables and gradient tables 16 bytes behind a 256-byte boundary (the 16-byte path stays legal) and 4 bytes behind one (the call
falls back to one float per lane).  The batch touches the first and the last row of both tables."""
import ctypes as C

import numpy as np
import pytest

import batch_reg_ref as BR
from abi_decl import declared_names
from test_gpu_guard_bands import F32, F64, P, Tables, edge_triples, run_case

pytestmark = pytest.mark.gpu


def case_batch_reg(ar, model, k, pad, offset, p, B=37, N=130, R=4):
    from ampligraph_amd import _ffi

    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    ent, rel, tri = ar.put("ent", T.ent_s, offset=offset), ar.put("rel", T.rel_s, offset=offset), ar.put("triples", X)
    ge = ar.put("g_ent", np.zeros((N, T.Ks), F32), "out", offset=offset)
    gr = ar.put("g_rel", np.zeros((R, T.Ks), F32), "out", offset=offset)
    acc = ar.put("reg_sum", np.zeros(1, F64), "out")
    norm_e = BR.MODULUS if BR.modulus_allowed(model, "ent") else BR.FLOAT
    norm_r = BR.MODULUS if BR.modulus_allowed(model, "rel") else BR.FLOAT
    terms = (p, 0.05, norm_e, 5 - p, 0.125, norm_r)
    _ffi.check(_ffi.lib().amdkge_batch_reg_fwdbwd(C.byref(T.m), P(ent), P(rel), P(tri), B, *terms, P(ge), P(gr), P(acc), None))
    ar.loose |= {"g_ent", "g_rel", "reg_sum"}          # unordered atomics: held to the restatement instead of bitwise between the runs
    pad_mask = np.ones(T.Ks, bool)
    for h in range(T.nc):
        pad_mask[h * T.ks:h * T.ks + k] = False
    ar.keep("g_ent", np.tile(pad_mask, N))
    ar.keep("g_rel", np.tile(pad_mask, R))
    wR, wGe, wGr = BR.batch_reg(model, k, T.ent, T.rel, X, *terms)

    def oracle(o):
        assert abs(float(o["reg_sum"][0]) - wR) <= 1e-6 * wR
        BR.assert_rows_close(T.dense(o["g_ent"]), wGe, 1e-5)
        BR.assert_rows_close(T.dense(o["g_rel"]), wGr, 1e-5)

    ar.expects.append(oracle)


BATCH_REG_CASES = {
    "amdkge_batch_reg_fwdbwd": [(case_batch_reg, dict(model="ComplEx", k=50, pad=True, offset=0, p=3)),
                                (case_batch_reg, dict(model="ComplEx", k=50, pad=True, offset=16, p=3)),
                                (case_batch_reg, dict(model="HolE", k=200, pad=True, offset=4, p=2)),
                                (case_batch_reg, dict(model="DistMult", k=7, pad=False, offset=0, p=3)),
                                (case_batch_reg, dict(model="TransE", k=300, pad=False, offset=16, p=2)),
                                (case_batch_reg, dict(model="RotatE", k=33, pad=False, offset=4, p=3))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id="-".join(str(v) for v in kw.values())) for cases in BATCH_REG_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, padding floats kept, outputs within their bars"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_batch_reg.h")
    assert declared and declared == set(BATCH_REG_CASES) and all(BATCH_REG_CASES.values())
