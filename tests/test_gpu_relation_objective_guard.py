"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the entry points of
include/amdkge_relation_objective.h are handed: no write outside a buffer, no result that depends on bytes outside one, the workspace
handed over with exactly amdkge_train_relation_workspace_bytes bytes at an unaligned offset -- as tests/test_gpu_shared_mask_guard.py
does for the masked shared step.  The padded layout, NULL ranges and NULL optional outputs are cases of their own."""
import ctypes as C

import numpy as np
import pytest

import relation_objective_ref as RR
from abi_decl import declared_names
from test_gpu_guard_bands import F32, F64, P, Tables, assert_grads_close, edge_triples, loss_desc, run_case

pytestmark = pytest.mark.gpu

I64 = np.int64


def _lib():
    from ampligraph_amd import _ffi

    return _ffi, _ffi.lib()


def case_train_relation(ar, model, k, pad, ranges, outputs, B=37, N=33, R=35, weight=0.25):
    """the bars of test_gpu_shared_mask_guard.py's step case: scores bitwise between the runs, loss and gradients (fp32 / fp64 atomics)
    against the restatement.  R = 35 and B = 37 leave every tile partly filled."""
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    rng = np.random.default_rng(11)
    more = X[rng.integers(0, B, 3 * B)].copy()
    more[:, 1] = rng.integers(0, R, len(more))                            # more relations for the batch's own pairs
    known = RR.known_relations(X, [X, more]) if ranges else None
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    rg = [ar.put(n, a) for n, a in zip(("lo", "hi", "known"), RR.csr(known))] if ranges else [None, None, None]
    ge, gr = ar.out("g_ent", (N, T.Ks), F32, 0.0), ar.out("g_rel", (R, T.Ks), F32, 0.0)
    ls = ar.out("loss", (1,), F64, 0.0)
    ps = ar.out("pos_scores", (B,), F32, 7.0) if outputs else None
    ns = ar.out("rel_scores", (B * R,), F32, 7.0) if outputs else None
    stats = ar.out("stats", (2,), I64, 0) if outputs else None
    need = lib.amdkge_train_relation_workspace_bytes(C.byref(T.m), B)
    assert need > 0
    work = ar.work("work", need)
    _ffi.check(lib.amdkge_train_relation_fwdbwd(C.byref(T.m), C.byref(loss_desc("self_adversarial")), weight, P(ent), P(rel), P(tri), B, *(P(t) for t in rg),
                                                P(ge), P(gr), P(ls), P(ps), P(ns), P(work), P(stats), None))
    ar.loose |= {"g_ent", "g_rel", "loss"}
    mask, masked, unmaskable = RR.mask_matrix(B, R, known)
    assert masked > B or not ranges
    total, Te, Tr, sp, sn = RR.relation_step(model, T.ent, T.rel, X, mask, "self_adversarial", "sum", weight)
    live = np.isfinite(sn)
    padding = np.ones((T.nc, T.ks), dtype=bool)
    padding[:, :k] = False

    def oracle(o):
        if outputs:
            assert np.allclose(o["pos_scores"], sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
            assert np.array_equal(np.isneginf(o["rel_scores"]), ~live)
            assert np.allclose(o["rel_scores"][live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
            assert o["stats"].tolist() == [masked, unmaskable]
        assert abs(float(o["loss"][0]) - total) <= 2e-5 * max(1.0, abs(float(o["loss"][0])))
        assert_grads_close(T.dense(o["g_ent"]), Te)
        assert_grads_close(T.dense(o["g_rel"]), Tr)
        assert not o["g_ent"][:, padding.reshape(-1)].any() and not o["g_rel"][:, padding.reshape(-1)].any()   # padding floats: never written

    ar.expects.append(oracle)


def case_workspace_bytes(ar, model, k, B):
    """no buffer is handed over: the size alone -- 2 B (K + 1) floats, B int32, a double, one chunk of scores, each on 256 bytes"""
    _ffi, lib = _lib()
    T = Tables(model, k, 33, 35, True)
    need = lib.amdkge_train_relation_workspace_bytes(C.byref(T.m), B)
    rows = min(B, (1 << 24) // 35)
    assert 4 * (2 * B * (T.Ks + 1) + B + rows * 35) + 8 <= need <= 4 * (2 * B * (T.Ks + 1) + B + rows * 35) + 8 + 7 * 256


# entry point of include/amdkge_relation_objective.h -> [(case function, its arguments), ...]
RELATION_CASES = {
    "amdkge_train_relation_workspace_bytes": [(case_workspace_bytes, dict(model="ComplEx", k=50, B=37)), (case_workspace_bytes, dict(model="DistMult", k=7, B=700000))],
    "amdkge_train_relation_fwdbwd": [(case_train_relation, dict(model="ComplEx", k=50, pad=True, ranges=True, outputs=True)),
                                     (case_train_relation, dict(model="DistMult", k=7, pad=False, ranges=True, outputs=True)),
                                     (case_train_relation, dict(model="DistMult", k=7, pad=True, ranges=False, outputs=False)),
                                     (case_train_relation, dict(model="HolE", k=200, pad=True, ranges=True, outputs=False))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in RELATION_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_relation_objective.h")
    assert declared and declared == set(RELATION_CASES) and all(RELATION_CASES.values())
