"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the entry points of
include/amdkge_shared.h are handed: no write outside a buffer, no result that depends on bytes outside one, and the size
amdkge_train_shared_workspace_bytes returns is what the step uses -- the workspace is handed over with exactly that many bytes."""
import ctypes as C

import numpy as np
import pytest

import shared_ref as SR
from abi_decl import declared_names
from oracle import kge_oracle as O
from test_gpu_guard_bands import F32, F64, I32, P, Tables, assert_grads_close, edge_triples, loss_desc, run_case

pytestmark = pytest.mark.gpu

SEED, STEP = 12345678901234, (1 << 33) + 5


def _lib():
    from ampligraph_amd import _ffi

    return _ffi, _ffi.lib()


def case_sample_shared(ar, B, G, M, mode, pool):
    _ffi, lib = _lib()
    rng = np.random.default_rng(7)
    N, R = 130, 5
    X = edge_triples(3, B, N, R)
    tri = ar.put("triples", X)
    thr_np = rng.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    thr = ar.put("thr", thr_np.view(np.int32)) if mode == SR.BERNOULLI else None
    pool_np = np.array([N - 1, 0, 5, 5, 77], I32) if pool else None
    pl = ar.put("pool", pool_np) if pool else None
    ng = SR.n_groups(B, G)
    ids, side = ar.out("ids", (ng, M), I32, -7), ar.out("side", (B,), I32, -7)
    _ffi.check(lib.amdkge_sample_shared(P(tri), B, G, M, 0, N, SEED, STEP, mode, P(thr), P(pl), 5 if pool else 0, P(ids), P(side), None))
    want_ids, want_side = SR.sample_shared(X, G, M, SEED, STEP, sample_range=N, side_mode=mode, side_thr=thr_np, pool=pool_np)
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["ids"], want_ids))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["side"], want_side))


def case_workspace_bytes(ar, model, k):
    """a host-only call: nothing to guard, but every header entry has a case"""
    _ffi, lib = _lib()
    T = Tables(model, k, 130, 4, True)
    assert lib.amdkge_train_shared_workspace_bytes(C.byref(T.m), 37, 5, 33) >= 4 * (2 * 37 * T.Ks + 2 * 37 + 37 * 33)


def case_train_shared(ar, model, k, pad, B=37, G=5, M=33, N=130, R=4):
    """fp32 atomics into both gradient tables, an fp64 atomic into the loss: those three outputs are held to the oracle with the bars of
    test_gpu_guard_bands.py's train_fwdbwd case; the scores (a deterministic product) bitwise between the runs."""
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    ids_np, side_np = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    ids_np[0, 0], ids_np[-1, -1] = N - 1, 0                                # the table's last and first row among the replacements
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    ids, side = ar.put("ids", ids_np), ar.put("side", side_np)
    ge, gr = ar.out("g_ent", (N, T.Ks), F32, 0.0), ar.out("g_rel", (R, T.Ks), F32, 0.0)
    ls = ar.out("loss", (1,), F64, 0.0)
    ps, ns = ar.out("pos_scores", (B,), F32, 7.0), ar.out("neg_scores", (B * M,), F32, 7.0)
    need = lib.amdkge_train_shared_workspace_bytes(C.byref(T.m), B, G, M)
    assert need > 0
    work = ar.work("work", need)
    _ffi.check(lib.amdkge_train_shared_fwdbwd(C.byref(T.m), C.byref(loss_desc("self_adversarial")), P(ent), P(rel), P(tri), B, G, M, P(ids), P(side),
                                              P(ge), P(gr), P(ls), P(ps), P(ns), P(work), None))
    ar.loose |= {"g_ent", "g_rel", "loss"}
    negs = SR.override_rows(X, G, ids_np, side_np)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, T.ent, T.rel, X, negs, M, "self_adversarial", None, "sum", R)

    def oracle(o):
        assert np.allclose(o["pos_scores"], sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(o["neg_scores"], sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(float(o["loss"][0]) - float(total)) <= 2e-5 * max(1.0, abs(float(o["loss"][0])))
        assert_grads_close(T.dense(o["g_ent"]), Te)
        assert_grads_close(T.dense(o["g_rel"]), Tr)

    ar.expects.append(oracle)


# entry point of include/amdkge_shared.h -> [(case function, its arguments), ...]
SHARED_CASES = {
    "amdkge_sample_shared": [(case_sample_shared, dict(B=37, G=5, M=33, mode=SR.BERNOULLI, pool=True)),
                             (case_sample_shared, dict(B=37, G=5, M=33, mode=SR.UNIFORM, pool=False)),
                             (case_sample_shared, dict(B=1, G=1, M=1, mode=SR.S_ONLY, pool=False))],
    "amdkge_train_shared_workspace_bytes": [(case_workspace_bytes, dict(model="ComplEx", k=50))],
    "amdkge_train_shared_fwdbwd": [(case_train_shared, dict(model="ComplEx", k=50, pad=True)), (case_train_shared, dict(model="DistMult", k=7, pad=False)),
                                   (case_train_shared, dict(model="HolE", k=200, pad=True))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in SHARED_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_shared.h")
    assert declared and declared == set(SHARED_CASES) and all(SHARED_CASES.values())
