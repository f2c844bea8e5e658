"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the three entry points of
include/amdkge_shared_labels.h are handed: no write outside a buffer, no result that depends on bytes outside one, the workspace
handed over with exactly its *_workspace_bytes bytes -- as tests/test_gpu_shared_mask_guard.py does for the masked step.  The id
arrays are exact to the byte and the last row's range ends at their last id: the identity walk's 64-id window must stop there."""
import ctypes as C

import numpy as np
import pytest

import shared_labels_ref as LR
import shared_ref as SR
from abi_decl import declared_names
from test_gpu_guard_bands import F32, F64, I32, P, Tables, assert_grads_close, edge_triples, run_case
from test_gpu_shared_mask_guard import I64, _lib, _ranges

pytestmark = pytest.mark.gpu


def _weights(ar, B):
    rng = np.random.default_rng(7)
    ws, wo = rng.uniform(0.2, 1.0, B).astype(F32), rng.uniform(0.2, 1.0, B).astype(F32)
    return (ws, wo), (ar.put("w_s", ws), ar.put("w_o", wo))


def case_label_loss(ar, B, G, M, N, identity, row0, rows, weights):
    _ffi, lib = _lib()
    R = 3
    X = edge_triples(5, B, N, R)
    if identity:
        ids_np = np.tile(np.arange(M, dtype=I32), (SR.n_groups(B, G), 1))
        side_np = SR.sample_shared(X, G, 1, 1, 0, sample_range=N)[1]
    else:
        ids_np, side_np = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    ks, ko, rg = _ranges(ar, X, N, R)
    assert len(ks[B - 1]) and len(ko[B - 1])                                  # the last row's range ends at the id array's last element
    S0 = (np.random.default_rng(2).normal(size=(rows, M)) * 2).astype(F32)
    S = ar.put("scores", S0, "out")
    ids = None if identity else ar.put("ids", ids_np)
    side = ar.put("side", side_np)
    w_np, w_dev = _weights(ar, B) if weights else (None, (None, None))
    stats = ar.out("stats", (2,), I64, 0)
    ls = ar.out("loss", (1,), F64, 0.0)
    eps, scale = 0.1, -0.5
    _ffi.check(lib.amdkge_shared_label_loss(P(S), row0, rows, min(G, B), M, P(ids), P(side), *(P(t) for t in rg), 1 if identity else 0, eps, 1, scale,
                                            P(w_dev[0]), P(w_dev[1]), P(ls), P(stats), None))
    ar.loose.add("loss")                                                      # (one fp64 atomic per workgroup, unordered)
    labels = LR.label_matrix(X, G, ids_np, side_np, ks, ko)[0][row0:row0 + rows]
    rw = LR.row_weights(side_np, w_np)[row0:row0 + rows]
    total, want = LR.label_loss(S0, labels, eps, "mean", scale, rw)

    def expect(o):
        assert (np.abs(o["scores"] - want) <= 1e-5 * abs(scale) * rw[:, None] / M).all()
        assert abs(float(o["loss"][0]) - total) <= 1e-5 * abs(total)
        assert o["stats"].tolist() == [int(labels.sum()), int((~labels.any(1)).sum())]

    ar.expects.append(expect)


def case_train_labels(ar, model, k, pad, identity, weights, B=37, G=5, N=33, R=4):
    """test_gpu_shared_mask_guard.py's case of the masked step; M = N = 33 so that the identity list is a legal one"""
    _ffi, lib = _lib()
    M = N
    dist = model in ("TransE", "RotatE")
    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    ids_np, side_np = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    if identity:
        ids_np = np.tile(np.arange(M, dtype=I32), (SR.n_groups(B, G), 1))
    ks, ko, rg = _ranges(ar, X, N, R)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    ids, side = ar.put("ids", ids_np), ar.put("side", side_np)
    w_np, w_dev = _weights(ar, B) if weights else (None, (None, None))
    ge, gr = ar.out("g_ent", (N, T.Ks), F32, 0.0), ar.out("g_rel", (R, T.Ks), F32, 0.0)
    ls = ar.out("loss", (1,), F64, 0.0)
    ps, ns = ar.out("pos_scores", (B,), F32, 7.0), ar.out("neg_scores", (B * M,), F32, 7.0)
    stats = ar.out("stats", (2,), I64, 0)
    need = (lib.amdkge_train_shared_dist_workspace_bytes if dist else lib.amdkge_train_shared_workspace_bytes)(C.byref(T.m), B, G, M)
    assert need > 0
    work = ar.work("work", need)
    fn = lib.amdkge_train_shared_dist_labels_fwdbwd if dist else lib.amdkge_train_shared_labels_fwdbwd
    _ffi.check(fn(C.byref(T.m), 0.1, 0, P(ent), P(rel), P(tri), B, G, M, P(ids), P(side), P(ge), P(gr), P(ls), P(ps), P(ns), P(work), *(P(t) for t in rg),
                  1 if identity else 0, P(w_dev[0]), P(w_dev[1]), P(stats), None))
    ar.loose |= {"g_ent", "g_rel", "loss"}
    labels, n_lab, n_none = LR.label_matrix(X, G, ids_np, side_np, ks, ko)
    assert n_lab > 0
    total, Te, Tr, sp, sn = LR.labelled_step(model, T.ent, T.rel, X, G, ids_np, side_np, labels, 0.1, "sum", w_np, R)

    def oracle(o):
        assert np.allclose(o["pos_scores"], sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(o["neg_scores"], sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(float(o["loss"][0]) - total) <= 2e-5 * max(1.0, abs(float(o["loss"][0])))
        assert_grads_close(T.dense(o["g_ent"]), Te)
        assert_grads_close(T.dense(o["g_rel"]), Tr)
        assert o["stats"].tolist() == [n_lab, n_none]

    ar.expects.append(oracle)


def case_train_dist_labels(ar, **kw):
    case_train_labels(ar, **kw)


# entry point of include/amdkge_shared_labels.h -> [(case function, its arguments), ...]
LABEL_CASES = {
    "amdkge_shared_label_loss": [(case_label_loss, dict(B=37, G=5, M=65, N=40, identity=False, row0=0, rows=37, weights=True)),
                                 (case_label_loss, dict(B=37, G=5, M=33, N=40, identity=False, row0=9, rows=17, weights=False)),
                                 (case_label_loss, dict(B=37, G=5, M=40, N=40, identity=True, row0=9, rows=28, weights=True)),
                                 (case_label_loss, dict(B=37, G=5, M=23, N=40, identity=True, row0=0, rows=37, weights=False)),
                                 (case_label_loss, dict(B=1, G=1, M=1, N=2, identity=False, row0=0, rows=1, weights=False))],
    "amdkge_train_shared_labels_fwdbwd": [(case_train_labels, dict(model="ComplEx", k=50, pad=True, identity=False, weights=False)),
                                          (case_train_labels, dict(model="DistMult", k=7, pad=False, identity=True, weights=True)),
                                          (case_train_labels, dict(model="HolE", k=200, pad=True, identity=True, weights=False))],
    "amdkge_train_shared_dist_labels_fwdbwd": [(case_train_dist_labels, dict(model="TransE", k=50, pad=True, identity=True, weights=True)),
                                               (case_train_dist_labels, dict(model="RotatE", k=12, pad=True, identity=False, weights=False))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in LABEL_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_shared_labels.h")
    assert declared and declared == set(LABEL_CASES) and all(LABEL_CASES.values())
