"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the entry points of
include/amdkge_shared_mask.h are handed: no write outside a buffer, no result that depends on bytes outside one, the workspace
handed over with exactly amdkge_train_shared_workspace_bytes bytes -- as tests/test_gpu_shared_guard.py does for the unmasked step."""
import ctypes as C

import numpy as np
import pytest

import shared_mask_ref as MR
from abi_decl import declared_names
import shared_ref as SR
from test_gpu_guard_bands import F32, F64, I32, P, Tables, assert_grads_close, edge_triples, loss_desc, run_case

pytestmark = pytest.mark.gpu

I64 = np.int64


def _lib():
    from ampligraph_amd import _ffi

    return _ffi, _ffi.lib()


def _ranges(ar, X, N, R):
    """the six range arrays of the batch over a graph that holds it: every positive's own entity is known"""
    rng = np.random.default_rng(11)
    more = np.stack([rng.integers(0, N, 400), rng.integers(0, R, 400), rng.integers(0, N, 400)], 1)
    more[:200, 1:] = X[rng.integers(0, len(X), 200), 1:]                   # more subjects for the batch's own (p, o) ...
    more[200:, :2] = X[rng.integers(0, len(X), 200), :2]                   # ... and more objects for its (s, p)
    ks, ko = MR.known_lists(X, [X, more], N, R)
    (slo, shi, sid), (olo, ohi, oid) = MR.csr(ks), MR.csr(ko)
    dev = [ar.put(n, a) for n, a in (("s_lo", slo), ("s_hi", shi), ("s_ids", sid), ("o_lo", olo), ("o_hi", ohi), ("o_ids", oid))]
    return ks, ko, dev


def case_mask_scores(ar, B, G, M, N, identity, row0, rows):
    _ffi, lib = _lib()
    R = 3
    X = edge_triples(5, B, N, R)
    if identity:
        ids_np = np.tile(np.arange(M, dtype=I32), (SR.n_groups(B, G), 1))
        side_np = SR.sample_shared(X, G, 1, 1, 0, sample_range=N)[1]
    else:
        ids_np, side_np = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    ks, ko, rg = _ranges(ar, X, N, R)
    S0 = np.random.default_rng(2).normal(size=(rows, M)).astype(F32)
    S = ar.put("scores", S0, "out")
    ids = None if identity else ar.put("ids", ids_np)
    side = ar.put("side", side_np)
    stats = ar.out("stats", (2,), I64, 0)
    _ffi.check(lib.amdkge_shared_mask_scores(P(S), row0, rows, min(G, B), M, P(ids), P(side), *(P(t) for t in rg), 1 if identity else 0, P(stats), None))
    mask, _, _ = MR.mask_matrix(X, G, ids_np, side_np, ks, ko)
    mask = mask[row0:row0 + rows]
    full = sum(1 for i in range(row0, row0 + rows) if np.isin(ids_np[i // min(G, B)], ks[i] if side_np[i] else ko[i]).all())

    def expect(o):
        assert np.array_equal(np.isneginf(o["scores"]), mask)
        assert np.array_equal(o["scores"][~mask].view(np.uint32), S0[~mask].view(np.uint32))
        assert o["stats"].tolist() == [int(mask.sum()), full]

    ar.expects.append(expect)


def case_train_shared_masked(ar, model, k, pad, identity, B=37, G=5, N=33, R=4):
    """the bars of test_gpu_shared_guard.py's case; M = N = 33 so that the identity list is a legal one"""
    _ffi, lib = _lib()
    M = N
    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    ids_np, side_np = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    if identity:
        ids_np = np.tile(np.arange(M, dtype=I32), (SR.n_groups(B, G), 1))
    ks, ko, rg = _ranges(ar, X, N, R)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    ids, side = ar.put("ids", ids_np), ar.put("side", side_np)
    ge, gr = ar.out("g_ent", (N, T.Ks), F32, 0.0), ar.out("g_rel", (R, T.Ks), F32, 0.0)
    ls = ar.out("loss", (1,), F64, 0.0)
    ps, ns = ar.out("pos_scores", (B,), F32, 7.0), ar.out("neg_scores", (B * M,), F32, 7.0)
    stats = ar.out("stats", (2,), I64, 0)
    need = lib.amdkge_train_shared_workspace_bytes(C.byref(T.m), B, G, M)
    assert need > 0
    work = ar.work("work", need)
    _ffi.check(lib.amdkge_train_shared_masked_fwdbwd(C.byref(T.m), C.byref(loss_desc("self_adversarial")), P(ent), P(rel), P(tri), B, G, M, P(ids), P(side),
                                                     P(ge), P(gr), P(ls), P(ps), P(ns), P(work), *(P(t) for t in rg), 1 if identity else 0, P(stats), None))
    ar.loose |= {"g_ent", "g_rel", "loss"}
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids_np, side_np, ks, ko)
    assert masked > 0
    total, Te, Tr, sp, sn = MR.masked_step(model, T.ent, T.rel, X, G, ids_np, side_np, mask, "self_adversarial", "sum", R)
    live = np.isfinite(sn)

    def oracle(o):
        assert np.allclose(o["pos_scores"], sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.array_equal(np.isneginf(o["neg_scores"]), ~live)
        assert np.allclose(o["neg_scores"][live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
        assert abs(float(o["loss"][0]) - total) <= 2e-5 * max(1.0, abs(float(o["loss"][0])))
        assert_grads_close(T.dense(o["g_ent"]), Te)
        assert_grads_close(T.dense(o["g_rel"]), Tr)
        assert o["stats"].tolist() == [masked, unmaskable]

    ar.expects.append(oracle)


# entry point of include/amdkge_shared_mask.h -> [(case function, its arguments), ...]
MASK_CASES = {
    "amdkge_shared_mask_scores": [(case_mask_scores, dict(B=37, G=5, M=65, N=40, identity=False, row0=0, rows=37)),
                                  (case_mask_scores, dict(B=37, G=5, M=33, N=40, identity=False, row0=9, rows=17)),
                                  (case_mask_scores, dict(B=37, G=5, M=23, N=40, identity=True, row0=9, rows=28)),
                                  (case_mask_scores, dict(B=1, G=1, M=1, N=2, identity=False, row0=0, rows=1))],
    "amdkge_train_shared_masked_fwdbwd": [(case_train_shared_masked, dict(model="ComplEx", k=50, pad=True, identity=False)),
                                          (case_train_shared_masked, dict(model="DistMult", k=7, pad=False, identity=True)),
                                          (case_train_shared_masked, dict(model="HolE", k=200, pad=True, identity=False))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in MASK_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_shared_mask.h")
    assert declared and declared == set(MASK_CASES) and all(MASK_CASES.values())
