"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the entry points of
include/amdkge_shared_dist.h are handed: no write outside a buffer, no result that depends on bytes outside one, the workspace handed
over with exactly amdkge_train_shared_dist_workspace_bytes bytes -- as tests/test_gpu_shared_guard.py does for the matrix-product step.
The scores (plain stores of a fixed summation order) are bitwise equal between the runs; the gradients and the loss (atomics) are
held to the header's arithmetic restated in numpy (tests/shared_dist_ref.py), which needs no condition on the inputs."""
import ctypes as C

import numpy as np
import pytest

import shared_dist_ref as DR
import shared_mask_ref as MR
import shared_ref as SR
from abi_decl import declared_names
from test_gpu_guard_bands import F32, F64, I32, P, Tables, assert_grads_close, edge_triples, loss_desc, run_case

pytestmark = pytest.mark.gpu

I64 = np.int64


def _lib():
    from ampligraph_amd import _ffi

    return _ffi, _ffi.lib()


def case_workspace_bytes(ar, model, k):
    """a host-only call: nothing to guard, but every header entry has a case"""
    _ffi, lib = _lib()
    T = Tables(model, k, 130, 4, True)
    assert lib.amdkge_train_shared_dist_workspace_bytes(C.byref(T.m), 37, 5, 33) >= 4 * (2 * 37 * T.Ks + 2 * 37 + 37 * 33)


def case_train_shared_dist(ar, model, k, pad, masked, B=37, G=5, M=33, N=130, R=4):
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    ids_np, side_np = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    ids_np[0, 0], ids_np[-1, -1] = N - 1, 0                                # the table's last and first row among the replacements
    mask = None
    rg = [None] * 6
    if masked:                                                             # the batch's own statements and every group's first three entries are known
        ks, ko = MR.known_lists(X, [X], N, R)
        grp = np.arange(B) // G
        ks = [np.unique(np.concatenate([a, ids_np[g, :3]])).astype(I32) for a, g in zip(ks, grp)]
        ko = [np.unique(np.concatenate([a, ids_np[g, :3]])).astype(I32) for a, g in zip(ko, grp)]
        (slo, shi, sid), (olo, ohi, oid) = MR.csr(ks), MR.csr(ko)
        rg = [ar.put(n, a) for n, a in (("s_lo", slo), ("s_hi", shi), ("s_ids", sid), ("o_lo", olo), ("o_hi", ohi), ("o_ids", oid))]
        mask, n_masked, unmaskable = MR.mask_matrix(X, G, ids_np, side_np, ks, ko)
        assert n_masked >= 3 * B and unmaskable == 0
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    ids, side = ar.put("ids", ids_np), ar.put("side", side_np)
    ge, gr = ar.out("g_ent", (N, T.Ks), F32, 0.0), ar.out("g_rel", (R, T.Ks), F32, 0.0)
    ls = ar.out("loss", (1,), F64, 0.0)
    ps, ns = ar.out("pos_scores", (B,), F32, 7.0), ar.out("neg_scores", (B * M,), F32, 7.0)
    stats = ar.out("stats", (2,), I64, 0)
    need = lib.amdkge_train_shared_dist_workspace_bytes(C.byref(T.m), B, G, M)
    assert need > 0
    work = ar.work("work", need)
    _ffi.check(lib.amdkge_train_shared_dist_fwdbwd(C.byref(T.m), C.byref(loss_desc("self_adversarial")), P(ent), P(rel), P(tri), B, G, M, P(ids), P(side),
                                                   P(ge), P(gr), P(ls), P(ps), P(ns), P(work), *(P(t) for t in rg), 0, P(stats), None))
    ar.loose |= {"g_ent", "g_rel", "loss"}                                 # atomics; the scores and the stats are bitwise equal between the runs
    total, Te, Tr, sp, sn = DR.DistStep(model, T.ent, T.rel, X, G, ids_np, side_np, R).step("self_adversarial", "sum", mask=mask)
    live = np.isfinite(sn)

    def ref(o):
        assert np.allclose(o["pos_scores"], sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.array_equal(np.isneginf(o["neg_scores"]), ~live) and (masked or live.all())
        assert np.allclose(o["neg_scores"][live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
        assert abs(float(o["loss"][0]) - total) <= 2e-5 * max(1.0, abs(float(o["loss"][0])))
        assert_grads_close(T.dense(o["g_ent"]), Te)
        assert_grads_close(T.dense(o["g_rel"]), Tr)
        assert o["stats"].tolist() == ([int(mask.sum()), 0] if masked else [0, 0])

    ar.expects.append(ref)


# entry point of include/amdkge_shared_dist.h -> [(case function, its arguments), ...]
DIST_CASES = {
    "amdkge_train_shared_dist_workspace_bytes": [(case_workspace_bytes, dict(model="RotatE", k=50))],
    "amdkge_train_shared_dist_fwdbwd": [(case_train_shared_dist, dict(model="TransE", k=7, pad=False, masked=False)),
                                        (case_train_shared_dist, dict(model="TransE", k=7, pad=False, masked=True)),
                                        (case_train_shared_dist, dict(model="RotatE", k=50, pad=True, masked=False)),
                                        (case_train_shared_dist, dict(model="RotatE", k=50, pad=True, masked=True))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in DIST_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_shared_dist.h")
    assert declared and declared == set(DIST_CASES) and all(DIST_CASES.values())
