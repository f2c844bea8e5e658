"""Shared-negative training on the GPU (kge_train_shared.hip, include/amdkge_shared.h): the draw against its numpy restatement bit for
bit, the matrix-product forward / backward against the oracle on the EQUIVALENT override rows (tests/shared_ref.py: override_rows is
the step's definition), against the fused per-corruption kernel on the same rows, whole optimizer steps, fit() as a drop-in."""
import ctypes as C

import numpy as np
import pytest
import torch

import shared_ref as SR
from margins import within
from oracle import kge_oracle as O
from test_gpu_kernels import assert_grads_close, dense, dev, loss_desc, make_engine, make_optimizer, rand_triples, run_fwdbwd

pytestmark = pytest.mark.gpu

SHARED_MODELS = ("DistMult", "ComplEx", "HolE")
LOSSES = list(O.LOSS_DEFAULTS)
SEED, STEP = 12345678901234, (1 << 33) + 5


def run_shared(eng, X, G, ids, side, loss_name, reduction):
    """-> (loss sum, dense entity gradient, dense relation gradient, positive scores, corruption scores [M * B])"""
    B, M = X.shape[0], ids.shape[1]
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * M,), 7.0, dtype=torch.float32, device="cuda")
    eng.train_shared_fwdbwd(dev(X), G, M, dev(ids), dev(side), loss_desc(loss_name, reduction), pos_scores=ps, neg_scores=ns)
    torch.cuda.synchronize()
    return float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel), ps.cpu().numpy(), ns.cpu().numpy()


def grad_gap(G, T):
    """assert_grads_close's figure: the largest error relative to the row's magnitude"""
    T = T.astype(np.float64)
    scale = np.maximum(np.abs(T).max(axis=1, keepdims=True), 1e-6 * max(np.abs(T).max(), 1e-30))
    return float((np.abs(G - T) / scale).max())


def check_against_oracle(model, ent, rel, X, G, ids, side, got, loss, reduction, R, tag=""):
    L, Ge, Gr, ps, ns = got
    M = ids.shape[1]
    negs = SR.override_rows(X, G, ids, side)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, M, loss, None, reduction, R)
    want = float(per.astype(np.float64).sum())
    print(f"{tag} {model} {loss} {reduction}: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, "
          f"score gap {np.abs(ns - sn).max() / np.abs(sn).max():.3g}")
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)
    return Te, Tr


# ------------------------------------------------------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("B,G,M,N", [(1, 1, 1, 1), (37, 8, 5, 10), (1000, 256, 256, 14505)])
def test_draw_bit_for_bit(gpu_lib, B, G, M, N):
    from ampligraph_amd.engine import KgeEngine

    R = 3
    eng = KgeEngine("DistMult", 4, max(N, 2), R)
    rng = np.random.default_rng(2)
    X = rand_triples(rng, B, max(N, 2), R)
    thr = rng.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    pool = rng.integers(0, max(N, 2), 7).astype(np.int32)
    for mode in (SR.UNIFORM, SR.BERNOULLI, SR.S_ONLY, SR.O_ONLY):
        for pl in (None, pool):
            ids, side = eng.sample_shared(dev(X), G, M, SEED, STEP, sample_range=N, side=SR.SIDE_NAMES[mode],
                                          side_thr=dev(thr.view(np.int32)) if mode == SR.BERNOULLI else None, pool=None if pl is None else dev(pl))
            torch.cuda.synchronize()
            want_ids, want_side = SR.sample_shared(X, G, M, SEED, STEP, sample_range=N, side_mode=mode, side_thr=thr, pool=pl)
            got_ids, got_side = ids.cpu().numpy(), side.cpu().numpy()
            assert got_ids.dtype == want_ids.dtype and got_ids.shape == want_ids.shape and np.array_equal(got_ids, want_ids), (mode, pl is None)
            assert got_side.dtype == want_side.dtype and np.array_equal(got_side, want_side), (mode, pl is None)


# ------------------------------------------------------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("model", SHARED_MODELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_shared_fwdbwd_parity(gpu_lib, model, loss):
    """B = 257 in groups of 64: a last group of ONE positive; M = 33 crosses the 32-wide MFMA tile.  The bars of
    test_gpu_kernels.py::test_train_fwdbwd_parity."""
    N, R, k, B, G, M = 300, 5, 32, 257, 64, 33
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X = rand_triples(np.random.default_rng(3), B, N, R)
    ids, side = SR.sample_shared(X, G, M, 9, 4, sample_range=N)
    assert ids.shape == (5, M) and 0 < side.sum() < B
    for reduction in ("sum", "mean"):
        check_against_oracle(model, ent, rel, X, G, ids, side, run_shared(eng, X, G, ids, side, loss, reduction), loss, reduction, R)


# ------------------------------------------------------------------------------------------------------------------ 3. geometries
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("G", [37, 5])
@pytest.mark.parametrize("model,k", [("DistMult", 7), ("DistMult", 400), ("ComplEx", 200), ("ComplEx", 350), ("HolE", 50)])
def test_shared_fwdbwd_geometries(gpu_lib, model, k, G, pad):
    """The K tail of the contraction chunks (K = 7, 100, 700 are no multiples of 32), padded units, a group smaller than a tile (5) and one
    that is the whole batch (37), M = 130 = two tiles and two columns.  The bars of item 2, unchanged."""
    N, R, B, M = 200, 4, 37, 130
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3 if k < 100 else 0.08, pad=pad)
    X = rand_triples(np.random.default_rng(4), B, N, R)
    ids, side = SR.sample_shared(X, G, M, 1, 0, sample_range=N)
    check_against_oracle(model, ent, rel, X, G, ids, side, run_shared(eng, X, G, ids, side, "self_adversarial", "sum"), "self_adversarial", "sum", R,
                         tag=f"G={G} pad={pad} k={k}")
    if pad:   # the padding units of the gradient tables stay exact zeros
        stored = eng.g_ent.cpu().numpy().reshape(N, -1, eng.ks)
        assert not stored[:, :, eng.k:].any()


# ------------------------------------------------------------------------------------------------------------------ 4. duplicates
@pytest.mark.parametrize("model", SHARED_MODELS)
def test_shared_duplicates(gpu_lib, model):
    """N = 5 entities, M = 12: every list repeats ids and holds the positives' own entities; s == o positives and a repeated positive."""
    N, R, k, G, M = 5, 2, 8, 4, 12
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X = rand_triples(np.random.default_rng(5), 11, N, R)
    X[2] = (3, 1, 3)
    X[3] = (0, 0, 0)
    X[7] = X[6] = X[1]
    ids, side = SR.sample_shared(X, G, M, 2, 3, sample_range=N)
    assert all(len(set(row.tolist())) < M for row in ids)
    for loss in ("multiclass_nll", "pairwise"):
        check_against_oracle(model, ent, rel, X, G, ids, side, run_shared(eng, X, G, ids, side, loss, "mean"), loss, "mean", R)


# ------------------------------------------------------------------------------------------------------------------ 5. two formulations
@pytest.mark.parametrize("model,k", [("DistMult", 48), ("ComplEx", 100), ("HolE", 36)])
def test_shared_equals_the_fused_kernel_on_the_override_rows(gpu_lib, model, k):
    """The same step through amdkge_train_fwdbwd(d_neg_override = the equivalent rows): both paths add with fp32 atomics in arrival
    order, so the bar is item 2's (row-scaled 2e-5 on the gradients, 1e-5 on scores and loss), through margins.within."""
    N, R, B, G, M = 150, 4, 70, 32, 40
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3)
    X = rand_triples(np.random.default_rng(6), B, N, R)
    ids, side = SR.sample_shared(X, G, M, 5, 6, sample_range=N, side_mode=SR.S_ONLY if model == "HolE" else SR.UNIFORM)
    L1, Ge1, Gr1, ps1, ns1 = run_shared(eng, X, G, ids, side, "nll", "mean")
    L2, Ge2, Gr2, ps2, ns2 = run_fwdbwd(eng, X, M, "nll", "mean", seed=0, step=0, negs=SR.override_rows(X, G, ids, side))
    assert within("shared_vs_fused_grad_ent", grad_gap(Ge1, Ge2), 2e-5)
    assert within("shared_vs_fused_grad_rel", grad_gap(Gr1, Gr2), 2e-5)
    assert within("shared_vs_fused_loss", abs(L1 - L2) / max(1.0, abs(L2)), 1e-5)
    assert np.allclose(ps1, ps2, rtol=1e-5, atol=1e-5 * np.abs(ps2).max()) and np.allclose(ns1, ns2, rtol=1e-5, atol=1e-5 * np.abs(ns2).max())


# ------------------------------------------------------------------------------------------------------------------ 6. whole steps
@pytest.mark.parametrize("model,k", [("ComplEx", 40), ("DistMult", 64), ("HolE", 24)])
def test_shared_whole_steps_match_oracle(gpu_lib, model, k):
    """Three Adam steps (draw on the device -> forward / backward -> amdkge_opt_step with an L2 regulariser) == the oracle's dense steps
    on the override rows: tables and slots, with the bars of test_gpu_cols.py::test_cols_whole_steps_match_oracle."""
    N, R, B, G, M, seed = 200, 4, 151, 40, 24, 4
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3)
    w, mk = make_optimizer("adam", {})
    st = mk(ent, rel)
    eng.prepare_training(w.name)
    rng = np.random.default_rng(5)
    ld = loss_desc("self_adversarial", "sum")
    oreg = dict(p=2, lam_e=1e-3, lam_r=1e-3)
    for t in range(1, 4):
        X = rand_triples(rng, B, N, R)
        Xd = dev(X)
        eng.loss_acc.zero_()
        ids, side = eng.sample_shared(Xd, G, M, seed, t)
        eng.train_shared_fwdbwd(Xd, G, M, ids, side, ld)
        eng.opt_step(w.to_ffi(t, 2), 1e-3, 1e-3)
        torch.cuda.synchronize()
        want_ids, want_side = SR.sample_shared(X, G, M, seed, t, sample_range=N)
        assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(side.cpu().numpy(), want_side)
        ref = float(O.train_step(st, model, X, M, "self_adversarial", seed, t, max_rel_size=R, reg=oreg, negs=SR.override_rows(X, G, want_ids, want_side)))
        tot = float(eng.loss_acc[0].item()) + float(eng.loss_acc[1].item())
        assert abs(tot - ref) <= 3e-5 * abs(ref), (t, tot, ref)
        assert not eng.g_flat.any().item()                                  # the sweep left the gradient buffers zero
    E, Rl = eng.get_tables()
    assert np.mean(np.abs(E - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.995 and np.abs(E - st.ent).max() < 2.5e-2
    assert np.mean(np.abs(Rl - st.rel) <= 1e-5 + 1e-3 * np.abs(st.rel)) > 0.99
    for nme in st.slots:
        if nme.endswith("_e"):
            S = dense(eng, eng.slots[nme])
            ok = np.isclose(S, st.slots[nme], rtol=2e-3, atol=1e-6 + 2e-5 * np.abs(st.slots[nme]).max())
            assert ok.mean() > 0.99, (nme, ok.mean())


# ------------------------------------------------------------------------------------------------------------------ 7. drop-in
class _RestatedShared:
    """What compile(negatives=SharedNegatives(num_negs, group_size)) computes, through the PER-CORRUPTION path: bind() -> a
    StepLoop.negatives that uploads the equivalent override rows of the numpy restatement (the model's eta must be num_negs)."""

    def __init__(self, num_negs, group_size):
        self.M, self.G, self.calls = num_negs, group_size, 0

    def bind(self, model, engine, train):
        self.N = int(model._n_ents)
        return self

    def __call__(self, global_batch, lo, hi, eta, seed, step):
        assert eta == self.M and lo == 0 and hi == int(global_batch.shape[0])
        X = global_batch.cpu().numpy()
        ids, side = SR.sample_shared(X, self.G, self.M, seed, step, sample_range=self.N)
        self.calls += 1
        self.last = dev(SR.override_rows(X, self.G, ids, side))
        return self.last


def test_fit_with_shared_negatives_equals_fit_on_the_override_rows(gpu_lib):
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.latent_features.negatives import BoundSharedNegatives, SharedNegatives

    X = toy_graph(seed=4, n=400, N=40, R=3)
    M, G = 48, 20

    def new(eta, **kw):
        m = ScoringBasedEmbeddingModel(eta=eta, k=16, scoring_type="ComplEx", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", entity_relation_regularizer="l2", **kw)
        return m

    m1 = new(2, negatives=SharedNegatives(num_negs=M, group_size=G))       # (the model's own eta plays no part)
    h1 = m1.fit(X, batch_size=128, epochs=3, verbose=False)                # 4 batches per epoch, the last one of 16; 7 groups, the last of 8
    assert isinstance(m1._loop.negatives, BoundSharedNegatives)
    m2 = new(M)
    m2._negatives = stub = _RestatedShared(M, G)
    h2 = m2.fit(X, batch_size=128, epochs=3, verbose=False)
    assert stub.calls == 12 and m2._loop.negatives is stub
    print("loss histories", h1.history["loss"], h2.history["loss"])
    assert len(h1.history["loss"]) == 3 and np.allclose(h1.history["loss"], h2.history["loss"], rtol=2e-4)
    assert np.allclose(m1.predict(X[:80]), m2.predict(X[:80]), rtol=1e-3, atol=1e-4)
    # the setting did something: the default draw at the same eta gives another history
    h3 = new(M).fit(X, batch_size=128, epochs=3, verbose=False)
    assert not np.allclose(h1.history["loss"], h3.history["loss"], rtol=2e-4)
    # a pool and the Bernoulli side through fit(); what the device path refuses
    ents = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
    m4 = new(2, negatives={"shared": 16, "side": "bernoulli", "entities": ents[:6]})
    m4.fit(X, batch_size=128, epochs=1, verbose=False)
    b = m4._loop.negatives
    ids, side = b.draw(torch.as_tensor(m4.data_indexer.get_indexes(X[:128]).astype(np.int32)).cuda(), m4.seed, 0)
    assert set(ids.cpu().numpy().ravel().tolist()) <= set(m4.data_indexer.get_indexes(ents[:6], "e").tolist()) and ids.shape == (8, 16)
    assert np.isfinite(m4.history.history["loss"]).all()
    m5 = new(2, negatives={"shared": 16, "entities": ["no such entity"]})
    with pytest.raises(ValueError, match="not in the training set"):
        m5.fit(X, batch_size=128, epochs=1, verbose=False)
    Xf = np.concatenate([X, np.ones((len(X), 1))], 1)
    m6 = new(2, negatives={"shared": 16})
    with pytest.raises(NotImplementedError, match="FocusE"):
        m6.fit(Xf, batch_size=128, epochs=1, verbose=False, focusE=True)


# ------------------------------------------------------------------------------------------------------------------ 9. refusals on the device path
def test_device_path_refusals(gpu_lib):
    """Argument checks only: every call returns before a kernel is launched."""
    from ampligraph_amd import _ffi

    N, R, B, G, M = 50, 3, 10, 4, 6
    X = dev(rand_triples(np.random.default_rng(7), B, N, R))
    ids = torch.zeros(3, M, dtype=torch.int32, device="cuda")
    side = torch.zeros(B, dtype=torch.int32, device="cuda")
    for model in ("TransE", "RotatE"):
        eng, _, _ = make_engine(model, 8, N, R)
        eng.prepare_training("adam")
        assert not eng.shared_supported(B, G, M)
        with pytest.raises(ValueError, match="not offered"):
            eng.train_shared_fwdbwd(X, G, M, ids, side, loss_desc("nll"))
        work = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        rc = eng.lib.amdkge_train_shared_fwdbwd(C.byref(eng.model), C.byref(loss_desc("nll")), eng.ent.data_ptr(), eng.rel.data_ptr(), X.data_ptr(), B, G, M, ids.data_ptr(),
                                                side.data_ptr(), eng.g_ent.data_ptr(), eng.g_rel.data_ptr(), eng.loss_acc.data_ptr(), None, None, work.data_ptr(), None)
        assert rc == -5 and b"contraction" in eng.lib.amdkge_last_error()
    eng, _, _ = make_engine("ComplEx", 8, N, R)
    eng.prepare_training("adam")
    assert eng.shared_supported(B, G, M)
    for bad in ((B, 0, M), (B, G, 0), (B, G, 1 << 24)):
        assert not eng.shared_supported(*bad)
        with pytest.raises(ValueError, match="not offered"):
            eng.train_shared_fwdbwd(X, bad[1], bad[2], ids, side, loss_desc("nll"))
        rc = eng.lib.amdkge_train_shared_fwdbwd(C.byref(eng.model), C.byref(loss_desc("nll")), eng.ent.data_ptr(), eng.rel.data_ptr(), X.data_ptr(), *bad, ids.data_ptr(),
                                                side.data_ptr(), eng.g_ent.data_ptr(), eng.g_rel.data_ptr(), eng.loss_acc.data_ptr(), None, None, ids.data_ptr(), None)
        assert rc == -1 and b"bad sizes" in eng.lib.amdkge_last_error()
    for G_, M_ in ((0, M), (G, 0)):
        with pytest.raises(_ffi.AmdKgeError, match="bad sizes"):
            eng.sample_shared(X, G_, M_, 1, 2)
    torch.cuda.synchronize()
    assert not eng.g_flat.any().item()                                      # nothing ran
