"""The relation-prediction training objective on the GPU (kge_train_relpred.hip, include/amdkge_relation_objective.h): the step
against its numpy restatement on the oracle's override rows (tests/relation_objective_ref.py) for three models, five losses and
both reductions; the matrix edges; the ranges and the weight; the chunked score buffer; NaN / inf; fit() against the steps written
out; a planted graph with save / restore."""
import numpy as np
import pytest
import torch

import relation_objective_ref as RR
from oracle import kge_oracle as O
from test_gpu_kernels import assert_grads_close, dense, dev, loss_desc, make_engine
from test_gpu_shared import grad_gap

pytestmark = pytest.mark.gpu

MODELS = ("DistMult", "ComplEx", "HolE")
LOSSES = list(O.LOSS_DEFAULTS)


def pair_case(B, N, R, seed, n_pair_ents=5, n_graph=None):
    """-> (X, known): a batch whose subjects and objects come from `n_pair_ents` entities, so pairs repeat, cut from a graph over the
    same pairs; known[i] = the relations the graph holds between (s_i, o_i)"""
    rng = np.random.default_rng(seed)
    pool = rng.choice(N, size=min(n_pair_ents, N), replace=False)
    n_graph = n_graph or 2 * B

    def draw(n):
        return np.stack([pool[rng.integers(0, len(pool), n)], rng.integers(0, R, n), pool[rng.integers(0, len(pool), n)]], 1).astype(np.int32)

    D = draw(n_graph)
    X = D[rng.integers(0, len(D), B)]
    return X, RR.known_relations(X, [D])


def run_step(eng, X, loss_name, reduction, weight, known):
    """-> ((loss, dense entity gradient, dense relation gradient, positive scores, relation scores [R * B]), [masked, unmaskable])"""
    B, R = X.shape[0], eng.n_rels
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * R,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    flt = None if known is None else tuple(dev(a) for a in RR.csr(known))
    eng.train_relation_fwdbwd(dev(X), loss_desc(loss_name, reduction), weight, flt=flt, stats=stats, pos_scores=ps, rel_scores=ns)
    torch.cuda.synchronize()
    return (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel), ps.cpu().numpy(), ns.cpu().numpy()), stats.cpu().tolist()


def check_against_step(model, ent, rel, X, mask, got, loss, reduction, weight, tag="", cancelling=False):
    """the shared step's bars (test_gpu_shared_mask.py::check_against_masked_step) on the live scores; the masked ones are -inf.
    cancelling=True (R = 1 only): the one relation score of a row IS the positive's, so dL/dneg = -dL/dpos and the true gradient is
    zero by cancellation of two contributions of the size of weight * 0.5 * |row|.  assert_grads_close's bar -- 2e-5 of the row's
    largest float -- is then a bar of 2e-5 of nothing; it is applied to the scale of what cancels instead: the sums of the
    contributions' absolute values (the fp32 product and the positive's wave sum round one score differently, ~1e-7 relative)."""
    L, Ge, Gr, ps, ns = got
    want, Te, Tr, sp, sn, Ae, Ar = RR.relation_step(model, ent, rel, X, mask, loss, reduction, weight, magnitude=True)
    live = np.isfinite(sn)
    print(f"{tag} {model} {loss} {reduction}: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, "
          f"score gap {np.abs(ns[live] - sn[live]).max() / np.abs(sn[live]).max():.3g}, masked {int((~live).sum())}")
    assert np.array_equal(np.isneginf(ns), ~live) and np.array_equal(~live, mask.T.reshape(-1))
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns[live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    if cancelling:
        for G, T, A in ((Ge, Te, Ae), (Gr, Tr, Ar)):
            scale = np.maximum(A.max(axis=1, keepdims=True), 1e-6 * A.max())
            assert A.max() > 1e-3 and (np.abs(G - T) / scale).max() < 2e-5, (np.abs(G - T) / scale).max()
        return
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_relation_fwdbwd_parity(gpu_lib, model, loss):
    """B = 37, R = 33 crosses the 32-wide MFMA tile, k = 8; weight 0.25; both reductions; pairs repeat, so rows hold several known
    relations"""
    N, R, k, B = 40, 33, 8, 37
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    for seed in (5, 6):
        X, known = pair_case(B, N, R, seed)
        mask, masked, unmaskable = RR.mask_matrix(B, R, known)
        second = int((mask.sum(1) > 1).sum())
        print(f"seed {seed}: masked {masked}, unmaskable {unmaskable}, rows with a second known relation {second}")
        assert masked > B and unmaskable == 0 and second > B // 2 and mask[np.arange(B), X[:, 1]].all()
        for reduction in ("sum", "mean"):
            got, stats = run_step(eng, X, loss, reduction, 0.25, known)
            check_against_step(model, ent, rel, X, mask, got, loss, reduction, 0.25, tag=f"seed {seed}")
            assert stats == [masked, unmaskable]


# ------------------------------------------------------------------------------------------------------------------ 2. matrix edges
@pytest.mark.parametrize("model", ("ComplEx", "DistMult"))
@pytest.mark.parametrize("R,k,B,n_pair,kind", [(65, 7, 37, 5, "padded"), (1, 8, 37, 5, "R=1"), (2, 8, 64, 2, "full tile, fully known rows"),
                                                (33, 8, 1, 5, "B=1")])
def test_matrix_edges(gpu_lib, model, R, k, B, n_pair, kind):
    N = 40
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, known = pair_case(B, N, R, seed=7, n_pair_ents=n_pair, n_graph=5 if R == 2 else None)    # (R = 2: five statements over four pairs)
    mask, masked, unmaskable = RR.mask_matrix(B, R, known)
    print(f"{kind}: Ks {eng.Ks} K {eng.K}, masked {masked}, unmaskable {unmaskable}")
    if kind == "padded":
        assert eng.Ks > eng.K and masked > 0
    elif kind == "R=1":
        assert (masked, unmaskable) == (0, B)               # every row fully known: unmasked and counted
    elif kind.startswith("full tile"):
        assert unmaskable > 0 and masked > 0
    got, stats = run_step(eng, X, "multiclass_nll", "sum", 0.25, known)
    check_against_step(model, ent, rel, X, mask, got, "multiclass_nll", "sum", 0.25, tag=kind, cancelling=R == 1)
    assert stats == [masked, unmaskable]
    if eng.Ks > eng.K:                                      # the padding floats of both gradient tables were never written
        pad = np.ones(eng.Ks // eng.ks * eng.ks, dtype=bool).reshape(-1, eng.ks)
        pad[:, :eng.k] = False
        assert not eng.g_ent.cpu().numpy()[:, pad.reshape(-1)].any() and not eng.g_rel.cpu().numpy()[:, pad.reshape(-1)].any()


# ------------------------------------------------------------------------------------------------------------------ 3. ranges and weight
@pytest.mark.parametrize("model", MODELS)
def test_null_ranges_equal_empty_ranges(gpu_lib, model):
    N, R, k, B = 40, 33, 8, 37
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, known = pair_case(B, N, R, seed=8)
    none = [a[:0] for a in known]
    (L0, Ge0, Gr0, ps0, ns0), st0 = run_step(eng, X, "self_adversarial", "mean", 0.5, None)
    (L1, Ge1, Gr1, ps1, ns1), st1 = run_step(eng, X, "self_adversarial", "mean", 0.5, none)
    assert np.array_equal(ns0.view(np.uint32), ns1.view(np.uint32)) and np.array_equal(ps0.view(np.uint32), ps1.view(np.uint32)) and st0 == st1 == [0, 0]
    assert grad_gap(Ge0, Ge1) <= 2e-5 and grad_gap(Gr0, Gr1) <= 2e-5 and abs(L0 - L1) <= 1e-5 * max(1.0, abs(L0))
    check_against_step(model, ent, rel, X, np.zeros((B, R), dtype=bool), (L0, Ge0, Gr0, ps0, ns0), "self_adversarial", "mean", 0.5)


def test_own_relation_ranges_mask_exactly_the_own_column(gpu_lib):
    """known=False's ranges: lo = i, hi = i + 1 over the batch's p column"""
    N, R, k, B = 40, 33, 8, 37
    eng, ent, rel = make_engine("ComplEx", k, N, R, scale=0.6)
    X, _ = pair_case(B, N, R, seed=9)
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ns = torch.full((B * R,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    rows = torch.arange(B + 1, dtype=torch.int64, device="cuda")
    Xd = dev(X)
    eng.train_relation_fwdbwd(Xd, loss_desc("multiclass_nll"), 1.0, flt=(rows[:B], rows[1:], Xd[:, 1].contiguous()), stats=stats, rel_scores=ns)
    torch.cuda.synchronize()
    want = np.zeros((B, R), dtype=bool)
    want[np.arange(B), X[:, 1]] = True
    assert np.array_equal(np.isneginf(ns.cpu().numpy().reshape(R, B).T), want) and stats.cpu().tolist() == [B, 0]
    got = (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel), O.compute_scores("ComplEx", *O.lookup(ent, rel, X)), ns.cpu().numpy())
    check_against_step("ComplEx", ent, rel, X, want, got, "multiclass_nll", "sum", 1.0)


def test_weight_zero_touches_nothing(gpu_lib):
    N, R, k, B = 40, 33, 8, 37
    eng, ent, rel = make_engine("ComplEx", k, N, R, scale=0.6)
    X, known = pair_case(B, N, R, seed=10)
    eng.prepare_training("adam")
    rng = np.random.default_rng(0)
    eng.g_flat.copy_(torch.as_tensor(rng.normal(size=eng.g_flat.shape).astype(np.float32)))
    eng.loss_acc.copy_(torch.as_tensor([1.5, 2.5, 3.5], dtype=torch.float64))
    g0, l0 = eng.g_flat.clone(), eng.loss_acc.clone()
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * R,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.full((2,), 3, dtype=torch.int64, device="cuda")
    eng.train_relation_fwdbwd(dev(X), loss_desc("multiclass_nll"), 0.0, flt=tuple(dev(a) for a in RR.csr(known)), stats=stats, pos_scores=ps, rel_scores=ns)
    torch.cuda.synchronize()
    assert torch.equal(eng.g_flat.view(torch.int32), g0.view(torch.int32)) and torch.equal(eng.loss_acc, l0)
    assert stats.cpu().tolist() == [3, 3] and (ps == 7.0).all() and (ns == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------ 4. the chunk seam
def test_step_across_the_score_chunk(gpu_lib):
    """B * R = 70 000 * 240 > 2^24: rows 0 .. 69 904 are the first chunk (2^24 // 240 rows), the rest the second, whose mask must be
    taken from ITS rows' ranges.  The reference is the step's matrix form in fp64 (DistMult: score = <s * o, rel[j]>), the loss by the
    oracle: the override rows of 17 M corruptions would cost minutes."""
    model, N, R, k, B = "DistMult", 50, 240, 7, 70000
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    rng = np.random.default_rng(11)
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
    seam = (1 << 24) // R
    assert 0 < seam < B
    # per-row ranges that do not repeat with the chunk: row i knows its own relation and (i * 7 + 3) % R
    other = (np.arange(B) * 7 + 3) % R
    known = [np.unique(np.array([p, q], dtype=np.int32)) for p, q in zip(X[:, 1], other)]
    mask = np.zeros((B, R), dtype=bool)
    mask[np.arange(B), X[:, 1]] = True
    mask[np.arange(B), other] = True
    assert not np.array_equal(mask[seam:seam + 64], mask[:64])
    w = 0.25
    (L, Ge, Gr, ps, ns), stats = run_step(eng, X, "multiclass_nll", "mean", w, known)
    S_got = ns.reshape(R, B).T
    assert np.array_equal(np.isneginf(S_got), mask) and stats == [int(mask.sum()), 0]
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    Q = RR.pair_queries(model, ent, X, k)
    S = Q @ r64.T
    S[mask] = -np.inf
    sp = (Q * r64[X[:, 1]]).sum(1)
    with np.errstate(invalid="ignore"):
        total, per, dP, dN = O.loss_and_grads("multiclass_nll", sp.astype(np.float32), S.T.reshape(-1).astype(np.float32), R, None, "mean")
    live = ~mask
    assert np.allclose(S_got[live], S[live], rtol=1e-5, atol=1e-5 * np.abs(S[live]).max())
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    want = w * float(per.astype(np.float64).sum())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    Cn = w * dN.reshape(R, B).T.astype(np.float64)
    cp = w * dP.astype(np.float64)[:, None]
    t = Cn @ r64 + cp * r64[X[:, 1]]                         # dL/dq
    Te, Tr = np.zeros_like(e64), Cn.T @ Q
    np.add.at(Te, X[:, 0], t * e64[X[:, 2]])
    np.add.at(Te, X[:, 2], t * e64[X[:, 0]])
    np.add.at(Tr, X[:, 1], cp * Q)
    print(f"chunked: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, masked {stats[0]}")
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


# ------------------------------------------------------------------------------------------------------------------ 5. NaN / inf
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("plant", ["rel_nan_row", "ent_inf_unit"])
def test_nonfinite_sets(gpu_lib, model, plant):
    """One NaN relation row / one inf in an entity row: the set of non-finite floats in loss, scores and both gradient tables equals
    the restatement's accumulated in float32, and the sets include/amdkge_relation_objective.h states."""
    from ampligraph_amd.engine import KgeEngine

    N, R, k, B = 40, 5, 8, 37
    rng = np.random.default_rng(12)
    K = O.internal_k(model, k)
    ent, rel = (rng.normal(size=(N, K)) * 0.3).astype(np.float32), (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    X, known = pair_case(B, N, R, seed=13)
    bad_e = int(X[0, 0])
    if plant == "rel_nan_row":
        rel[2, :] = np.nan
    else:
        ent[bad_e, 5] = np.inf
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    mask, masked, unmaskable = RR.mask_matrix(B, R, known)
    holders = (X[:, 0] == bad_e) | (X[:, 2] == bad_e)
    for loss in LOSSES:
        (L, Ge, Gr, ps, ns), stats = run_step(eng, X, loss, "sum", 0.25, known)
        wL, Te, Tr, sp, sn = RR.relation_step(model, ent, rel, X, mask, loss, "sum", 0.25, finite=False, dtype=np.float32)
        assert stats == [masked, unmaskable]
        # (the restatement's loss is fp64 arithmetic on fp32 scores: where fp32 underflows e^-75 / Z to 0 -- a positive at -inf next to
        # relations at +inf -- the kernel's -log is +inf and the restatement's a finite 150-odd; NaN is NaN in both)
        assert np.isnan(L) == np.isnan(wL) and (np.isfinite(L) == np.isfinite(wL) or (L == np.inf and "inf" in plant)), (loss, L, wL)
        assert np.array_equal(np.isnan(ns), np.isnan(sn)) and np.array_equal(np.isposinf(ns), np.isposinf(sn)) and np.array_equal(np.isneginf(ns), np.isneginf(sn))
        assert np.array_equal(~np.isfinite(Ge), ~np.isfinite(Te)), (loss, np.argwhere(~np.isfinite(Ge) != ~np.isfinite(Te))[:5])
        assert np.array_equal(~np.isfinite(Gr), ~np.isfinite(Tr)), (loss, np.argwhere(~np.isfinite(Gr) != ~np.isfinite(Tr))[:5])
        S = ns.reshape(R, B).T
        if plant == "rel_nan_row":   # every positive is scored against the row: every loss, and every positive's s / o gradient rows
            assert np.isnan(L) and np.isnan(S[:, 2][~mask[:, 2]]).all()
            used = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
            assert (~np.isfinite(Ge[used])).all(1).all() and np.isfinite(Ge[np.setdiff1d(np.arange(N), used)]).all()
        else:                        # the positives that hold the entity; every relation gradient row; no entity row of another positive
            assert not np.isfinite(S[holders][~mask[holders]]).all() and np.isfinite(S[~holders][~mask[~holders]]).all()
            assert (~np.isfinite(Gr)).any(1).all()
            touched = np.unique(np.concatenate([X[holders, 0], X[holders, 2]]))
            assert np.isfinite(Ge[np.setdiff1d(np.arange(N), touched)]).all()


# ------------------------------------------------------------------------------------------------------------------ 6. through fit()
def _written_out(m2, X, bs, epochs, term, main):
    """the same steps through the engine: main(eng, loop, batch, step) -> relation term -> batch regulariser -> sweep"""
    from ampligraph_amd.datasets.filters import PairFilterIndex

    eng, loop = m2._engine, m2._loop
    Xi = m2.data_indexer.get_indexes(X).astype(np.int32)
    index = PairFilterIndex([Xi], int(m2._n_ents), int(m2._n_rels))
    lo, hi = index.relation_ranges(Xi)
    known_all = [index.r_ids[a:b] for a, b in zip(lo, hi)]
    steps = -(-len(Xi) // bs)
    hist, masked_total = [], 0
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    R = int(m2._n_rels)
    for epoch in range(epochs):
        loop.reset_loss()
        for step in range(steps):
            rows = slice(step * bs, min((step + 1) * bs, len(Xi)))
            batch = dev(Xi[rows])
            main(eng, loop, batch, epoch * steps + step)
            known = known_all[rows]
            eng.train_relation_fwdbwd(batch, term.loss.to_ffi(), term.weight, flt=tuple(dev(a) for a in RR.csr(known)), stats=stats)
            lam, lam_r = loop.reg, loop.reg if isinstance(loop.reg_rel, str) else loop.reg_rel
            breg_e, breg_r = (r if getattr(r, "batch", False) else None for r in (lam, lam_r))
            if breg_e is not None or breg_r is not None:
                eng.batch_reg_fwdbwd(batch, breg_e, breg_r)
            loop.optimizer.iterations += 1
            eng.opt_step(loop.optimizer.to_ffi(loop.optimizer.iterations, 2), None if breg_e is not None else lam, None if breg_r is not None else lam_r)
            loop.n_steps += 1
            masked_total += RR.mask_matrix(int(batch.shape[0]), R, known)[1]
        hist.append(loop.mean_batch_loss())
    return hist, masked_total, stats.cpu().tolist()


@pytest.mark.parametrize("path", ["shared_all", "per_corruption"])
def test_fit_with_the_term_equals_the_steps_written_out(gpu_lib, path):
    from test_gpu_model import toy_graph

    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.latent_features import RelationPrediction, ScoringBasedEmbeddingModel, optimizers
    from test_gpu_shared_mask import filters

    X = toy_graph(seed=4, n=400, N=40, R=3)
    bs, epochs = 128, 3
    term = RelationPrediction(weight=0.25)
    if path == "shared_all":
        scoring, kw, reg = "ComplEx", dict(negatives={"shared": "all", "mask_known": True}), "N3"
    else:
        scoring, kw, reg = "DistMult", {}, "l2"

    def new(**extra):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type=scoring, seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", entity_relation_regularizer=reg, **kw, **extra)
        return m

    m1 = new(relation_prediction=term)
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    m2 = new()
    m2.fit(X, batch_size=bs, epochs=0, verbose=False)
    N = int(m2._n_ents)
    Xi = m2.data_indexer.get_indexes(X).astype(np.int32)
    fs, fo = FilterIndex([Xi], N, int(m2._n_rels)).as_lists(Xi)
    row_of = {}

    def main(eng, loop, batch, step):
        if path == "shared_all":
            B = int(batch.shape[0])
            G = m1._loop.negatives.group_size
            _, side = eng.sample_shared(batch, G, 1, loop.seed, step)
            ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(-(-B // min(G, B)), 1)
            r0 = (step % (-(-len(Xi) // bs))) * bs
            sf, of = filters(fs[r0:r0 + B], fo[r0:r0 + B])
            eng.train_shared_masked_fwdbwd(batch, G, N, ids, side, loop.loss_ffi, s_filter=sf, o_filter=of, identity=True)
        else:
            eng.train_fwdbwd(batch, loop.eta, loop.loss_ffi, loop.seed, step, row_offset=0, b_global=int(batch.shape[0]))

    hist, masked_total, stats = _written_out(m2, X, bs, epochs, term, main)
    print(path, "loss histories", h1.history["loss"], hist, "stats", m1.relation_prediction_stats_, masked_total)
    assert len(h1.history["loss"]) == epochs and np.allclose(h1.history["loss"], hist, rtol=2e-4)
    assert m1.relation_prediction_stats_ == {"masked": masked_total, "unmaskable": stats[1]} and stats[0] == masked_total
    assert masked_total >= epochs * len(Xi)
    # the term did something: the run without it has another history
    h3 = new().fit(X, batch_size=bs, epochs=epochs, verbose=False)
    assert not np.allclose(h1.history["loss"], h3.history["loss"], rtol=2e-4)


def test_none_is_the_model_compiled_without_the_keyword(gpu_lib):
    """bit-identical histories: in deterministic mode, the one in which two runs of ONE configuration are bit-identical at all (the
    default step adds relation gradients with atomics in arrival order)"""
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = toy_graph(seed=4, n=400, N=40, R=3)
    hs = []
    for kw in ({}, {"relation_prediction": None}):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", deterministic=True, **kw)
        hs.append(m.fit(X, batch_size=128, epochs=3, verbose=False).history["loss"])
        assert m._loop.relation is None and not hasattr(m, "relation_prediction_stats_") and "relation_prediction" not in m.get_config()
    assert hs[0] == hs[1]


# ------------------------------------------------------------------------------------------------------------------ 7. a planted graph
def test_planted_graph_trains_saves_and_restores(gpu_lib, tmp_path):
    from planted import planted_kg

    from ampligraph_amd.evaluation import mrr_score
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.utils import restore_model, save_model

    kg = planted_kg("ComplEx", n_ents=120, n_rels=4, n_test=50, seed=0)
    train, test = kg["train"].astype(str), kg["test"].astype(str)

    def new(**kw):
        m = ScoringBasedEmbeddingModel(eta=5, k=16, scoring_type="ComplEx", seed=0)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", **kw)
        return m

    mrr = {}
    for name, kw in (("with", {"relation_prediction": {"weight": 0.5, "known": True}}), ("without", {})):
        m = new(**kw)
        h = m.fit(train, batch_size=256, epochs=8, verbose=False).history["loss"]
        assert np.isfinite(h).all() and h[-1] < h[0], h
        mrr[name] = float(mrr_score(m.evaluate_relations(test, use_filter={"train": train, "test": test})))
        if name == "with":
            kept, hist = m, h
    print("evaluate_relations MRR on the test split: with the term", mrr["with"], "without", mrr["without"])
    assert np.isfinite(mrr["with"]) and np.isfinite(mrr["without"])
    assert kept.relation_prediction_stats_["masked"] >= 8 * len(train)
    save_model(kept, str(tmp_path / "m"))
    back = restore_model(str(tmp_path / "m"))
    assert back.get_config() == kept.get_config() and back._relation_prediction.weight == 0.5
    assert np.array_equal(back.predict(test), kept.predict(test))
    h2 = back.fit(train, batch_size=256, epochs=1, verbose=False).history["loss"]                # a continued epoch takes the term again
    assert back._loop.relation is not None and back.relation_prediction_stats_["masked"] >= len(train) and np.isfinite(h2).all()
