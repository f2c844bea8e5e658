"""Masked shared-negative training on the GPU (shared_mask_kernel in kge_train_shared.hip, include/amdkge_shared_mask.h): the mask
kernel against its numpy restatement (tests/shared_mask_ref.py: the set of -inf positions, every other entry bit-untouched, both
counts), the masked forward / backward against the oracle on the equivalent override rows with those scores at -inf, the chunked
score buffer, the equivalences with the unmasked step, and fit() with mask_known / num_negs="all"."""
import numpy as np
import pytest
import torch

import shared_mask_ref as MR
import shared_ref as SR
from oracle import kge_oracle as O
from test_gpu_kernels import assert_grads_close, dense, dev, loss_desc, make_engine, rand_triples
from test_gpu_shared import SHARED_MODELS, grad_gap, run_shared

pytestmark = pytest.mark.gpu

LOSSES = list(O.LOSS_DEFAULTS)


def dense_graph(seed, n, N, R):
    return rand_triples(np.random.default_rng(seed), n, N, R)


def filters(ks, ko):
    """per-row known lists -> (s_filter, o_filter) device triples, FilterIndex.device_filter's form"""
    return tuple(tuple(dev(a) for a in MR.csr(k)) for k in (ks, ko))


def run_mask(eng, S0, row0, G, ids, side, ks, ko, identity=False):
    """-> (the buffer after amdkge_shared_mask_scores, [masked, unmaskable])"""
    S = dev(S0)
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    sf, of = filters(ks, ko)
    eng.shared_mask_scores(S, row0, G, None if ids is None else dev(ids), dev(side), sf, of, identity=identity, stats=stats)
    torch.cuda.synchronize()
    return S.cpu().numpy(), stats.cpu().tolist()


def check_mask(got, S0, mask, want_stats):
    S, stats = got
    assert np.array_equal(np.isneginf(S), mask)                                           # the set of -inf positions
    assert np.array_equal(S[~mask].view(np.uint32), S0[~mask].view(np.uint32))             # every other entry bit-untouched
    assert stats == list(want_stats)                                                      # both counts


def mask_case(B, G, M, N, kind="", seed=0):
    """-> (X, ids, side, known_s, known_o): a batch cut from a graph dense enough that most ranges hold several ids"""
    R = 2
    rng = np.random.default_rng(seed)
    D = dense_graph(seed + 1, max(6 * N, 4), max(N, 1), R)
    X = D[rng.integers(0, len(D), B)] if N > 1 else np.zeros((B, 3), np.int32)
    if N == 1:
        D = X
    ids, side = SR.sample_shared(X, G, M, 3, 4, sample_range=N)
    ks, ko = MR.known_lists(X, [D], N, R)
    if kind == "empty":                                                                   # rows whose key no dataset holds
        for i in (0, B // 2, B - 1):
            ks[i], ko[i] = ks[i][:0], ko[i][:0]
    return X, ids, side, ks, ko


@pytest.fixture(scope="module")
def mask_engine(gpu_lib):
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("DistMult", 4, 64, 2)


# ------------------------------------------------------------------------------------------------------------------ 1. the mask kernel
@pytest.mark.parametrize("B,G,M,N,kind", [(1, 1, 1, 1, "fully known"), (37, 8, 5, 10, ""), (37, 8, 63, 40, ""), (37, 8, 64, 40, ""), (37, 8, 65, 40, ""),
                                          (301, 64, 130, 50, "short last group"), (37, 8, 20, 6, "repeated ids"), (37, 8, 33, 40, "empty"),
                                          (37, 8, 3, 40, "range longer than M")])
def test_mask_kernel_given(mask_engine, B, G, M, N, kind):
    X, ids, side, ks, ko = mask_case(B, G, M, N, kind)
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids, side, ks, ko)
    S0 = np.random.default_rng(9).normal(size=(B, M)).astype(np.float32)
    print(f"B={B} G={G} M={M} N={N} {kind}: masked {masked} of {B * M}, unmaskable {unmaskable}, longest range {max(len(a) for a in ks + ko)}")
    if kind == "fully known":
        assert (masked, unmaskable) == (0, 1)
    elif kind == "repeated ids":
        assert all(len(set(r.tolist())) < M for r in ids) and masked > 0
    elif kind == "range longer than M":
        assert max(len(a) for a in ks + ko) > M and masked > 0
    elif kind == "empty":
        assert not mask[0].any() and not mask[B - 1].any() and masked > 0
    else:
        assert 0 < masked < B * M
    check_mask(run_mask(mask_engine, S0, 0, G, ids, side, ks, ko), S0, mask, (masked, unmaskable))


def test_mask_kernel_fully_known_rows_among_others(mask_engine):
    """N = 3, dense: several rows are fully known (left untouched, counted), their neighbours in the same group are masked"""
    X, ids, side, ks, ko = mask_case(37, 8, 4, 3, seed=2)
    mask, masked, unmaskable = MR.mask_matrix(X, 8, ids, side, ks, ko)
    assert unmaskable > 0 and masked > 0
    S0 = np.random.default_rng(9).normal(size=(37, 4)).astype(np.float32)
    check_mask(run_mask(mask_engine, S0, 0, 8, ids, side, ks, ko), S0, mask, (masked, unmaskable))


@pytest.mark.parametrize("B,G,M,N", [(37, 8, 23, 23), (37, 8, 15, 23), (37, 8, 3, 23), (301, 64, 130, 130)])
def test_mask_kernel_identity(mask_engine, B, G, M, N):
    """ids[g][j] == j.  M < N: the range ids >= M are ignored (M = 3: some rows are then fully known).  IDENTITY == GIVEN on the
    arange list, bit for bit."""
    X, _, side, ks, ko = mask_case(B, G, M, N, seed=3)
    ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids, side, ks, ko)
    assert masked > 0 and (M >= N or max(max(a) for a in ks + ko if len(a)) >= M)
    S0 = np.random.default_rng(9).normal(size=(B, M)).astype(np.float32)
    got_i = run_mask(mask_engine, S0, 0, G, None, side, ks, ko, identity=True)
    check_mask(got_i, S0, mask, (masked, unmaskable))
    got_g = run_mask(mask_engine, S0, 0, G, ids, side, ks, ko)
    assert np.array_equal(got_i[0].view(np.uint32), got_g[0].view(np.uint32)) and got_i[1] == got_g[1]


@pytest.mark.parametrize("identity", [False, True])
def test_mask_kernel_window(mask_engine, identity):
    """row0 != 0: the buffer is rows [13, 30) of a batch of 37 -- the window starts and ends inside a group"""
    B, G, M, N, row0, rows = 37, 8, 33, 40, 13, 17
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=4)
    if identity:
        ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
    full, _, _ = MR.mask_matrix(X, G, ids, side, ks, ko)
    mask = full[row0:row0 + rows]
    assert mask.any() and not np.array_equal(mask, full[:rows])
    S0 = np.random.default_rng(9).normal(size=(rows, M)).astype(np.float32)
    check_mask(run_mask(mask_engine, S0, row0, G, None if identity else ids, side, ks, ko, identity=identity), S0, mask, (int(mask.sum()), 0))


# ------------------------------------------------------------------------------------------------------------------ 2. forward / backward
def run_masked(eng, X, G, ids, side, loss_name, reduction, ks, ko, identity=False):
    """-> ((loss sum, dense entity gradient, dense relation gradient, positive scores, corruption scores [M * B]), [masked, unmaskable])"""
    B, M = X.shape[0], ids.shape[1]
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * M,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    sf, of = filters(ks, ko) if ks is not None else (None, None)
    eng.train_shared_masked_fwdbwd(dev(X), G, M, dev(ids), dev(side), loss_desc(loss_name, reduction), s_filter=sf, o_filter=of, identity=identity, stats=stats,
                                   pos_scores=ps, neg_scores=ns)
    torch.cuda.synchronize()
    return (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel), ps.cpu().numpy(), ns.cpu().numpy()), stats.cpu().tolist()


def check_against_masked_step(model, ent, rel, X, G, ids, side, mask, got, loss, reduction, R, tag=""):
    """test_gpu_shared.py::check_against_oracle's figures, on the live scores; the masked ones are -inf"""
    L, Ge, Gr, ps, ns = got
    want, Te, Tr, sp, sn = MR.masked_step(model, ent, rel, X, G, ids, side, mask, loss, reduction, R)
    live = np.isfinite(sn)
    print(f"{tag} {model} {loss} {reduction}: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, "
          f"score gap {np.abs(ns[live] - sn[live]).max() / np.abs(sn[live]).max():.3g}, masked {int((~live).sum())}")
    assert np.array_equal(np.isneginf(ns), ~live) and np.array_equal(~live, mask.T.reshape(-1))
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns[live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


@pytest.mark.parametrize("model", SHARED_MODELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_masked_fwdbwd_parity(gpu_lib, model, loss):
    """B = 37 in groups of 8 (a last group of 5), M = 33 crosses the 32-wide MFMA tile; both reductions"""
    N, R, k, B, G, M = 40, 2, 8, 37, 8, 33
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=5)
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids, side, ks, ko)
    assert masked > B and unmaskable == 0 and 0 < side.sum() < B
    for reduction in ("sum", "mean"):
        got, stats = run_masked(eng, X, G, ids, side, loss, reduction, ks, ko)
        check_against_masked_step(model, ent, rel, X, G, ids, side, mask, got, loss, reduction, R)
        assert stats == [masked, unmaskable]


def test_masked_fwdbwd_identity_list(gpu_lib):
    """the all-entities step: ids[g][j] = j, M = N, the mask in IDENTITY mode; == the same call in GIVEN mode"""
    N, R, k, B, G = 40, 2, 8, 37, 8
    eng, ent, rel = make_engine("ComplEx", k, N, R, scale=0.6)
    X, _, side, ks, ko = mask_case(B, G, N, N, seed=6)
    ids = np.tile(np.arange(N, dtype=np.int32), (SR.n_groups(B, G), 1))
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids, side, ks, ko)
    got, stats = run_masked(eng, X, G, ids, side, "multiclass_nll", "mean", ks, ko, identity=True)
    check_against_masked_step("ComplEx", ent, rel, X, G, ids, side, mask, got, "multiclass_nll", "mean", R)
    assert stats == [masked, unmaskable] and mask[np.arange(B), np.where(side != 0, X[:, 0], X[:, 2])].all()   # the positive itself is masked
    got_g, stats_g = run_masked(eng, X, G, ids, side, "multiclass_nll", "mean", ks, ko)
    assert np.array_equal(got[4].view(np.uint32), got_g[4].view(np.uint32)) and stats_g == stats


# ------------------------------------------------------------------------------------------------------------------ 3. the chunked buffer
def test_masked_step_across_the_score_chunk(gpu_lib):
    """B * M = 4 200 * 4 097 > 2^24: 63 groups of 64 fill the first chunk, rows 4 032 .. 4 199 are the second, whose mask must be
    taken from ITS rows' ranges.  The reference is the step's matrix form in fp64 (DistMult: score = <q_i, e>), the loss by the
    oracle: the override rows of 17 M corruptions would cost minutes."""
    model, N, R, k, B, G, M = "DistMult", 50, 2, 7, 4200, 64, 4097
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=7)
    known = np.zeros((B, N), dtype=bool)                                                  # (mask_matrix, vectorised: ids < N)
    for i in range(B):
        known[i, ks[i] if side[i] else ko[i]] = True
    grp = np.arange(B) // G
    mask = known[np.arange(B)[:, None], ids[grp]]
    assert not mask.all(1).any() and mask[4032:].any() and not np.array_equal(mask[4032:], mask[:168])
    got, stats = run_masked(eng, X, G, ids, side, "pairwise", "mean", ks, ko)
    L, Ge, Gr, ps, ns = got
    assert np.array_equal(np.isneginf(ns.reshape(M, B).T), mask) and stats == [int(mask.sum()), 0]
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    subj = side != 0
    kept = np.where(subj[:, None], e64[X[:, 2]], e64[X[:, 0]])
    own = np.where(subj[:, None], e64[X[:, 0]], e64[X[:, 2]])
    p = r64[X[:, 1]]
    Q = p * kept
    groups = [slice(g * G, min((g + 1) * G, B)) for g in range(SR.n_groups(B, G))]
    S = np.concatenate([Q[rows] @ e64[ids[g]].T for g, rows in enumerate(groups)])         # [B, M]
    S[mask] = -np.inf
    sp = (Q * own).sum(1)
    with np.errstate(invalid="ignore"):
        total, per, dP, dN = O.loss_and_grads("pairwise", sp.astype(np.float32), S.T.reshape(-1).astype(np.float32), M, None, "mean")
    Cn = dN.reshape(M, B).T.astype(np.float64)
    live = ~mask
    assert np.allclose(ns.reshape(M, B).T[live], S[live], rtol=1e-5, atol=1e-5 * np.abs(S[live]).max())
    want = float(per.astype(np.float64).sum())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    t = np.concatenate([Cn[rows] @ e64[ids[g]] for g, rows in enumerate(groups)]) + dP[:, None] * own   # dL/dq
    Te, Tr = np.zeros_like(e64), np.zeros_like(r64)
    np.add.at(Te, np.where(subj, X[:, 0], X[:, 2]), dP[:, None] * Q)
    np.add.at(Te, np.where(subj, X[:, 2], X[:, 0]), t * p)
    np.add.at(Tr, X[:, 1], t * kept)
    for g, rows in enumerate(groups):
        np.add.at(Te, ids[g], Cn[rows].T @ Q[rows])
    print(f"chunked: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, masked {stats[0]}")
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


# ------------------------------------------------------------------------------------------------------------------ 4. equivalences, edges
@pytest.mark.parametrize("model", SHARED_MODELS)
def test_empty_ranges_are_the_unmasked_step(gpu_lib, model):
    """every range empty -> amdkge_train_shared_fwdbwd: scores bit for bit, loss and gradients (fp32 atomics in arrival order on both
    sides) within the bars of test_gpu_shared.py's item 5; and so is the call without ranges"""
    N, R, k, B, G, M = 40, 2, 8, 37, 8, 33
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=8)
    none = [a[:0] for a in ks]
    L0, Ge0, Gr0, ps0, ns0 = run_shared(eng, X, G, ids, side, "self_adversarial", "mean")
    for kw in (dict(ks=none, ko=none), dict(ks=None, ko=None)):
        (L, Ge, Gr, ps, ns), stats = run_masked(eng, X, G, ids, side, "self_adversarial", "mean", **kw)
        assert np.array_equal(ns.view(np.uint32), ns0.view(np.uint32)) and np.array_equal(ps.view(np.uint32), ps0.view(np.uint32)) and stats == [0, 0]
        assert grad_gap(Ge, Ge0) <= 2e-5 and grad_gap(Gr, Gr0) <= 2e-5 and abs(L - L0) <= 1e-5 * max(1.0, abs(L0))


def test_self_adversarial_with_a_fully_known_list(gpu_lib):
    """one positive whose whole list is known: its row stays unmasked (no -inf - (-inf)), the loss is finite, stats[1] == 1"""
    N, R, k, B, G, M = 40, 2, 8, 37, 8, 6
    eng, ent, rel = make_engine("ComplEx", k, N, R, scale=0.6)
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=9)
    i = 11
    full = np.unique(ids[i // G]).astype(np.int32)
    ks[i], ko[i] = full, full
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids, side, ks, ko)
    assert unmaskable == 1 and not mask[i].any() and masked > 0
    for reduction in ("sum", "mean"):
        got, stats = run_masked(eng, X, G, ids, side, "self_adversarial", reduction, ks, ko)
        assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all() and stats == [masked, 1]
        assert np.isfinite(got[4].reshape(M, B)[:, i]).all()
        check_against_masked_step("ComplEx", ent, rel, X, G, ids, side, mask, got, "self_adversarial", reduction, R)


# ------------------------------------------------------------------------------------------------------------------ 5. through fit()
@pytest.mark.parametrize("spec", ["all", "sampled"])
def test_fit_with_masked_shared_negatives_equals_the_steps_written_out(gpu_lib, spec):
    from test_gpu_model import toy_graph

    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.latent_features.negatives import BoundMaskedSharedNegatives, SharedNegatives

    X = toy_graph(seed=4, n=400, N=40, R=3)
    bs, epochs = 128, 3
    extra = {} if spec == "all" else {"valid": X[:50]}                      # (statements of the training set: known twice)
    negatives = {"shared": "all", "mask_known": True} if spec == "all" else {"shared": 48, "group_size": 20, "mask_known": extra}

    def new(**kw):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", entity_relation_regularizer="l2", **kw)
        return m

    m1 = new(negatives=negatives)
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    b = m1._loop.negatives
    assert isinstance(b, BoundMaskedSharedNegatives) and b.identity == (spec == "all")
    N = int(m1._n_ents)
    G, M = (b.group_size, N) if spec == "all" else (20, 48)
    assert b.num_negs == M and (spec != "all" or G == SharedNegatives.ALL_GROUP_SIZE)

    # the same steps written out: a model built the same way (epochs=0: tables initialised, no step), then draw -> masked step -> sweep
    m2 = new()
    m2.fit(X, batch_size=bs, epochs=0, verbose=False)
    eng, loop = m2._engine, m2._loop
    Xi = m2.data_indexer.get_indexes(X).astype(np.int32)
    assert np.array_equal(Xi, m1.data_indexer.get_indexes(X))
    index = FilterIndex([Xi] + [m2.data_indexer.get_indexes(v) for v in extra.values()], N, int(m2._n_rels))
    fs, fo = index.as_lists(Xi)
    steps = -(-len(Xi) // bs)
    hist, masked_total = [], 0
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    for epoch in range(epochs):
        loop.reset_loss()
        for step in range(steps):
            rows = slice(step * bs, min((step + 1) * bs, len(Xi)))
            batch = dev(Xi[rows])
            B = int(batch.shape[0])
            ids, side = eng.sample_shared(batch, G, 1 if spec == "all" else M, loop.seed, epoch * steps + step)
            if spec == "all":
                ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(SR.n_groups(B, G), 1)
            ks, ko = fs[rows], fo[rows]
            sf, of = filters(ks, ko)
            eng.train_shared_masked_fwdbwd(batch, G, M, ids, side, loop.loss_ffi, s_filter=sf, o_filter=of, identity=spec == "all", stats=stats)
            loop.optimizer.iterations += 1
            eng.opt_step(loop.optimizer.to_ffi(loop.optimizer.iterations, 2), loop.reg, loop.reg if isinstance(loop.reg_rel, str) else loop.reg_rel)
            loop.n_steps += 1
            masked_total += MR.mask_matrix(Xi[rows], G, ids.cpu().numpy(), side.cpu().numpy(), ks, ko)[1]
        hist.append(loop.mean_batch_loss())
    print("loss histories", h1.history["loss"], hist, "masked", m1.negative_sampling_stats_, masked_total)
    assert len(h1.history["loss"]) == epochs and np.allclose(h1.history["loss"], hist, rtol=2e-4)
    assert m1.negative_sampling_stats_ == {"masked": masked_total, "unmaskable": 0} and stats.cpu().tolist() == [masked_total, 0]
    assert masked_total >= (epochs * len(Xi) if spec == "all" else 1)        # the all-entities list holds every positive's own entity
    # the setting did something: the unmasked run has another history, and no stats
    m3 = new(negatives={k: v for k, v in negatives.items() if k != "mask_known"})
    h3 = m3.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    assert not np.allclose(h1.history["loss"], h3.history["loss"], rtol=2e-4) and not hasattr(m3, "negative_sampling_stats_")
    assert not hasattr(m3._loop.negatives, "mask") and np.isfinite(h3.history["loss"]).all()


def test_all_with_a_pool_and_what_bind_refuses(gpu_lib):
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = toy_graph(seed=4, n=400, N=40, R=3)
    ents = np.unique(np.concatenate([X[:, 0], X[:, 2]]))

    def new(**kw):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", **kw)
        return m

    pool = ents[[7, 3, 3, 11, 0, 5]]                                        # an order of its own, one label twice
    m = new(negatives={"shared": "all", "entities": pool, "mask_known": True, "side": "bernoulli"})
    m.fit(X, batch_size=128, epochs=1, verbose=False)
    b = m._loop.negatives
    assert b.num_negs == 6 and not b.identity
    batch = torch.as_tensor(m.data_indexer.get_indexes(X[:128]).astype(np.int32)).cuda()
    ids, side = b.draw(batch, m.seed, 0)
    assert ids.shape == (1, 6) and ids.cpu().numpy()[0].tolist() == m.data_indexer.get_indexes(pool, "e").tolist()
    assert np.isfinite(m.history.history["loss"]).all() and set(m.negative_sampling_stats_) == {"masked", "unmaskable"}
    with pytest.raises(ValueError, match="not a row slice"):
        b.mask(batch)                                                       # (a copy, not a slice of the bound tensor)
    with pytest.raises(ValueError, match="not in the training set"):
        new(negatives={"shared": "all", "entities": ["no such entity"]}).fit(X, batch_size=128, epochs=1, verbose=False)
    Xf = np.concatenate([X, np.ones((len(X), 1))], 1)
    with pytest.raises(NotImplementedError, match="FocusE"):
        new(negatives={"shared": "all", "mask_known": True}).fit(Xf, batch_size=128, epochs=1, verbose=False, focusE=True)
