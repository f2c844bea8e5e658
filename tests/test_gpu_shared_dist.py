"""Shared negatives for TransE and RotatE on the GPU (kge_train_shared_dist.hip, include/amdkge_shared_dist.h): the distance tiles'
forward / backward against the oracle on the EQUIVALENT override rows (tests/shared_ref.py: override_rows is the step's definition),
against the header's arithmetic restated in numpy (tests/shared_dist_ref.py), against the fused per-corruption kernel on the same
rows, the masked step, whole steps through fit().

A precondition on the inputs, not a tolerance: against the fp64 oracle a TransE residual within rounding of zero flips a sign and a
RotatE modulus near zero is ill-conditioned, so every oracle comparison first asserts, in fp64 on the CPU, |d| > 1e-6 (TransE) /
|z| > 1e-3 (RotatE) on every scored pair-unit; the seeds below were chosen so that it holds."""
import numpy as np
import pytest
import torch

import shared_dist_ref as DR
import shared_mask_ref as MR
import shared_ref as SR
from margins import within
from oracle import kge_oracle as O
from test_gpu_kernels import assert_grads_close, dense, dev, loss_desc, make_engine, make_optimizer, rand_triples, run_fwdbwd
from test_gpu_shared import check_against_oracle, grad_gap
from test_gpu_shared_mask import filters

pytestmark = pytest.mark.gpu

DIST_MODELS = ("TransE", "RotatE")
LOSSES = list(O.LOSS_DEFAULTS)
MIN_UNIT = {"TransE": 1e-6, "RotatE": 1e-3}


def min_unit_fp64(model, ent, rel, X, negs, R):
    """the smallest |s + p - o| (TransE) / |s o r - o| (RotatE) over every unit of the positives and the override rows, in fp64"""
    rows = np.concatenate([np.asarray(X, dtype=np.int64), np.asarray(negs, dtype=np.int64)])
    s, p, o = (a.astype(np.float64) for a in O.lookup(ent, rel, rows))
    if model == "TransE":
        return float(np.abs(s + p - o).min())
    k = ent.shape[1] // 2
    phi = (rel[rows[:, 1], :k] / O.rotate_phase_divisor(k, R)).astype(np.float32).astype(np.float64)
    c, sn = np.cos(phi), np.sin(phi)
    re = s[:, :k] * c - s[:, k:] * sn - o[:, :k]
    im = s[:, :k] * sn + s[:, k:] * c - o[:, k:]
    return float(np.sqrt(re * re + im * im).min())


def assert_conditioned(model, ent, rel, X, G, ids, side, R):
    got = min_unit_fp64(model, ent, rel, X, SR.override_rows(X, G, ids, side), R)
    assert got > MIN_UNIT[model], (model, got)


def assert_softmax_conditioned(model, ent, rel, X, G, ids, side, R, min_x=0.05):
    """multiclass_nll's coefficient of the positive is formed in fp32 as -1 + eP / Z (kge_loss.h, every train path's; Z = sum eN / red
    + eP): with x = (sum eN / M) / eP -- the "mean" form, the smaller of the two -- it is -x / (1 + x) carrying the absolute rounding
    of a value next to 1, 6e-8, a RELATIVE error of 6e-8 (1 + x) / x.  A positive that dominates its list (x -> 0) is ill-conditioned
    in fp32 whatever scores the step is given; x > 0.05 keeps that error at 1.3e-6, an order below the gradient bar.  Asserted in
    fp64 on the header's arithmetic; the tables of the tests that compare multiclass_nll gradients are scaled so that it holds."""
    st = DR.DistStep(model, ent, rel, X, G, ids, side, R)
    x = np.exp(st.neg_matrix).sum(1) / st.M / np.exp(st.pos_scores)
    assert x.min() > min_x, (model, float(x.min()))


def case(seed, B, G, M, N, R):
    """-> (X, ids, side): both sides in the batch, the table's last and first row in the first list"""
    X = rand_triples(np.random.default_rng(seed), B, N, R)
    ids, side = SR.sample_shared(X, G, M, seed, 4, sample_range=N)
    ids[0, 0] = N - 1
    ids[0, M // 2] = 0
    assert B < 2 or 0 < side.sum() < B
    return X, ids, side


def run_dist(eng, X, G, ids, side, loss_name, reduction, ks=None, ko=None, identity=False):
    """-> ((loss sum, dense entity gradient, dense relation gradient, positive scores, corruption scores [M * B]), [masked, unmaskable])"""
    B, M = X.shape[0], ids.shape[1]
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * M,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    sf, of = filters(ks, ko) if ks is not None else (None, None)
    eng.train_shared_dist_fwdbwd(dev(X), G, M, dev(ids), dev(side), loss_desc(loss_name, reduction), s_filter=sf, o_filter=of, identity=identity, stats=stats,
                                 pos_scores=ps, neg_scores=ns)
    torch.cuda.synchronize()
    return (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel), ps.cpu().numpy(), ns.cpu().numpy()), stats.cpu().tolist()


def check_against_ref(model, ent, rel, X, G, ids, side, got, loss, reduction, R, mask=None, tag=""):
    """the bars of check_against_oracle, against the header's arithmetic (no precondition: the ref rounds where the kernel rounds)"""
    L, Ge, Gr, ps, ns = got
    want, Te, Tr, sp, sn = DR.DistStep(model, ent, rel, X, G, ids, side, R).step(loss, reduction, mask=mask)
    live = np.isfinite(sn)
    print(f"{tag} {model} {loss} {reduction} vs ref: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, "
          f"score gap {np.abs(ns[live] - sn[live]).max() / np.abs(sn[live]).max():.3g}")
    assert np.array_equal(np.isneginf(ns), ~live)
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns[live], sn[live], rtol=1e-5, atol=1e-5 * np.abs(sn[live]).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


# ------------------------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("model", DIST_MODELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_shared_dist_fwdbwd_parity(gpu_lib, model, loss):
    """B = 37 in groups of 8 (a last group of 5), M = 5, k = 32: the bars of test_gpu_shared.py::check_against_oracle"""
    N, R, k, B, G, M = 300, 5, 32, 37, 8, 5
    eng, ent, rel = make_engine(model, k, N, R, scale=0.2)
    assert eng.shared_dist_supported(B, G, M) and not eng.shared_supported(B, G, M)
    X, ids, side = case(3, B, G, M, N, R)
    assert_conditioned(model, ent, rel, X, G, ids, side, R)
    assert_softmax_conditioned(model, ent, rel, X, G, ids, side, R)
    for reduction in ("sum", "mean"):
        got, stats = run_dist(eng, X, G, ids, side, loss, reduction)
        check_against_oracle(model, ent, rel, X, G, ids, side, got, loss, reduction, R)
        check_against_ref(model, ent, rel, X, G, ids, side, got, loss, reduction, R)
        assert stats == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ 2. geometries
# (model, k) -> {(G, M): a seed of case() for which the precondition holds}, found on the CPU: the first that passes, counting from 1
GEOMETRY_SEEDS = {("TransE", 7): {(37, 33): 1, (37, 65): 1, (5, 33): 1, (5, 65): 1},
                  ("TransE", 200): {(37, 33): 4, (37, 65): 4, (5, 33): 3, (5, 65): 31},
                  ("RotatE", 7): {(37, 33): 1, (37, 65): 1, (5, 33): 1, (5, 65): 1},
                  ("RotatE", 50): {(37, 33): 2, (37, 65): 3, (5, 33): 2, (5, 65): 2}}


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("M", [33, 65])
@pytest.mark.parametrize("G", [37, 5])
@pytest.mark.parametrize("model,k", list(GEOMETRY_SEEDS))
def test_shared_dist_geometries(gpu_lib, model, k, G, M, pad):
    """The K tail of the unit chunks (7, 200 and 50 are no multiples of 32), padded units, a group smaller than a tile (5, the last of
    2) and one that is the whole batch (37), M = 33 inside one tile and M = 65 = a tile and one column, the list chunks of 32 of the
    backward tiles with tails of 1.  The bars of item 1, unchanged; with pad the padding floats of the gradients are exact zeros."""
    N, R, B = 200, 4, 37
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3 if k < 100 else 0.08, pad=pad)
    X, ids, side = case(GEOMETRY_SEEDS[model, k][G, M], B, G, M, N, R)
    assert_conditioned(model, ent, rel, X, G, ids, side, R)
    got, _ = run_dist(eng, X, G, ids, side, "self_adversarial", "sum")
    tag = f"G={G} M={M} pad={pad} k={k}"
    check_against_oracle(model, ent, rel, X, G, ids, side, got, "self_adversarial", "sum", R, tag=tag)
    check_against_ref(model, ent, rel, X, G, ids, side, got, "self_adversarial", "sum", R, tag=tag)
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    if pad:
        for g, n in ((eng.g_ent, N), (eng.g_rel, R)):
            stored = g.cpu().numpy().reshape(n, -1, eng.ks)
            assert eng.ks >= eng.k and not stored[:, :, eng.k:].any() and np.isfinite(stored).all()


@pytest.mark.parametrize("model", DIST_MODELS)
def test_shared_dist_one_positive_one_negative(gpu_lib, model):
    N, R, k = 130, 4, 7
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3)
    X = np.array([[5, 1, 9]], dtype=np.int32)
    ids = np.array([[N - 1]], dtype=np.int32)
    for sd in (0, 1):
        side = np.array([sd], dtype=np.int32)
        assert_conditioned(model, ent, rel, X, 1, ids, side, R)
        got, _ = run_dist(eng, X, 1, ids, side, "nll", "sum")
        check_against_oracle(model, ent, rel, X, 1, ids, side, got, "nll", "sum", R)


# ------------------------------------------------------------------------------------------------------------------ 3. duplicates
@pytest.mark.parametrize("model", DIST_MODELS)
def test_shared_dist_duplicates(gpu_lib, model):
    """one list is a single id M times, one holds positives' own entities (on both sides), one id is in two groups' lists; a repeated
    positive.  Against the header's arithmetic (an own entity as the replacement is the positive itself: a pair of the oracle's rows
    with the same residual, no ill-conditioned one), and against the oracle under the precondition."""
    N, R, k, B, G, M = 130, 4, 16, 23, 8, 12
    eng, ent, rel = make_engine(model, k, N, R, scale=0.2)
    X, ids, side = case(5, B, G, M, N, R)
    X[7] = X[6] = X[1]
    ids[1, :] = 77                                                          # one id M times
    for j, i in enumerate((16, 17, 18, 19)):                                # group 2: own entities of its positives, either side
        ids[2, 2 * j], ids[2, 2 * j + 1] = X[i, 0], X[i, 2]
    ids[0, 3] = ids[2, 9] = 77                                              # ... and the repeated id again in the two other lists
    assert_conditioned(model, ent, rel, X, G, ids, side, R)
    assert_softmax_conditioned(model, ent, rel, X, G, ids, side, R)
    for loss in ("multiclass_nll", "pairwise"):
        got, _ = run_dist(eng, X, G, ids, side, loss, "mean")
        check_against_ref(model, ent, rel, X, G, ids, side, got, loss, "mean", R)
        check_against_oracle(model, ent, rel, X, G, ids, side, got, loss, "mean", R)


# ------------------------------------------------------------------------------------------------------------------ 4. two formulations
@pytest.mark.parametrize("model,k", [("TransE", 48), ("RotatE", 36)])
def test_shared_dist_equals_the_fused_kernel_on_the_override_rows(gpu_lib, model, k):
    """The same step through amdkge_train_fwdbwd(d_neg_override = the equivalent rows): the bars of
    test_gpu_shared.py::test_shared_equals_the_fused_kernel_on_the_override_rows.  (The fused kernel rounds s + p - o in another order:
    the precondition keeps every TransE sign the same on both sides.)"""
    N, R, B, G, M = 150, 4, 70, 32, 40
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3)
    X, ids, side = case(6, B, G, M, N, R)
    assert_conditioned(model, ent, rel, X, G, ids, side, R)
    (L1, Ge1, Gr1, ps1, ns1), _ = run_dist(eng, X, G, ids, side, "nll", "mean")
    L2, Ge2, Gr2, ps2, ns2 = run_fwdbwd(eng, X, M, "nll", "mean", seed=0, step=0, negs=SR.override_rows(X, G, ids, side))
    assert within("shared_dist_vs_fused_grad_ent", grad_gap(Ge1, Ge2), 2e-5)
    assert within("shared_dist_vs_fused_grad_rel", grad_gap(Gr1, Gr2), 2e-5)
    assert within("shared_dist_vs_fused_loss", abs(L1 - L2) / max(1.0, abs(L2)), 1e-5)
    assert np.allclose(ps1, ps2, rtol=1e-5, atol=1e-5 * np.abs(ps2).max()) and np.allclose(ns1, ns2, rtol=1e-5, atol=1e-5 * np.abs(ns2).max())


# ------------------------------------------------------------------------------------------------------------------ 5. the masked step
def masked_case(seed, B, G, M, N, R, identity):
    """a batch cut from a graph dense enough that most ranges hold several ids; ranges from a FilterIndex over the graph"""
    from ampligraph_amd.datasets.filters import FilterIndex

    rng = np.random.default_rng(seed)
    D = rand_triples(np.random.default_rng(seed + 1), 6 * N, N, R)
    X = D[rng.integers(0, len(D), B)]
    if identity:
        ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
        side = SR.sample_shared(X, G, 1, seed, 4, sample_range=N)[1]
    else:
        ids, side = SR.sample_shared(X, G, M, seed, 4, sample_range=N)
    ks, ko = FilterIndex([D], N, R).as_lists(X)
    ks, ko = [np.asarray(a, dtype=np.int32) for a in ks], [np.asarray(a, dtype=np.int32) for a in ko]
    return X, ids, side, ks, ko


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("model", DIST_MODELS)
def test_shared_dist_masked_step(gpu_lib, model, identity):
    """GIVEN and IDENTITY lists, one fully known row (kept and counted): the mask of tests/shared_mask_ref.py applied to the reference
    scores, then the oracle's loss; the stats; an exact zero gradient from the masked entries."""
    N, R, k, B, G = 40, 2, 8, 37, 8
    M = N if identity else 33
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = masked_case(5, B, G, M, N, R, identity)
    if not identity:
        i = 11                                                              # a row whose whole list is known
        ks[i] = ko[i] = np.unique(ids[i // G]).astype(np.int32)
    mask, masked, unmaskable = MR.mask_matrix(X, G, ids, side, ks, ko)
    assert masked > B and unmaskable == (0 if identity else 1) and 0 < side.sum() < B
    assert_conditioned(model, ent, rel, X, G, ids, side, R)
    for loss, reduction in (("self_adversarial", "sum"), ("multiclass_nll", "mean")):
        got, stats = run_dist(eng, X, G, ids, side, loss, reduction, ks, ko, identity=identity)
        assert stats == [masked, unmaskable]
        assert np.array_equal(np.isneginf(got[4]), mask.T.reshape(-1)) and np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
        check_against_ref(model, ent, rel, X, G, ids, side, got, loss, reduction, R, mask=mask)
        L, Te, Tr, sp, sn = MR.masked_step(model, ent, rel, X, G, ids, side, mask, loss, reduction, R)   # the oracle's own rows
        assert abs(got[0] - L) <= 1e-5 * max(1.0, abs(L))
        assert_grads_close(got[1], Te)
        assert_grads_close(got[2], Tr)
    # masked entries send an exact zero: an entity that is reached ONLY through masked entries keeps a zero gradient row
    lists = ids[np.arange(B) // G]
    live_ids = set(lists[~mask].tolist()) | set(X[:, 0].tolist()) | set(X[:, 2].tolist())
    only_masked = sorted(set(lists[mask].tolist()) - live_ids)
    assert not got[1][only_masked].any()
    if identity:                                                            # IDENTITY == GIVEN on the arange list: scores and stats bit for bit
        got_g, stats_g = run_dist(eng, X, G, ids, side, "multiclass_nll", "mean", ks, ko)
        assert np.array_equal(got[4].view(np.uint32), got_g[4].view(np.uint32)) and stats_g == stats


def test_shared_dist_masked_zero_gradient_rows(gpu_lib):
    """every corruption of every positive masked but one per row: only that entry's entity and the positives' rows receive a gradient"""
    model, N, R, k, B, G, M = "RotatE", 40, 2, 8, 9, 9, 6
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X = rand_triples(np.random.default_rng(2), B, 10, R)                    # the positives use entities 0 .. 9
    ids = np.array([[20, 21, 22, 23, 24, 25]], dtype=np.int32)
    side = (np.arange(B) % 2).astype(np.int32)
    known = np.array([20, 21, 22, 23, 24], dtype=np.int32)
    ks = ko = [known] * B
    (L, Ge, Gr, ps, ns), stats = run_dist(eng, X, G, ids, side, "nll", "sum", ks, ko)
    assert stats == [5 * B, 0] and np.isneginf(ns.reshape(M, B)[:5]).all() and np.isfinite(ns.reshape(M, B)[5]).all()
    assert not Ge[20:25].any() and Ge[25].any() and not Ge[26:].any() and np.isfinite(Ge).all() and np.isfinite(Gr).all()


def test_shared_dist_masked_step_across_the_score_chunk(gpu_lib):
    """B * M = 4 200 * 4 097 > 2^24 (test_gpu_shared_mask.py::test_masked_step_across_the_score_chunk's shape and batch) on the
    distance tiles: 63 groups of 64 fill the first chunk, rows 4 032 .. 4 199 are the second, whose tiles must read ITS groups' lists
    and whose mask ITS rows' ranges.  The reference is the header's arithmetic (tests/shared_dist_ref.py), a DistStep per group: the
    pairwise loss is a sum over the positives, so the groups' losses and gradients add.  The bars are check_against_ref's, but for
    the entity gradient: a row there is the fp32 sum, by atomics in arrival order, of some 3 * 10^5 terms +-c (TransE: a coefficient
    times a sign, so the terms cancel down to a sum far below their number).  Its gap was 4.47e-5 and 4.63e-5 of the row's largest
    entry in two runs of the two per-family drivers this test was first run on, against 2e-5; the bar is twice the larger.  The
    relation gradient's was 1.95e-6 and 2.01e-6, the scores' 1.55e-7: their bars stay."""
    from test_gpu_shared_mask import mask_case

    model, N, R, k, B, G, M = "TransE", 50, 2, 7, 4200, 64, 4097
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=7)
    known = np.zeros((B, N), dtype=bool)                                     # (mask_matrix, vectorised: ids < N)
    for i in range(B):
        known[i, ks[i] if side[i] else ko[i]] = True
    mask = known[np.arange(B)[:, None], ids[np.arange(B) // G]]
    assert not mask.all(1).any() and mask[4032:].any() and not np.array_equal(mask[4032:], mask[:168])
    got, stats = run_dist(eng, X, G, ids, side, "pairwise", "mean", ks, ko)
    L, Ge, Gr, ps, ns = got
    assert np.array_equal(np.isneginf(ns.reshape(M, B).T), mask) and not np.isposinf(ns).any() and stats == [int(mask.sum()), 0]
    want, Te, Tr, sp, S = 0.0, np.zeros(ent.shape), np.zeros(rel.shape), np.empty(B, np.float32), np.empty((B, M), np.float32)
    for g in range(SR.n_groups(B, G)):
        rows = slice(g * G, min((g + 1) * G, B))
        Lg, Eg, Rg, sp[rows], sn = DR.DistStep(model, ent, rel, X[rows], G, ids[g:g + 1], side[rows], R).step("pairwise", "mean", mask=mask[rows])
        S[rows] = sn.reshape(M, -1).T
        want, Te, Tr = want + Lg, Te + Eg, Tr + Rg
    live = ~mask
    nsm = ns.reshape(M, B).T
    print(f"chunked: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, "
          f"score gap {np.abs(nsm[live] - S[live]).max() / np.abs(S[live]).max():.3g}, masked {stats[0]}")
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(nsm[live], S[live], rtol=1e-5, atol=1e-5 * np.abs(S[live]).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    assert_grads_close(Ge, Te, tol=2 * 4.63e-5)
    assert_grads_close(Gr, Tr)


def test_shared_dist_device_path_refusals(gpu_lib):
    N, R, B, G, M = 50, 3, 10, 4, 6
    X = dev(rand_triples(np.random.default_rng(7), B, N, R))
    ids = torch.zeros(3, M, dtype=torch.int32, device="cuda")
    side = torch.zeros(B, dtype=torch.int32, device="cuda")
    for model in ("DistMult", "ComplEx", "HolE"):
        eng, _, _ = make_engine(model, 8, N, R)
        eng.prepare_training("adam")
        assert not eng.shared_dist_supported(B, G, M) and eng.shared_supported(B, G, M)
        with pytest.raises(ValueError, match="not offered"):
            eng.train_shared_dist_fwdbwd(X, G, M, ids, side, loss_desc("nll"))
    eng, _, _ = make_engine("TransE", 8, N, R)
    eng.prepare_training("adam")
    for bad in ((B, 0, M), (B, G, 0), (B, G, 1 << 24)):
        assert not eng.shared_dist_supported(*bad)
        with pytest.raises(ValueError, match="not offered"):
            eng.train_shared_dist_fwdbwd(X, bad[1], bad[2], ids, side, loss_desc("nll"))
    with pytest.raises(ValueError, match="together"):
        eng.train_shared_dist_fwdbwd(X, G, M, ids, side, loss_desc("nll"), s_filter=(ids, ids, ids))
    torch.cuda.synchronize()
    assert not eng.g_flat.any().item()                                      # nothing ran


# ------------------------------------------------------------------------------------------------------------------ 6. whole steps, fit()
class _RestatedShared:
    """What compile(negatives={"shared_distance": num_negs, ...}) computes, through the PER-CORRUPTION path: a StepLoop.negatives that
    uploads the equivalent override rows of the numpy restatement (the model's eta must be num_negs)."""

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


@pytest.mark.parametrize("model", DIST_MODELS)
def test_fit_with_shared_distance_negatives_equals_fit_on_the_override_rows(gpu_lib, model):
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.latent_features.negatives import BoundSharedNegatives, SharedDistanceNegatives

    X = toy_graph(seed=4, n=400, N=40, R=3)
    M, G = 48, 20

    def new(eta, **kw):
        m = ScoringBasedEmbeddingModel(eta=eta, k=16, scoring_type=model, seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="self_adversarial", entity_relation_regularizer="l2", **kw)
        return m

    m1 = new(2, negatives={"shared_distance": M, "group_size": G})         # (the model's own eta plays no part)
    assert type(m1._negatives) is SharedDistanceNegatives
    h1 = m1.fit(X, batch_size=128, epochs=3, verbose=False)                # 4 batches per epoch, the last one of 16; 7 groups, the last of 8
    assert isinstance(m1._loop.negatives, BoundSharedNegatives) and m1._loop.negatives.distance is True
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


def test_fit_rotate_with_all_entities_masked_equals_the_steps_written_out(gpu_lib):
    """compile(negatives={"shared_distance": "all", "mask_known": True, "side": "bernoulli"}) on RotatE == draw -> masked distance
    step -> sweep written out, in the form of test_gpu_shared_mask.py's fit() test; and the class form trains end to end."""
    from test_gpu_model import toy_graph

    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.latent_features.negatives import BoundMaskedSharedNegatives, SharedDistanceNegatives

    X = toy_graph(seed=4, n=400, N=40, R=3)
    bs, epochs = 128, 2

    def new(**kw):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="RotatE", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", **kw)
        return m

    m1 = new(negatives={"shared_distance": "all", "mask_known": True, "side": "bernoulli"})
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    b = m1._loop.negatives
    assert isinstance(b, BoundMaskedSharedNegatives) and b.identity and b.distance is True
    N = int(m1._n_ents)
    G, M = b.group_size, N
    assert N <= 200 and b.num_negs == N

    m2 = new()
    m2.fit(X, batch_size=bs, epochs=0, verbose=False)
    eng, loop = m2._engine, m2._loop
    Xi = m2.data_indexer.get_indexes(X).astype(np.int32)
    index = FilterIndex([Xi], N, int(m2._n_rels), engine=eng)
    fs, fo = index.as_lists(Xi)
    thr = eng.negatives_side_thresholds(*index.device_keys(eng), index.n_ents, index.n_rels)
    steps = -(-len(Xi) // bs)
    hist, masked_total = [], 0
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    for epoch in range(epochs):
        loop.reset_loss()
        for step in range(steps):
            rows = slice(step * bs, min((step + 1) * bs, len(Xi)))
            batch = dev(Xi[rows])
            B = int(batch.shape[0])
            _, side = eng.sample_shared(batch, G, 1, loop.seed, epoch * steps + step, side="bernoulli", side_thr=thr)
            ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(SR.n_groups(B, G), 1)
            sf, of = filters(fs[rows], fo[rows])
            eng.train_shared_dist_fwdbwd(batch, G, M, ids, side, loop.loss_ffi, s_filter=sf, o_filter=of, identity=True, stats=stats)
            loop.optimizer.iterations += 1
            eng.opt_step(loop.optimizer.to_ffi(loop.optimizer.iterations, 2), loop.reg, loop.reg if isinstance(loop.reg_rel, str) else loop.reg_rel)
            loop.n_steps += 1
            masked_total += MR.mask_matrix(Xi[rows], G, ids.cpu().numpy(), side.cpu().numpy(), fs[rows], fo[rows])[1]
        hist.append(loop.mean_batch_loss())
    print("loss histories", h1.history["loss"], hist, "masked", m1.negative_sampling_stats_, masked_total)
    assert len(h1.history["loss"]) == epochs and np.allclose(h1.history["loss"], hist, rtol=2e-4)
    assert m1.negative_sampling_stats_ == {"masked": masked_total, "unmaskable": 0} and masked_total >= epochs * len(Xi)
    # the class form of the issue's closing example, on a toy graph: finite losses that fall
    m3 = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="RotatE", seed=2)
    m3.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="self_adversarial",
               negatives=SharedDistanceNegatives(1024, side="bernoulli", mask_known=True))
    h3 = m3.fit(X, batch_size=bs, epochs=3, verbose=False)
    assert np.isfinite(h3.history["loss"]).all() and h3.history["loss"][-1] < h3.history["loss"][0]
    assert set(m3.negative_sampling_stats_) == {"masked", "unmaskable"} and m3.negative_sampling_stats_["masked"] > 0


@pytest.mark.parametrize("model,k", [("TransE", 40), ("RotatE", 24)])
def test_shared_dist_whole_steps_match_oracle(gpu_lib, model, k):
    """Three Adam steps (draw on the device -> distance tiles -> amdkge_opt_step with an L2 regulariser) == the oracle's dense steps on
    the override rows: the bars of test_gpu_shared.py::test_shared_whole_steps_match_oracle."""
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
        eng.train_shared_dist_fwdbwd(Xd, G, M, ids, side, ld)
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
