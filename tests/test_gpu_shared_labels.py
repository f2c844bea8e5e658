"""KvsAll training on the GPU (shared_label_loss_kernel in kge_train_shared_labels.hip, include/amdkge_shared_labels.h): the loss
kernel alone against its numpy restatement (tests/shared_labels_ref.py: coefficients, loss sum, both counts), the whole labelled step of
the five models against labelled_step, the NaN / inf positions against the float32 restatement, and fit() with KvsAll + BCELoss."""
import numpy as np
import pytest
import torch

import shared_labels_ref as LR
import shared_mask_ref as MR
import shared_nonfinite_cases as NC
import shared_ref as SR
from test_gpu_kernels import assert_grads_close, dense, dev, make_engine
from test_gpu_shared import grad_gap
from test_gpu_shared_dist import masked_case
from test_gpu_shared_mask import filters, mask_case

pytestmark = pytest.mark.gpu

MODELS = ("TransE", "DistMult", "ComplEx", "HolE", "RotatE")


@pytest.fixture(scope="module")
def label_engine(gpu_lib):
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("DistMult", 4, 64, 2)


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel alone
def run_kernel(eng, S0, row0, G, ids, side, ks, ko, eps, reduction, scale=1.0, w=None, identity=False):
    """-> (the buffer after amdkge_shared_label_loss, loss sum, [labelled, unlabelled_rows])"""
    S = dev(S0)
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    sf, of = filters(ks, ko)
    eng.shared_label_loss(S, row0, G, None if ids is None else dev(ids), dev(side), sf, of, label_smoothing=eps, reduction=reduction, scale=scale,
                          weights=None if w is None else (dev(w[0]), dev(w[1])), identity=identity, loss_sum=acc, stats=stats)
    torch.cuda.synchronize()
    return S.cpu().numpy(), float(acc.item()), stats.cpu().tolist()


def check_kernel(got, S0, labels, side, eps, reduction, scale, w, tag=""):
    """the coefficient is a difference of two O(1) numbers: its bar is absolute, 1e-5 * w / red (times |scale|, which the buffer
    carries); the loss sum rtol 1e-5; the counts exact"""
    C, L, stats = got
    rw = LR.row_weights(side, w)[:labels.shape[0]] if w is not None else np.ones(labels.shape[0])
    want_L, want_C = LR.label_loss(S0, labels, eps, reduction, scale, rw)
    bar = 1e-5 * abs(scale) * rw / (labels.shape[1] if reduction == "mean" else 1.0)
    gap = np.abs(C - want_C)
    print(f"{tag} eps={eps} {reduction}: loss {L:.9g} / {want_L:.9g}, coefficient gap {(gap / bar[:, None]).max():.3g} of the bar, stats {stats}")
    assert (gap <= bar[:, None]).all()
    assert abs(L - want_L) <= 1e-5 * abs(want_L)
    assert stats == [int(labels.sum()), int((~labels.any(1)).sum())]


def both_settings(eng, S0, row0, G, ids, side, ks, ko, labels, identity=False, tag=""):
    """eps = 0 / "sum" / no weights / scale 1, and eps = 0.1 / "mean" / weights / HolE's kind of scale"""
    B = side.shape[0]
    rng = np.random.default_rng(11)
    w = (rng.uniform(0.2, 1.0, B).astype(np.float32), rng.uniform(0.2, 1.0, B).astype(np.float32))
    rows = labels.shape[0]
    for eps, reduction, scale, ww in ((0.0, "sum", 1.0, None), (0.1, "mean", -0.25, w)):
        got = run_kernel(eng, S0, row0, G, ids, side, ks, ko, eps, reduction, scale, ww, identity)
        wrow = None if ww is None else (ww[0][row0:row0 + rows], ww[1][row0:row0 + rows])
        check_kernel(got, S0, labels, side[row0:row0 + rows], eps, reduction, scale, wrow, tag)


def scores(rows, M, seed=9):
    return (np.random.default_rng(seed).normal(size=(rows, M)) * 3).astype(np.float32)


@pytest.mark.parametrize("B,G,M,N,kind", [(1, 1, 1, 1, "fully known"), (37, 8, 5, 10, ""), (37, 8, 63, 40, ""), (37, 8, 64, 40, ""), (37, 8, 65, 40, ""),
                                          (37, 8, 20, 6, "repeated ids"), (37, 8, 33, 40, "empty")])
def test_label_kernel_given(label_engine, B, G, M, N, kind):
    X, ids, side, ks, ko = mask_case(B, G, M, N, kind)
    if kind == "empty":
        ks[1], ko[1] = ks[1][:1], ko[1][:1]                                               # ... and a range of one id
    labels, n_lab, n_none = LR.label_matrix(X, G, ids, side, ks, ko)
    if kind == "fully known":
        assert labels.all() and (n_lab, n_none) == (1, 0)
    elif kind == "repeated ids":
        hits = np.array([len(np.intersect1d(ids[i // G], ks[i] if side[i] else ko[i])) for i in range(B)])   # distinct known ids of the list
        assert all(len(set(r.tolist())) < M for r in ids) and (labels.sum(1) > hits).any()              # ... labelled at each of their places
    elif kind == "empty":
        assert not labels[0].any() and not labels[B - 1].any() and n_none >= 2
    else:
        assert 0 < n_lab < B * M
    both_settings(label_engine, scores(B, M), 0, G, ids, side, ks, ko, labels, tag=f"given B={B} M={M} {kind}")


def test_label_kernel_given_fully_known_rows_among_others(label_engine):
    """N = 3, dense: several rows are all ones (there is no exception), their neighbours are not"""
    X, ids, side, ks, ko = mask_case(37, 8, 4, 3, seed=2)
    labels, n_lab, n_none = LR.label_matrix(X, 8, ids, side, ks, ko)
    assert labels.all(1).any() and not labels.all()
    both_settings(label_engine, scores(37, 4), 0, 8, ids, side, ks, ko, labels, tag="fully known rows")


@pytest.mark.parametrize("B,G,M,N", [(37, 8, 23, 23), (37, 8, 15, 23), (301, 64, 130, 130)])
def test_label_kernel_identity(label_engine, B, G, M, N):
    """ids[g][j] == j: the range is walked beside the chunks of j.  M < N: the range's ids >= M are ignored.  IDENTITY == GIVEN on the
    arange list, bit for bit."""
    X, _, side, ks, ko = mask_case(B, G, M, N, seed=3)
    ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
    labels, n_lab, n_none = LR.label_matrix(X, G, ids, side, ks, ko)
    assert n_lab > 0 and (M >= N or max(max(a) for a in ks + ko if len(a)) >= M)
    S0 = scores(B, M)
    both_settings(label_engine, S0, 0, G, None, side, ks, ko, labels, identity=True, tag=f"identity B={B} M={M}")
    gi = run_kernel(label_engine, S0, 0, G, None, side, ks, ko, 0.1, "mean", identity=True)
    gg = run_kernel(label_engine, S0, 0, G, ids, side, ks, ko, 0.1, "mean")
    assert np.array_equal(gi[0].view(np.uint32), gg[0].view(np.uint32)) and gi[2] == gg[2]


def test_label_kernel_identity_edges(label_engine):
    """M = 200 (three chunks of 64 and a tail of 8).  Rows: an empty range; a range of one id; a fully known row (200 ids: windows of
    64 reloaded three times); a range of more than 64 ids with gaps; ids 63 and 64 together (the chunk seam) and 127, 128; the last id
    of the list alone; a range that ENDS at the last element of its id array (the o side's is built last)."""
    B, G, M = 9, 4, 200
    rng = np.random.default_rng(5)
    ranges = [np.zeros(0, np.int32), np.array([77], np.int32), np.arange(M, dtype=np.int32),
              np.sort(rng.choice(M, 90, replace=False)).astype(np.int32), np.array([63, 64, 127, 128], np.int32), np.array([M - 1], np.int32),
              np.array([0, 63], np.int32), np.array([64], np.int32), np.sort(rng.choice(M, 70, replace=False)).astype(np.int32)]
    side = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0], np.int32)
    other = [np.sort(rng.choice(M, 5, replace=False)).astype(np.int32) for _ in range(B)]   # the side NOT taken: must not be read as labels
    ks = [ranges[i] if side[i] else other[i] for i in range(B)]
    ko = [other[i] if side[i] else ranges[i] for i in range(B)]
    X = np.zeros((B, 3), np.int32)
    ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
    labels, n_lab, n_none = LR.label_matrix(X, G, ids, side, ks, ko)
    assert n_none == 1 and labels[2].all() and labels[4, 63] and labels[4, 64] and labels[3].sum() == 90 and labels[5, M - 1] and labels.sum(1).tolist() == [len(r) for r in ranges]
    lo, hi, flat = MR.csr(ko)
    assert hi[B - 1] == len(flat)                                                         # row 8 (side o) ends at the array's last id
    both_settings(label_engine, scores(B, M), 0, G, None, side, ks, ko, labels, identity=True, tag="identity edges")
    both_settings(label_engine, scores(B, M), 0, G, ids, side, ks, ko, labels, tag="the same, given")


@pytest.mark.parametrize("identity", [False, True])
def test_label_kernel_window(label_engine, identity):
    """row0 != 0: the buffer is rows [13, 30) of a batch of 37 -- the window starts inside a group and ends in a short last one"""
    B, G, M, N, row0, rows = 37, 8, 33, 40, 13, 17
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=4)
    if identity:
        ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
    full, _, _ = LR.label_matrix(X, G, ids, side, ks, ko)
    labels = full[row0:row0 + rows]
    assert labels.any() and not np.array_equal(labels, full[:rows])
    both_settings(label_engine, scores(rows, M), row0, G, None if identity else ids, side, ks, ko, labels, identity=identity, tag=f"window identity={identity}")
    B2, row2, rows2 = 37, 24, 13                                                          # rows [24, 37): ends in the last group of 5
    both_settings(label_engine, scores(rows2, M), row2, G, None if identity else ids, side, ks, ko, full[row2:row2 + rows2], identity=identity, tag="window to the end")


# ------------------------------------------------------------------------------------------------------------------ 2. the whole step
def run_labelled(eng, X, G, ids, side, ks, ko, eps, reduction, w=None, identity=False):
    """-> ((loss sum, dense entity gradient, dense relation gradient, positive scores, corruption scores [M * B]), [labelled, unlabelled_rows])"""
    B, M = X.shape[0], ids.shape[1]
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ps = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B * M,), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    sf, of = filters(ks, ko)
    fn = eng.train_shared_dist_labels_fwdbwd if eng.scoring_type in ("TransE", "RotatE") else eng.train_shared_labels_fwdbwd
    fn(dev(X), G, M, dev(ids), dev(side), sf, of, label_smoothing=eps, reduction=reduction, weights=None if w is None else (dev(w[0]), dev(w[1])),
       identity=identity, stats=stats, pos_scores=ps, neg_scores=ns)
    torch.cuda.synchronize()
    return (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel), ps.cpu().numpy(), ns.cpu().numpy()), stats.cpu().tolist()


def check_against_labelled_step(model, ent, rel, X, G, ids, side, labels, got, eps, reduction, w, R, tag=""):
    """test_gpu_shared_mask.py::check_against_masked_step's bars: rtol 1e-5, atol 1e-5 * max|ref|"""
    L, Ge, Gr, ps, ns = got
    want, Te, Tr, sp, sn = LR.labelled_step(model, ent, rel, X, G, ids, side, labels, eps, reduction, w, R)
    print(f"{tag} {model} eps={eps} {reduction}: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, "
          f"score gap {np.abs(ns - sn).max() / np.abs(sn).max():.3g}")
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


@pytest.mark.parametrize("model", MODELS)
def test_labelled_fwdbwd_parity(gpu_lib, model):
    """B = 37 in groups of 8 (a last group of 5), M = 33 crosses the 32-wide tile; eps in {0, 0.1} x both reductions"""
    N, R, k, B, G, M = 40, 2, 8, 37, 8, 33
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = masked_case(5, B, G, M, N, R, False)
    labels, n_lab, n_none = LR.label_matrix(X, G, ids, side, ks, ko)
    assert n_lab > B and 0 < side.sum() < B
    for eps in (0.0, 0.1):
        for reduction in ("sum", "mean"):
            got, stats = run_labelled(eng, X, G, ids, side, ks, ko, eps, reduction)
            check_against_labelled_step(model, ent, rel, X, G, ids, side, labels, got, eps, reduction, None, R)
            assert stats == [n_lab, n_none]


@pytest.mark.parametrize("model", ["ComplEx", "RotatE"])
def test_labelled_fwdbwd_identity_list_with_weights(gpu_lib, model):
    """the KvsAll step proper: ids[g][j] = j, M = N, IDENTITY mode, row weights; every positive's own entity is a labelled column;
    == the same call in GIVEN mode"""
    N, R, k, B, G = 40, 2, 8, 37, 8
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = masked_case(6, B, G, N, N, R, True)
    labels, n_lab, n_none = LR.label_matrix(X, G, ids, side, ks, ko)
    assert labels[np.arange(B), np.where(side != 0, X[:, 0], X[:, 2])].all() and n_none == 0
    rng = np.random.default_rng(3)
    w = (rng.uniform(0.2, 1.0, B).astype(np.float32), rng.uniform(0.2, 1.0, B).astype(np.float32))
    got, stats = run_labelled(eng, X, G, ids, side, ks, ko, 0.1, "mean", w, identity=True)
    check_against_labelled_step(model, ent, rel, X, G, ids, side, labels, got, 0.1, "mean", w, R, tag="identity")
    assert stats == [n_lab, 0]
    unweighted, _ = run_labelled(eng, X, G, ids, side, ks, ko, 0.1, "mean", None, identity=True)
    assert abs(unweighted[0] - got[0]) > 0.05 * abs(got[0])                               # the weights did something
    got_g, stats_g = run_labelled(eng, X, G, ids, side, ks, ko, 0.1, "mean", w)
    assert np.array_equal(got[4].view(np.uint32), got_g[4].view(np.uint32)) and stats_g == stats and abs(got_g[0] - got[0]) <= 1e-6 * abs(got[0])


def test_labelled_step_with_empty_ranges(gpu_lib):
    """every range empty: every label 0, every row counted as unlabelled -- equal to the restatement"""
    N, R, k, B, G, M = 40, 2, 8, 37, 8, 33
    eng, ent, rel = make_engine("DistMult", k, N, R, scale=0.6)
    X, ids, side, ks, ko = masked_case(8, B, G, M, N, R, False)
    none = [a[:0] for a in ks]
    labels = np.zeros((B, M), dtype=bool)
    got, stats = run_labelled(eng, X, G, ids, side, none, none, 0.1, "sum")
    check_against_labelled_step("DistMult", ent, rel, X, G, ids, side, labels, got, 0.1, "sum", None, R, tag="empty ranges")
    assert stats == [0, B]


def test_labelled_step_across_the_score_chunk(gpu_lib):
    """B * M = 4 200 * 4 097 > 2^24 (test_masked_step_across_the_score_chunk's shape): rows 4 032 .. 4 199 are the second chunk, whose
    labels must be taken from ITS rows' ranges.  The reference is the step's matrix form in fp64 (DistMult: score = <q_i, e>).
    Every one of the 17 M coefficients is non-zero here (a hinge zeroes most of them in the masked test), so an entity row is the
    fp32 sum of about 340 000 terms of both signs: the entity gradient's gap was 1.39e-5 and 1.41e-5 of the row's largest entry in
    two runs, against the bar of 2e-5; the relation gradient's 1.4e-6 and 1.7e-6."""
    model, N, R, k, B, G, M = "DistMult", 50, 2, 7, 4200, 64, 4097
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    X, ids, side, ks, ko = mask_case(B, G, M, N, seed=7)
    known = np.zeros((B, N), dtype=bool)
    for i in range(B):
        known[i, ks[i] if side[i] else ko[i]] = True
    grp = np.arange(B) // G
    labels = known[np.arange(B)[:, None], ids[grp]]
    assert labels[4032:].any() and not np.array_equal(labels[4032:], labels[:168])
    got, stats = run_labelled(eng, X, G, ids, side, ks, ko, 0.1, "mean")
    L, Ge, Gr, ps, ns = got
    assert stats == [int(labels.sum()), int((~labels.any(1)).sum())]
    e64, r64 = ent.astype(np.float64), rel.astype(np.float64)
    subj = side != 0
    kept = np.where(subj[:, None], e64[X[:, 2]], e64[X[:, 0]])
    p = r64[X[:, 1]]
    Q = p * kept
    groups = [slice(g * G, min((g + 1) * G, B)) for g in range(SR.n_groups(B, G))]
    S = np.concatenate([Q[rows] @ e64[ids[g]].T for g, rows in enumerate(groups)])         # [B, M]
    assert np.allclose(ns.reshape(M, B).T, S, rtol=1e-5, atol=1e-5 * np.abs(S).max())
    per, Cn = LR.bce64(S, labels, 0.1, "mean", np.ones(B))
    want = float(per.sum())
    assert abs(L - want) <= 1e-5 * max(1.0, abs(L)), (L, want)
    t = np.concatenate([Cn[rows] @ e64[ids[g]] for g, rows in enumerate(groups)])          # dL/dq: the positive's own coefficient is zero
    Te, Tr = np.zeros_like(e64), np.zeros_like(r64)
    np.add.at(Te, np.where(subj, X[:, 2], X[:, 0]), t * p)
    np.add.at(Tr, X[:, 1], t * kept)
    for g, rows in enumerate(groups):
        np.add.at(Te, ids[g], Cn[rows].T @ Q[rows])
    print(f"chunked: loss {L:.9g} / {want:.9g}, grad gap ent {grad_gap(Ge, Te):.3g} rel {grad_gap(Gr, Tr):.3g}, labelled {stats[0]}")
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


# ------------------------------------------------------------------------------------------------------------------ 3. NaN and inf
def test_label_kernel_nonfinite_scores(label_engine):
    """NaN, +inf and -inf scores under both labels: the NaN / inf POSITIONS of the coefficients and the loss are the float32
    restatement's (bce32: the header's formula in IEEE fp32); rows without one are untouched by their neighbours"""
    B, G, M = 8, 4, 70
    rng = np.random.default_rng(2)
    S0 = scores(B, M)
    side = np.zeros(B, np.int32)
    ko = [np.array([1, 66], np.int32) for _ in range(B)]
    ks = [np.zeros(0, np.int32) for _ in range(B)]
    for r, v in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        S0[r, 1], S0[r, 5], S0[r, 66], S0[r, 69] = v, v, v, v                             # labelled and unlabelled, both chunks
    ids = np.tile(np.arange(M, dtype=np.int32), (2, 1))
    labels = LR.label_matrix(np.zeros((B, 3), np.int32), G, ids, side, ks, ko)[0]
    for eps in (0.0, 0.1):
        ell, c, wr = LR.bce32(S0, labels, eps, "sum", np.ones(B))
        for row in range(B):                                                              # a row at a time: the loss sum of that row alone
            C, L, _ = run_kernel(label_engine, S0[row:row + 1], row, G, None, side, ks, ko, eps, "sum", identity=True)
            with np.errstate(invalid="ignore"):
                want = ell[row].astype(np.float64).sum()
            assert np.array_equal(np.isnan(C[0]), np.isnan(c[row])) and np.array_equal(np.isinf(C[0]), np.isinf(c[row])), (eps, row)
            assert np.isnan(L) == np.isnan(want) and np.isposinf(L) == np.isposinf(want), (eps, row, L, want)
            assert (row in (1, 2, 3)) != bool(np.isfinite(L))
            fin = np.isfinite(c[row])
            assert np.allclose(C[0][fin], c[row][fin], rtol=0, atol=1e-5)
        C, L, _ = run_kernel(label_engine, S0, 0, G, None, side, ks, ko, eps, "sum", identity=True)
        assert np.isnan(L) and np.isfinite(C[[0, 4, 5, 6, 7]]).all()


@pytest.mark.parametrize("entry,model,plant", [("masked_given", "ComplEx", "list_nan_row"), ("masked_given", "ComplEx", "list_inf_unit"),
                                               ("dist_given", "TransE", "list_inf_unit")])
def test_labelled_step_nonfinite_tables(gpu_lib, entry, model, plant):
    """ONE list entry of group 1 is an entity row holding NaN (ComplEx), +inf (ComplEx: +-inf or NaN scores) or +inf (TransE: a
    distance of inf, a score of -inf).  Where NaN and inf land -- scores, loss, gradient rows -- is where the float32 restatement puts
    them; the rows that belong to the other groups alone are finite and right."""
    case = NC.build(entry, model, plant)
    eng = make_engine(model, case.k, case.N, case.R)[0]
    eng.set_tables(case.ent, case.rel)
    X, ids, side, ks, ko = case.X, case.ids, case.side, case.ks, case.ko
    labels = LR.label_matrix(X, case.G, ids, side, ks, ko)[0]
    for eps in (0.0, 0.1):
        with np.errstate(all="ignore"):
            ell, c, Te, Tr, sn = LR.labelled_step32(model, case.ent, case.rel, X, case.G, ids, side, labels, eps, "sum", None, case.R)
            want = ell.astype(np.float64).sum()
        (L, Ge, Gr, ps, ns), _ = run_labelled(eng, X, case.G, ids, side, ks, ko, eps, "sum")
        ns = ns.reshape(case.M, case.B).T
        grp1 = np.arange(case.B) // case.G == 1
        assert not np.isfinite(sn[grp1, 2]).all() and np.isfinite(np.delete(sn, 2, 1)).all() and np.isfinite(sn[~grp1]).all()   # the plant is where it should be
        assert np.array_equal(np.isnan(ns), np.isnan(sn)) and np.array_equal(np.isposinf(ns), np.isposinf(sn)) and np.array_equal(np.isneginf(ns), np.isneginf(sn))
        assert np.isnan(L) == np.isnan(want) and np.isposinf(L) == np.isposinf(want) and not np.isfinite(L), (L, want)
        print(f"{model} {plant} eps={eps}: loss {L} / {want}, bad entity rows {int(NC.bad_rows(Ge).sum())} / {int(NC.bad_rows(Te).sum())}, "
              f"relation rows {int(NC.bad_rows(Gr).sum())} / {int(NC.bad_rows(Tr).sum())}")
        assert np.array_equal(NC.bad_rows(Ge), NC.bad_rows(Te)) and np.array_equal(NC.bad_rows(Gr), NC.bad_rows(Tr))
        clean_e, clean_r = case.clean_rows()
        assert np.isfinite(Ge[clean_e]).all() and np.isfinite(Gr[clean_r]).all() and len(clean_e) > 0
        ok_e, ok_r = ~NC.bad_rows(Te), ~NC.bad_rows(Tr)
        assert_grads_close(Ge[ok_e], Te[ok_e])
        assert_grads_close(Gr[ok_r], Tr[ok_r])


# ------------------------------------------------------------------------------------------------------------------ 4. through fit()
def repeated_query_graph(seed=4, n=400, N=40, R=3):
    """tests/test_gpu_model.py::toy_graph with a few duplicated triples: 400 rows over 120 (s, p) pairs, so queries repeat"""
    from test_gpu_model import toy_graph

    X = toy_graph(seed=seed, n=n, N=N, R=R)
    return np.concatenate([X, X[:8]])


def new_model(scoring="ComplEx", reg="l2", **kw):
    from ampligraph_amd.latent_features import BCELoss, ScoringBasedEmbeddingModel, optimizers

    m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type=scoring, seed=2)
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss=BCELoss({"label_smoothing": 0.1, "reduction": "mean"}),
              entity_relation_regularizer=reg, **kw)
    return m


def written_out(m2, X, bs, epochs, weight, G, batch_reg=False):
    """the steps of fit() written out on a model built the same way (epochs=0: tables initialised, no step): side draw -> labelled step
    (-> batch regulariser) -> sweep.  -> (loss history, labelled total, unlabelled rows total)"""
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.latent_features.negatives import KvsAll

    eng, loop = m2._engine, m2._loop
    Xi = m2.data_indexer.get_indexes(X).astype(np.int32)
    N = int(m2._n_ents)
    fs, fo = FilterIndex([Xi], N, int(m2._n_rels)).as_lists(Xi)
    ws, wo = KvsAll.query_weights(Xi)
    steps = -(-len(Xi) // bs)
    hist, lab, unl = [], 0, 0
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    fn = eng.train_shared_dist_labels_fwdbwd if m2.scoring_type in ("TransE", "RotatE") else eng.train_shared_labels_fwdbwd
    for epoch in range(epochs):
        loop.reset_loss()
        for step in range(steps):
            rows = slice(step * bs, min((step + 1) * bs, len(Xi)))
            batch = dev(Xi[rows])
            B = int(batch.shape[0])
            _, side = eng.sample_shared(batch, G, 1, loop.seed, epoch * steps + step)
            ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(SR.n_groups(B, G), 1)
            sf, of = filters(fs[rows], fo[rows])
            w = (dev(ws[rows]), dev(wo[rows])) if weight == "query" else None
            fn(batch, G, N, ids, side, sf, of, label_smoothing=0.1, reduction="mean", weights=w, identity=True, stats=stats)
            loop.optimizer.iterations += 1
            reg_e, reg_r = loop.reg, loop.reg if isinstance(loop.reg_rel, str) else loop.reg_rel
            if batch_reg:
                eng.batch_reg_fwdbwd(batch, reg_e, reg_r)
                reg_e = reg_r = None
            eng.opt_step(loop.optimizer.to_ffi(loop.optimizer.iterations, 2), reg_e, reg_r)
            loop.n_steps += 1
            _, a, b = LR.label_matrix(Xi[rows], G, ids.cpu().numpy(), side.cpu().numpy(), fs[rows], fo[rows])
            lab, unl = lab + a, unl + b
        hist.append(loop.mean_batch_loss())
    assert stats.cpu().tolist() == [lab, unl]
    return hist, lab, unl


@pytest.mark.parametrize("model,weight", [("ComplEx", "triple"), ("ComplEx", "query"), ("TransE", "triple")])
def test_fit_with_kvsall_equals_the_steps_written_out(gpu_lib, model, weight):
    from ampligraph_amd.latent_features.negatives import BoundKvsAll, SharedNegatives

    X = repeated_query_graph()
    bs, epochs = 128, 3
    m1 = new_model(model, negatives={"kvsall": "all", "weight": weight})
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    b = m1._loop.negatives
    assert isinstance(b, BoundKvsAll) and b.identity and b.num_negs == int(m1._n_ents) and b.group_size == SharedNegatives.ALL_GROUP_SIZE
    assert b.distance == (model == "TransE") and (b.row_weights is None) == (weight == "triple")
    m2 = new_model(model, negatives={"kvsall": "all", "weight": weight})
    m2.fit(X, batch_size=bs, epochs=0, verbose=False)
    hist, lab, unl = written_out(m2, X, bs, epochs, weight, b.group_size)
    print("loss histories", h1.history["loss"], hist, "stats", m1.negative_sampling_stats_, (lab, unl))
    assert len(h1.history["loss"]) == epochs and np.allclose(h1.history["loss"], hist, rtol=2e-4)
    assert m1.negative_sampling_stats_ == {"labelled": lab, "unlabelled_rows": unl} and unl == 0 and lab >= epochs * len(X)
    if weight == "query":                                                                 # queries repeat: another objective
        h3 = new_model(model, negatives={"kvsall": "all", "weight": "triple"}).fit(X, batch_size=bs, epochs=epochs, verbose=False)
        assert not np.allclose(h1.history["loss"], h3.history["loss"], rtol=2e-4) and np.isfinite(h3.history["loss"]).all()


def test_fit_with_kvsall_and_n3(gpu_lib):
    """labelled step -> batch regulariser -> sweep; the epoch loss includes the penalty"""
    X = repeated_query_graph()
    bs, epochs = 128, 2
    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer

    n3 = lambda: BatchLPRegularizer(3, 1e-2)   # noqa: E731
    m1 = new_model(reg=n3(), negatives={"kvsall": "all"})
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False)
    m2 = new_model(reg=n3(), negatives={"kvsall": "all"})
    m2.fit(X, batch_size=bs, epochs=0, verbose=False)
    hist, _, _ = written_out(m2, X, bs, epochs, "triple", m1._loop.negatives.group_size, batch_reg=True)
    h0 = new_model(reg=None, negatives={"kvsall": "all"}).fit(X, batch_size=bs, epochs=epochs, verbose=False)
    print("with N3", h1.history["loss"], hist, "without", h0.history["loss"])
    assert np.allclose(h1.history["loss"], hist, rtol=2e-4)
    assert h1.history["loss"][0] > h0.history["loss"][0] * (1 + 1e-3)                     # the same first steps' data loss, plus the penalty


def test_kvsall_learns_the_planted_graph_and_survives_a_round_trip(gpu_lib, tmp_path):
    from planted import planted_kg

    from ampligraph_amd.latent_features import BCELoss, KvsAll, ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.utils.model_utils import restore_model, save_model

    kg = planted_kg("ComplEx", n_ents=120, n_rels=4, n_test=50, seed=0)
    X = kg["train"].astype(str)
    m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=0)
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": 2e-2}), loss=BCELoss({"label_smoothing": 0.1}), negatives=KvsAll(weight="query"))
    h = m.fit(X, batch_size=512, epochs=8, verbose=False).history["loss"]
    print("planted graph, epoch losses", h)
    assert np.isfinite(h).all() and h[-1] < h[0]
    save_model(m, str(tmp_path / "kvsall"))
    r = restore_model(str(tmp_path / "kvsall"))
    assert isinstance(r.loss, BCELoss) and r.loss._loss_parameters == m.loss._loss_parameters and r._negatives.get_config() == m._negatives.get_config()
    assert np.array_equal(r.predict(X[:20]), m.predict(X[:20]))
    h2 = r.fit(X, batch_size=512, epochs=1, verbose=False).history["loss"]                # continued training takes the labelled step again
    assert np.isfinite(h2).all() and set(r.negative_sampling_stats_) == {"labelled", "unlabelled_rows"}
