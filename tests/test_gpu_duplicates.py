"""find_duplicates / find_clusters on the MI355X: the self-join kernels (kge_join.hip) against fp64 brute force, the public
functions against the reference's procedure restated on the downloaded embeddings (sklearn radius_neighbors per tolerance,
scipy.optimize.bisect on [0, largest euclidean pair distance]), and the reference's own tests restated."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine():
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("DistMult", 4, 4, 2)


def _d2_fp64(X):
    """Squared distances in fp64, direct form, a few rows at a time."""
    t = torch.as_tensor(X, dtype=torch.float64).cuda()
    n, d = t.shape
    step = max(1, (1 << 27) // (n * d))
    return torch.cat([((t[i:i + step, None, :] - t[None, :, :]) ** 2).sum(-1) for i in range(0, n, step)]).cpu().numpy()


def _table(n, d, seed):
    """Gaussian rows with integer-valued rows (exact ties) and exact duplicate rows mixed in."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[::3] = rng.integers(-2, 3, size=X[::3].shape)
    if n > 5:
        X[5::17] = X[4::17][:len(X[5::17])]
    return X


@pytest.mark.parametrize("d", [1, 3, 4, 10, 400, 1200])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097])
def test_join_nearest_and_radius_against_fp64(gpu_lib, n, d):
    eng = _engine()
    X = _table(n, d, n * 7 + d)
    dist, idx, mx = eng.join_nearest(torch.as_tensor(X).cuda())
    dist, idx, mx = dist.cpu().numpy(), idx.cpu().numpy(), float(mx.item())
    if n == 1:
        assert dist[0] == np.inf and idx[0] == -1 and mx == 0.0
        assert eng.join_radius(torch.as_tensor(X).cuda(), 1e30).shape == (0, 2)
        return
    D = _d2_fp64(X)
    rel = (d + 2) * 2.0 ** -24
    assert abs(mx - D.max()) <= rel * D.max()
    np.fill_diagonal(D, np.inf)
    want = D.min(1)
    assert np.all(np.abs(dist - want) <= rel * want)
    # nearest index: identical (lower index on ties) wherever fp64 separates the best from the next other candidate by more than
    # the rounding bound; elsewhere the kernel's pick lies within the bound
    first = D.argmin(1)
    Dn = D.copy()
    Dn[np.arange(n), first] = np.inf
    tied = Dn.min(1) == want
    second = Dn.min(1)
    exact = (want == np.round(want)) & (second == np.round(second))   # integer rows: both sums exact in fp32 as well
    clear = tied | exact | (second - want > 4 * rel * np.maximum(want, 1e-30))
    assert clear.mean() > 0.95
    assert np.array_equal(idx[clear & ~tied], first[clear & ~tied])
    for i in np.flatnonzero(tied):   # exact ties (integer rows, duplicate rows): the lowest index among the equal minima
        assert idx[i] == np.flatnonzero(D[i] == want[i])[0]
    assert np.all(D[np.arange(n), idx] <= want * (1 + 2 * rel))
    # radius pairs at thresholds in gaps of the pair distances
    iu = np.triu_indices(n, 1)
    v = np.sort(D[iu])
    for q in (0.001, 0.05, 0.5):
        k = int(q * (len(v) - 1))
        while k + 1 < len(v) and (v[k + 1] - v[k]) <= 2e-4 * v[k + 1]:
            k += 1
        if k + 1 >= len(v):
            continue
        thr = 0.5 * (v[k] + v[k + 1])
        assert not np.any(np.abs(v - thr) <= 1e-4 * thr)
        got = eng.join_radius(torch.as_tensor(X).cuda(), thr).cpu().numpy()
        m = D[iu] <= thr
        wantp = np.stack([iu[0][m], iu[1][m]], 1)
        assert np.array_equal(got, wantp)   # sorted lexicographically


def test_radius_capacity_and_retry(gpu_lib):
    from ampligraph_amd import _ffi

    eng = _engine()
    X = torch.as_tensor(_table(200, 10, 1)).cuda()
    buf = torch.empty(1, 2, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    _ffi.check(gpu_lib.amdkge_join_radius(C.c_void_p(X.data_ptr()), 200, 10, 1e30, C.c_void_p(buf.data_ptr()), 1,
                                          C.c_void_p(count.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert int(count.item()) == 200 * 199 // 2
    got = eng.join_radius(X, 1e30).cpu().numpy()   # 19900 pairs > the first buffer (4096): one relaunch
    iu = np.triu_indices(200, 1)
    assert np.array_equal(got, np.stack(iu, 1))


def test_nearest_and_radius_agree(gpu_lib):
    """Rows in join_radius pairs are exactly the rows whose join_nearest distance is <= thr (the same fp32 values)."""
    eng = _engine()
    rng = np.random.default_rng(4)
    X = torch.as_tensor(_table(3000, 24, 9)).cuda()
    dist = eng.join_nearest(X)[0].cpu().numpy().astype(np.float64)
    for thr in np.concatenate([rng.uniform(dist.min(), np.quantile(dist, 0.3), 6), np.quantile(dist, [0.1, 0.2])]):
        p = eng.join_radius(X, float(thr)).cpu().numpy()
        assert set(np.unique(p).tolist()) == set(np.flatnonzero(dist <= thr).tolist())


def test_large_n_planted(gpu_lib):
    """n = 100 000 (782 tile columns; beyond a 65 535-split grid): the planted near-duplicate pairs, and nothing else."""
    eng = _engine()
    rng = np.random.default_rng(0)
    n, d = 100_000, 64
    X = rng.normal(size=(n, d)).astype(np.float32)
    a = rng.choice(n, 600, replace=False)
    src, dst = a[:300], a[300:]
    X[dst] = X[src] + 1e-3 * rng.normal(size=(300, d)).astype(np.float32)
    Xd = torch.as_tensor(X).cuda()
    got = eng.join_radius(Xd, 0.25).cpu().numpy()
    want = np.stack([np.minimum(src, dst), np.maximum(src, dst)], 1)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    assert np.array_equal(got, want)
    dist, idx, _ = eng.join_nearest(Xd)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx[src], dst) and np.array_equal(idx[dst], src)


# ------------------------------------------------------------------------------------------------------------- public API
def _ref_dups(emb, labels, metric, tol):
    from sklearn.neighbors import NearestNeighbors

    nb = NearestNeighbors(metric=metric, radius=tol).fit(emb).radius_neighbors(emb)[1]
    return {frozenset(labels[j] for j in row) for row in nb if len(row) > 1}


def _ref(emb, labels, metric, tolerance, expected=0.1):
    """The reference's find_duplicates on numpy embeddings -> (sets, tolerance, the tolerances its bisection evaluated)."""
    from scipy import optimize, spatial

    seen = []

    def f(t):
        seen.append(t)
        return len(set().union(*_ref_dups(emb, labels, metric, t))) / len(emb) - expected

    if tolerance == "auto":
        tolerance = optimize.bisect(f, 0.0, spatial.distance_matrix(emb, emb).max(), xtol=1e-3, maxiter=50)
    return _ref_dups(emb, labels, metric, tolerance), tolerance, seen


def _margins_ok(emb, metric, tol, seen):
    from sklearn.metrics import pairwise_distances

    D = pairwise_distances(emb.astype(np.float64), metric=metric)
    np.fill_diagonal(D, np.inf)
    near = D.min(1)
    if any(np.any(np.abs(near - t) <= 1e-4 * t) for t in seen if t > 0):   # (0: exact duplicates sit there)
        return False
    return not np.any(np.abs(D[np.isfinite(D)] - tol) <= 1e-4 * tol)


def _planted_model(seed, fitted=None):
    from test_gpu_discovery import _fit_model

    m, X = fitted or _fit_model()
    eng = m._engine
    rng = np.random.default_rng(seed)
    ent = rng.normal(size=(eng.n_ents, eng.K)).astype(np.float32)
    rel = rng.normal(size=(eng.n_rels, eng.K)).astype(np.float32)
    p = rng.choice(eng.n_ents, 24, replace=False)
    ent[p[12:]] = ent[p[:12]] + 3e-3 * rng.normal(size=(12, eng.K)).astype(np.float32)
    ent[p[0]] = 0.0   # zero-norm row: cosine distance 1 to every other row in sklearn
    rel[1] = rel[0] + 3e-3 * rng.normal(size=eng.K).astype(np.float32)
    eng.set_tables(ent, rel)
    m._planted_rows = p
    return m, X


def _inputs(m, X, mode):
    ents = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
    if mode == "e":
        return ents, m.get_embeddings(ents, "e"), ents.tolist()
    if mode == "r":
        rels = np.unique(X[:, 1])
        return rels, m.get_embeddings(rels, "r"), rels.tolist()
    # repeated triples (one-element sets) and triples that differ only in a planted near-duplicate subject
    p = m.data_indexer.get_indexes(m._planted_rows, "e", "ind2raw")
    near = np.array([[p[k], "r0", X[0, 2]] for k in range(1, 24) if k != 12])
    T = np.concatenate([X[:150], X[:5], near])
    emb = np.hstack([m.get_embeddings(T[:, 0], "e"), m.get_embeddings(T[:, 1], "r"), m.get_embeddings(T[:, 2], "e")])
    return T, emb, [tuple(r) for r in T.tolist()]


@pytest.mark.parametrize("mode", ["e", "r", "t"])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("tolerance", ["num", "auto"])
def test_find_duplicates_matches_reference(gpu_lib, mode, metric, tolerance):
    from ampligraph_amd.discovery import find_duplicates

    fitted = None
    for seed in range(20):   # planted tables whose distances keep the asserted margins
        m, X = fitted = _planted_model(seed, fitted)
        Xin, emb, labels = _inputs(m, X, mode)
        tol = tolerance if tolerance == "auto" else (1e-3 if metric == "cosine" else 0.1)
        expected = 0.3 if mode == "r" else 0.1
        want, want_tol, seen = _ref(emb, labels, metric, tol, expected)
        if _margins_ok(emb, "cosine" if metric == "cosine" else "euclidean", want_tol, seen):
            break
    else:
        pytest.fail("no planted table keeps the margins")
    got, got_tol = find_duplicates(Xin, m, mode=mode, metric=metric, tolerance=tol, expected_fraction_duplicates=expected)
    if tolerance == "auto":
        assert got_tol == pytest.approx(want_tol, rel=1e-5)
    else:
        assert got_tol == tol
    assert got == want


def test_fallback_metric_and_errors(gpu_lib):
    from ampligraph_amd.discovery import find_duplicates

    m, X = _planted_model(0)
    Xin, emb, labels = _inputs(m, X, "e")
    got, tol = find_duplicates(Xin, m, metric="manhattan", tolerance=0.2)
    assert tol == 0.2 and got == _ref_dups(emb, labels, "manhattan", 0.2)
    with pytest.raises(ValueError, match="mode"):
        find_duplicates(Xin, m, mode="x")
    with pytest.raises(ValueError, match="three columns"):
        find_duplicates(Xin, m, mode="t")
    with pytest.raises(ValueError, match="must be an array"):
        find_duplicates(X, m, mode="e")
    with pytest.raises(ValueError, match="nobody"):
        find_duplicates(np.array(["e1", "nobody"]), m, mode="e", tolerance=0.1)
    ent, rel = m._engine.get_tables()
    ent[3, 0] = np.nan
    m._engine.set_tables(ent, rel)
    with pytest.raises(ValueError, match="NaN"):
        find_duplicates(Xin, m, tolerance=0.1)

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    u = ScoringBasedEmbeddingModel(eta=1, k=4, scoring_type="TransE")
    with pytest.raises(ValueError, match="not been fitted"):
        find_duplicates(Xin, u)


def _reference_toy_model(seed=0, batch_size=2):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = np.array([["a", "y", "b"], ["b", "y", "a"], ["a", "y", "c"], ["c", "y", "a"], ["a", "y", "d"], ["c", "x", "d"],
                  ["b", "y", "c"], ["f", "y", "e"], ["a", "z", "e"]])
    model = ScoringBasedEmbeddingModel(eta=5, k=10, scoring_type="ComplEx", seed=seed)
    model.compile(optimizer="adam", loss="multiclass_nll")
    model.fit(X, batch_size=batch_size, epochs=10, verbose=False)
    return model, X


def test_reference_find_duplicates(gpu_lib):
    """tests/ampligraph/discovery/test_discovery.py::test_find_duplicates of the reference, restated."""
    from ampligraph_amd.discovery import find_duplicates

    model, X = _reference_toy_model()
    entities, relations = set("a b c d e f".split()), set("x y z".split())

    def asserts(tol, dups, ent_rel, subspace):
        assert tol > 0.0
        assert len(dups) <= len(ent_rel)
        assert all(len(d) <= len(ent_rel) for d in dups)
        assert all(d.issubset(subspace) for d in dups)

    dups, tol = find_duplicates(X, model, mode="t", tolerance="auto", expected_fraction_duplicates=0.5, verbose=True)
    asserts(tol, dups, X, {tuple(x) for x in X})
    dups, tol = find_duplicates(X, model, mode="t", tolerance=1.0, verbose=True)
    assert tol == 1.0
    asserts(tol, dups, X, {tuple(x) for x in X})
    dups, tol = find_duplicates(np.unique(X[:, 0]), model, mode="e", tolerance="auto", expected_fraction_duplicates=0.5, verbose=True)
    asserts(tol, dups, entities, entities)
    dups, tol = find_duplicates(np.unique(X[:, 2]), model, mode="e", tolerance="auto", expected_fraction_duplicates=0.5, verbose=True)
    asserts(tol, dups, entities, entities)
    dups, tol = find_duplicates(np.unique(X[:, 1]), model, mode="r", tolerance="auto", expected_fraction_duplicates=0.5, verbose=True)
    asserts(tol, dups, relations, relations)
    for args in ((X, "hah"), (X, "e"), (X, "r"), (np.unique(X[:, 0]), "t")):
        with pytest.raises(ValueError):
            find_duplicates(args[0], model, mode=args[1], verbose=True)


def test_reference_find_clusters(gpu_lib):
    """tests/ampligraph/discovery/test_discovery.py::test_find_clusters of the reference, restated."""
    from sklearn.cluster import DBSCAN

    from ampligraph_amd.discovery import find_clusters

    model, X = _reference_toy_model(batch_size=1)
    X = X[:8]
    algo = DBSCAN(eps=1e-3, min_samples=1)
    assert np.array_equal(find_clusters(X, model, algo, mode="t"), np.arange(8))
    assert np.array_equal(find_clusters(np.unique(X[:, 0]), model, algo, mode="e"), np.arange(4))
    assert np.array_equal(find_clusters(np.unique(X[:, 1]), model, algo, mode="r"), np.arange(2))
    assert np.array_equal(find_clusters(np.unique(X[:, 2]), model, algo, mode="e"), np.arange(5))
    assert find_clusters(np.unique(X[:, 0]), model).shape == (4,)   # default: DBSCAN()
    for args in ((X, "hah"), (X, "e"), (X, "r"), (np.unique(X[:, 0]), "t")):
        with pytest.raises(ValueError):
            find_clusters(args[0], model, algo, mode=args[1])
    with pytest.raises(ValueError, match="fit_predict"):
        find_clusters(X, model, object(), mode="t")


def test_find_duplicates_row_sharded(gpu_lib):
    """Two row-sharded engines (in-process rendezvous) return the answer of the gathered table on both ranks."""
    from test_gpu_discovery import _fit_model
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.discovery import find_duplicates

    def body(dist):
        m, X = _fit_model(dist, sharding=True)
        ents = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
        emb = m.get_embeddings(ents, "e")
        D = np.sqrt(((emb[:, None, :].astype(np.float64) - emb[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(D, np.inf)
        tol = float(np.quantile(D.min(1), 0.3))
        tol = 0.5 * (tol + np.sort(D.min(1))[np.searchsorted(np.sort(D.min(1)), tol, side="right")])   # a gap between two rows
        got = find_duplicates(ents, m, mode="e", tolerance=tol)[0]
        auto = find_duplicates(ents, m, mode="e")
        return got, _ref_dups(emb, ents.tolist(), "euclidean", tol), auto

    res = ThreadedWorld(2).run(body)
    assert res[0][0] == res[0][1] and res[1][0] == res[1][1]
    assert res[0][0] == res[1][0] and res[0][2] == res[1][2]
