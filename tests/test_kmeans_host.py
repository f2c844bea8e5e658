"""Host side of the device KMeans (ampligraph_amd/discovery.py, kge_kmeans.hip) without a GPU: the three C-ABI symbols and their
argument validation, the Lloyd rule the kernels implement -- restated here in numpy fp64 (lloyd_ref: stop rules, n_iter, the
empty-cluster rule, ties to the lowest centre) and compared with sklearn.cluster.KMeans; tests/test_gpu_kmeans.py holds the kernels
to the restatement --, the estimator's parameters and seeding, and the routing of find_clusters."""
import ctypes as C

import numpy as np
import pytest
import torch


# ------------------------------------------------------------------------------------------------------------ shared data and rule
def dyadic_mixture(n, d, k, sigma, seed, with_blobs=False):
    """Rows = centre + N(0, sigma), rounded to multiples of 2^-6 and clipped to |x| <= 16, float32.  2 k blobs drawn uniformly (twice
    as many as the clusters asked for: whole blobs then move between centres from one iteration to the next, which gives
    trajectories of several iterations whose rows all stay clear of ties); the blob centres differ in the first min(d, 8) columns
    (uniform in [-8, 8]), so that their mutual distances do not concentrate in the wide shapes.  Any sum of up to 2^12 such values is
    below 2^16 in magnitude and a multiple of 2^-6: 22 significant bits, exact in fp32 in any order.  The mean of a cluster is then
    float32(exact sum) / float32(count), one rounding, whatever the summation order."""
    rng = np.random.default_rng(seed)
    centres = np.zeros((2 * k, d))
    centres[:, :min(d, 8)] = rng.uniform(-8.0, 8.0, size=(2 * k, min(d, 8)))
    blobs = rng.integers(0, 2 * k, n)
    X = centres[blobs] + sigma * rng.normal(size=(n, d))
    X = np.clip(np.round(X * 64.0) / 64.0, -16.0, 16.0).astype(np.float32)
    return (X, blobs) if with_blobs else X


def sq_dists(X, Cn):
    """fp64 squared distances [n, k] in the direct form, a block of centres at a time."""
    X, Cn = np.asarray(X, dtype=np.float64), np.asarray(Cn, dtype=np.float64)
    out = np.empty((len(X), len(Cn)))
    step = max(1, (1 << 24) // max(X.size, 1))
    for c in range(0, len(Cn), step):
        out[:, c:c + step] = ((X[:, None, :] - Cn[None, c:c + step, :]) ** 2).sum(-1)
    return out


def rel_gaps(D):
    """Per row (second-best - best) / second-best of the distances D [n, k] (1 for k == 1 or a second-best of 0)."""
    if D.shape[1] < 2:
        return np.ones(len(D))
    two = np.partition(D, 1, axis=1)[:, :2]
    return np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1.0), 1.0)


def lloyd_step(X, Cn, labels_old):
    """One iteration: labels of the centres as they are (np.argmin: the lowest centre among equal distances), the means of the rows by
    label -- a centre without rows keeps its value --, and what the control step reads."""
    X, Cn = np.asarray(X, dtype=np.float64), np.asarray(Cn, dtype=np.float64)
    D = sq_dists(X, Cn)
    labels = D.argmin(1)
    mind2 = D[np.arange(len(X)), labels]
    counts = np.bincount(labels, minlength=len(Cn))
    new = Cn.copy()
    for c in np.flatnonzero(counts):
        new[c] = X[labels == c].sum(0) / counts[c]
    return {"labels": labels, "mind2": mind2, "inertia": float(mind2.sum()), "counts": counts, "centres": new,
            "changed": int((labels != labels_old).sum()), "shift2": float(((new - Cn) ** 2).sum()), "min_gap": float(rel_gaps(D).min())}


def lloyd_ref(X, C0, max_iter=300, tol_abs=0.0):
    """sklearn's Lloyd loop around lloyd_step -> dict(centres, labels, inertia, n_iter, done, min_gap): done = 1 when no label
    changed (n_iter > 1), else 2 when shift2 <= tol_abs, else 0 at max_iter; unless done == 1, labels and inertia are taken once
    more against the final centres.  min_gap: the smallest relative gap between a row's two nearest centres met on the way."""
    Cn, labels, done, n_iter, gap, inertia = np.asarray(C0, dtype=np.float64), np.full(len(X), -1), 0, 0, 1.0, 0.0
    for n_iter in range(1, max_iter + 1):
        s = lloyd_step(X, Cn, labels)
        Cn, labels, inertia, gap = s["centres"], s["labels"], s["inertia"], min(gap, s["min_gap"])
        if n_iter > 1 and s["changed"] == 0:
            done = 1
            break
        if s["shift2"] <= tol_abs:
            done = 2
            break
    if done != 1:
        s = lloyd_step(X, Cn, labels)
        labels, inertia, gap = s["labels"], s["inertia"], min(gap, s["min_gap"])
    return {"centres": Cn, "labels": labels, "inertia": inertia, "n_iter": n_iter, "done": done, "min_gap": gap}


def start_rows(X, k, seed, blobs=None):
    """k distinct rows of X as initial centres; with the rows' blob ids, one row from each of k distinct blobs."""
    rng = np.random.default_rng(1000 + seed)
    if blobs is None:
        return X[rng.choice(len(X), k, replace=False)].copy()
    return np.stack([X[rng.choice(np.flatnonzero(blobs == j))] for j in rng.choice(np.unique(blobs), k, replace=False)])


def clean_case(n, d, k, sigma, min_gap=1e-3, min_iter=3):
    """(seed, X, C0, trajectory) of the first seed in range(20) whose fp64 trajectory keeps every gap above min_gap, lasts at least
    min_iter iterations, stops on equal labels and never empties a cluster; None when there is none."""
    for seed in range(20):
        X, blobs = dyadic_mixture(n, d, k, sigma, seed, with_blobs=True)
        C0 = start_rows(X, k, seed, blobs)
        t = lloyd_ref(X, C0)
        if t["min_gap"] > min_gap and t["n_iter"] >= min_iter and t["done"] == 1 and len(np.unique(t["labels"])) == k:
            return seed, X, C0, t
    return None


WHOLE_RUN_SHAPES = [(300, 2, 3), (1000, 3, 6), (1000, 10, 6), (2000, 400, 6), (1500, 1200, 6)]


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_library_exports_the_kmeans_symbols_and_validates_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    names = {"amdkge_kmeans_workspace_bytes", "amdkge_kmeans_assign", "amdkge_kmeans_lloyd"}
    assert names <= set(_ffi.ABI["amdkge.h"]) and all(hasattr(lib, s) for s in names)
    buf = C.c_void_p(16)   # never dereferenced: every call below returns before touching the device

    def assign(**kw):
        order = ("x", "n", "d", "c", "k", "runs", "labels", "mind2", "stream")
        a = dict(zip(order, (buf, 5, 4, buf, 2, 1, buf, buf, None)))
        a.update(kw)
        return lib.amdkge_kmeans_assign(*[a[o] for o in order])

    def lloyd(**kw):
        order = ("x", "n", "d", "c", "k", "runs", "iters", "tol", "labels", "mind2", "state", "inertia", "work", "stream")
        a = dict(zip(order, (buf, 5, 4, buf, 2, 1, 1, 0.0, buf, buf, buf, buf, buf, None)))
        a.update(kw)
        return lib.amdkge_kmeans_lloyd(*[a[o] for o in order])

    for call in (assign, lloyd):
        for bad in ({"n": -1}, {"n": 1 << 31}, {"d": 0}, {"k": 0}, {"k": -2}, {"runs": 0}):
            assert call(**bad) == -1 and b"bad sizes" in lib.amdkge_last_error(), (call.__name__, bad)
    assert lloyd(iters=-1) == -1 and b"bad sizes" in lib.amdkge_last_error()
    assert lloyd(tol=float("nan")) == -1 and b"tol_abs" in lib.amdkge_last_error()
    assert lloyd(tol=-1e-9) == -1 and b"tol_abs" in lib.amdkge_last_error()
    for name in ("x", "c", "labels"):
        assert assign(**{name: None}) == -1 and b"NULL" in lib.amdkge_last_error(), name
    for name in ("x", "c", "labels", "mind2", "state", "inertia", "work"):
        assert lloyd(**{name: None}) == -1 and b"NULL" in lib.amdkge_last_error(), name
    # no rows: nothing to do, nothing launched
    assert assign(n=0, x=None, labels=None, mind2=None) == 0
    assert lloyd(n=0, x=None, labels=None, mind2=None, work=None) == 0
    assert lloyd(n=0, c=None) == -1 and lloyd(n=0, state=None) == -1


def test_workspace_bytes():
    from ampligraph_amd import _ffi

    ws = _ffi.lib().amdkge_kmeans_workspace_bytes
    assert ws(0, 4, 3, 2) == 0
    for bad in ((-1, 4, 3, 2), (1 << 31, 4, 3, 2), (10, 0, 3, 2), (10, 4, 0, 2), (10, 4, 3, 0), (10, -4, 3, 2)):
        assert ws(*bad) == -1, bad
    assert ws((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1) == -1   # beyond int64: refused, not wrapped
    last = 0
    for n in (1, 2, 127, 128, 129, 4097, 65536, 65537, 100_000, 1_000_000, (1 << 31) - 1):
        b = ws(n, 16, 6, 3)
        assert b > 0 and b >= last and b % 8 == 0, n
        last = b
    last = 0
    for runs in (1, 2, 5, 100, 4096):
        b = ws(14505, 400, 6, runs)
        assert b > last
        last = b
    # O(runs n) plus the partial sums: [runs][at most 256 row blocks][k][d] fp32
    n, d, k, runs = 1_000_000, 64, 64, 4
    assert runs * 256 * k * d * 4 <= ws(n, d, k, runs) <= runs * 256 * k * d * 4 + runs * n + (1 << 16)


# ------------------------------------------------------------------------------------------------------------ the Lloyd rule
@pytest.mark.parametrize("shape", [(300, 2, 3), (1000, 3, 6), (1000, 10, 6), (4097, 16, 129), (1500, 1200, 6)])
def test_lloyd_rule_reproduces_sklearn(shape):
    from sklearn.cluster import KMeans as SkKMeans

    n, d, k = shape
    compared = 0
    for sigma, seed in ((0.1, 0), (0.3, 1), (0.3, 2)):
        X, blobs = dyadic_mixture(n, d, k, sigma, seed, with_blobs=True)
        X = X.astype(np.float64)
        C0 = start_rows(X, k, seed, blobs)
        got = lloyd_ref(X, C0)
        if len(np.unique(got["labels"])) < k:
            continue   # (sklearn moves an emptied centre; the rule here keeps it: no comparison)
        want = SkKMeans(n_clusters=k, init=C0, n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(X)
        assert got["done"] == 1 and got["n_iter"] == want.n_iter_, (shape, sigma, seed)
        assert np.array_equal(got["labels"], want.labels_)
        assert np.abs(got["centres"] - want.cluster_centers_).max() <= 1e-6
        assert abs(got["inertia"] - want.inertia_) <= 1e-12 * want.inertia_
        compared += 1
    assert compared >= 2


def test_lloyd_rule_stop_rules_empty_cluster_and_ties():
    X = dyadic_mixture(400, 3, 4, 0.3, 0).astype(np.float64)
    C0 = start_rows(X, 4, 0)
    full = lloyd_ref(X, C0)
    assert full["done"] == 1 and full["n_iter"] >= 2
    # the strict stop: the last iteration changed no label, and its centres are the means of its labels
    last = lloyd_step(X, full["centres"], full["labels"])
    assert last["changed"] == 0 and np.array_equal(last["centres"], full["centres"]) and last["inertia"] == full["inertia"]
    # a huge tolerance stops after one iteration, and the labels are taken once more against the moved centres
    one = lloyd_ref(X, C0, tol_abs=1e30)
    first = lloyd_step(X, C0, np.full(len(X), -1))
    assert one["done"] == 2 and one["n_iter"] == 1 and np.array_equal(one["centres"], first["centres"])
    assert np.array_equal(one["labels"], sq_dists(X, first["centres"]).argmin(1))
    assert first["changed"] == len(X)   # (labels start at -1)
    # max_iter
    two = lloyd_ref(X, C0, max_iter=2)
    if full["n_iter"] > 2:
        assert two["done"] == 0 and two["n_iter"] == 2
    # a centre far from every row has no rows and keeps its value
    far = np.concatenate([C0, np.full((1, 3), 1000.0)])
    s = lloyd_step(X, far, np.full(len(X), -1))
    assert s["counts"][4] == 0 and np.array_equal(s["centres"][4], far[4]) and np.isfinite(s["centres"]).all()
    assert np.array_equal(lloyd_ref(X, far)["labels"], full["labels"])
    # equal distances go to the lowest centre: duplicated centres never get a row at the higher index
    dup = np.concatenate([C0[:2], C0[:2]])
    s = lloyd_step(X, dup, np.full(len(X), -1))
    assert s["counts"][2] == 0 and s["counts"][3] == 0 and s["min_gap"] == 0.0
    # integer rows halfway between two integer centres
    Xi = np.array([[0.0], [1.0], [2.0]])
    assert lloyd_step(Xi, np.array([[2.0], [0.0]]), np.full(3, -1))["labels"].tolist() == [1, 0, 0]


def test_clean_trajectories_exist_for_the_whole_run_shapes():
    """The seed search of tests/test_gpu_kmeans.py (whole runs against sklearn) finds a seed for every shape and both spreads."""
    for n, d, k in WHOLE_RUN_SHAPES:
        for sigma in (0.1, 0.3):
            assert clean_case(n, d, k, sigma) is not None, (n, d, k, sigma)


# ------------------------------------------------------------------------------------------------------------ the estimator
def test_parameter_validation():
    from ampligraph_amd.discovery import KMeans

    km = KMeans()
    assert (km.n_clusters, km.init, km.n_init, km.max_iter, km.tol, km.random_state) == (8, "k-means++", 10, 300, 1e-4, None)
    with pytest.raises(TypeError):
        KMeans(3, "random")   # keyword-only beyond n_clusters, as in sklearn
    X = np.zeros((5, 2), dtype=np.float32)
    eng = _RecordingEngine()
    bad = [dict(n_clusters=0), dict(n_clusters=2.5), dict(n_init=0), dict(max_iter=0), dict(tol=-1.0), dict(tol=float("nan")), dict(init="kmeans"),
           dict(init=lambda X, k, rs: X[:k]), dict(init=np.zeros((2, 2)), n_clusters=2, n_init=3), dict(random_state=-1), dict(random_state="x")]
    for kw in bad:
        with pytest.raises(ValueError):
            KMeans(**{"n_clusters": 2, **kw}).fit(X, engine=eng)
    with pytest.raises(ValueError, match="n_clusters"):
        KMeans(n_clusters=6, n_init=1).fit(X, engine=eng)
    with pytest.raises(ValueError, match="shape"):
        KMeans(n_clusters=2, n_init=1, init=np.zeros((2, 3))).fit(X, engine=eng)
    with pytest.raises(ValueError, match="shape"):
        KMeans(n_clusters=2, n_init=1, init=np.zeros((3, 2))).fit(X, engine=eng)
    for Xbad in (np.array([[0.0, np.nan], [1.0, 2.0]]), np.array([[np.inf, 0.0], [1.0, 2.0]]), np.zeros((0, 2)), np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            KMeans(n_clusters=1, n_init=1).fit(Xbad, engine=eng)
    with pytest.raises(ValueError, match="not fitted"):
        KMeans().predict(X)
    assert eng.calls == []


def test_from_sklearn():
    from sklearn.cluster import KMeans as SkKMeans

    from ampligraph_amd.discovery import KMeans

    km = KMeans.from_sklearn(SkKMeans(n_clusters=6, n_init=100, max_iter=500, tol=1e-3, random_state=7, init="random"))
    assert (km.n_clusters, km.init, km.n_init, km.max_iter, km.tol, km.random_state) == (6, "random", 100, 500, 1e-3, 7)
    C0 = np.arange(6.0).reshape(3, 2)
    km = KMeans.from_sklearn(SkKMeans(n_clusters=3, init=C0, n_init=1))
    assert km.init is C0 and km.n_init == 1 and km.random_state is None
    assert KMeans.from_sklearn(SkKMeans(n_clusters=3, n_init="auto")).n_init == 1
    assert KMeans.from_sklearn(SkKMeans(n_clusters=3, n_init="auto", init="random")).n_init == 10
    with pytest.raises(ValueError, match="elkan"):
        KMeans.from_sklearn(SkKMeans(algorithm="elkan"))
    with pytest.raises(ValueError, match="callable"):
        KMeans.from_sklearn(SkKMeans(init=lambda X, k, rs: X[:k]))


class _RecordingEngine:
    """Stands in for KgeEngine on CPU tensors: records kmeans calls and answers them and kmeans_assign from the fp64 rule."""

    def __init__(self, rel=None):
        self.rel, self.calls, self.dbscan_calls = rel, [], []

    def unpack(self, rows):
        return rows

    def dbscan(self, X, thr, min_samples):
        self.dbscan_calls.append(tuple(X.shape))
        raise AssertionError("DBSCAN on a KMeans call")

    def kmeans_assign(self, X, centres):
        Xn, Cn = X.double().numpy(), centres.double().numpy()
        if Cn.ndim == 2:
            D = sq_dists(Xn, Cn)
            return torch.as_tensor(D.argmin(1).astype(np.int32)), torch.as_tensor(D.min(1).astype(np.float32))
        D = [sq_dists(Xn, c) for c in Cn]
        return torch.as_tensor(np.stack([x.argmin(1) for x in D]).astype(np.int32)), torch.as_tensor(np.stack([x.min(1) for x in D]).astype(np.float32))

    def kmeans(self, X, centres0, max_iter, tol_abs, check_every=8):
        self.calls.append((tuple(X.shape), tuple(centres0.shape), int(max_iter), float(tol_abs), X.dtype))
        runs = [lloyd_ref(X.double().numpy(), c, max_iter, tol_abs) for c in centres0.double().numpy()]
        t = lambda key, dt: torch.as_tensor(np.stack([np.asarray(r[key]) for r in runs]).astype(dt))   # noqa: E731
        return t("centres", np.float32), t("labels", np.int32), t("inertia", np.float64), t("n_iter", np.int32), t("done", np.int32)


def test_seeding_of_a_run_does_not_depend_on_n_init():
    from ampligraph_amd.discovery import KMeans, _kmeans_plusplus

    X = torch.as_tensor(dyadic_mixture(500, 3, 5, 0.3, 4))
    eng = _RecordingEngine()
    c4 = _kmeans_plusplus(eng, X, 5, 4, seed=11)
    c2 = _kmeans_plusplus(eng, X, 5, 2, seed=11)
    assert c4.shape == (4, 5, 3) and torch.equal(c4[:2], c2) and torch.equal(c4, _kmeans_plusplus(eng, X, 5, 4, seed=11))
    assert not torch.equal(c4[0], c4[1]) and not torch.equal(c4, _kmeans_plusplus(eng, X, 5, 4, seed=12))
    rows = {tuple(r) for r in X.numpy().tolist()}
    assert all(tuple(c) in rows for c in c4.reshape(-1, 3).numpy().tolist())      # every centre is a row of X
    # the documented draws: the first centre is row floor(u_0 n) of the run's own generator
    u = np.random.default_rng(np.random.SeedSequence(11, spawn_key=(3,))).random(5)
    assert torch.equal(c4[3, 0], X[int(u[0] * 500)])
    # groups of exact duplicates: D^2 sampling gives an already chosen group probability 0
    G = torch.as_tensor(np.repeat(np.arange(6.0, dtype=np.float32)[:, None] * np.ones((1, 2), np.float32), 7, axis=0))
    for seed in range(10):
        c = _kmeans_plusplus(eng, G, 6, 3, seed=seed)
        assert all(len(set(run[:, 0].tolist())) == 6 for run in c)
    # all rows equal: the total is 0, and step j takes row floor(u_j n)
    Z = torch.zeros(9, 2)
    assert torch.equal(_kmeans_plusplus(eng, Z, 3, 2, seed=0), torch.zeros(2, 3, 2))
    # "random": k distinct rows per run, run r independent of n_init
    a = KMeans(5, init="random", n_init=4)._initial_centres(eng, X, 3)
    b = KMeans(5, init="random", n_init=2)._initial_centres(eng, X, 3)
    assert torch.equal(a[:2], b) and all(len({tuple(r) for r in run.numpy().tolist()}) == 5 for run in a)


def test_estimator_on_the_recording_engine():
    """fit's plumbing on host tensors: tol, the best run, the attributes."""
    from ampligraph_amd.discovery import KMeans

    X = dyadic_mixture(600, 4, 3, 0.2, 2)
    eng = _RecordingEngine()
    km = KMeans(3, n_init=5, max_iter=50, tol=1e-3, random_state=0).fit(X, engine=eng)
    (xs, cs, mi, tol_abs, dt), = eng.calls
    assert xs == (600, 4) and cs == (5, 3, 4) and mi == 50 and dt == torch.float32
    assert tol_abs == pytest.approx(1e-3 * X.astype(np.float64).var(0).mean(), rel=1e-12)
    assert km.cluster_centers_.dtype == np.float32 and km.cluster_centers_.shape == (3, 4)
    assert km.labels_.dtype == np.int32 and km.labels_.shape == (600,) and km.n_features_in_ == 4 and km.n_iter_ >= 1
    runs = [lloyd_ref(X, c, 50, tol_abs) for c in km._initial_centres(eng, torch.as_tensor(X), 0).numpy()]
    best = int(np.argmin([r["inertia"] for r in runs]))
    assert km.inertia_ == runs[best]["inertia"] and np.array_equal(km.labels_, runs[best]["labels"])
    assert np.array_equal(km.predict(X), km.labels_)


# ------------------------------------------------------------------------------------------------------------ routing
class _Indexer:
    def get_indexes(self, labels, kind, order="raw2ind"):
        return np.arange(len(labels))


class _Placement:
    def __init__(self, table):
        self.table = table

    def entity_table(self):
        return self.table


class _Model:
    is_fitted = True

    def __init__(self, E, engine=None):
        self.data_indexer = _Indexer()
        self._placement = _Placement(torch.as_tensor(E))
        self._engine = engine or _RecordingEngine(torch.as_tensor(E))


def test_find_clusters_routes_our_kmeans_to_the_engine_and_sklearns_to_the_host(monkeypatch):
    from sklearn.cluster import KMeans as SkKMeans

    from ampligraph_amd.discovery import KMeans, find_clusters

    E = dyadic_mixture(90, 4, 3, 0.25, 3)
    names = np.array(["e%d" % i for i in range(len(E))])
    m = _Model(E)
    km = KMeans(3, n_init=2, random_state=1)
    monkeypatch.setattr(KMeans, "fit_predict", lambda self, X, y=None: pytest.fail("fit_predict on downloaded rows"))
    got = find_clusters(names, m, km)
    assert [c[:2] for c in m._engine.calls] == [(E.shape, (2, 3, 4))] and m._engine.dbscan_calls == []
    assert got.dtype == np.int64 and np.array_equal(got, km.labels_) and km.labels_.dtype == np.int32
    # sklearn's own object: the host, on a numpy array, with sklearn's labels
    seen = []
    real = SkKMeans.fit_predict
    monkeypatch.setattr(SkKMeans, "fit_predict", lambda self, X, y=None, sample_weight=None: (seen.append(X), real(self, X))[1])
    m = _Model(E)
    got = find_clusters(names, m, SkKMeans(n_clusters=3, n_init=2, random_state=0))
    assert m._engine.calls == [] and len(seen) == 1 and isinstance(seen[0], np.ndarray) and np.array_equal(seen[0], E)
    assert np.array_equal(got, SkKMeans(n_clusters=3, n_init=2, random_state=0).fit_predict(E))
    # no rows
    m = _Model(E)
    with pytest.raises(ValueError):
        find_clusters(np.array([], dtype=str), m, KMeans(3))
    assert m._engine.calls == []


def test_device_branch_is_never_computed_on_the_host():
    """Without a GPU the estimator raises: there is no host implementation behind it, standalone or through find_clusters."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.discovery import KMeans, find_clusters
    from ampligraph_amd.engine import KgeEngine

    if torch.cuda.is_available():
        return   # (with a GPU the branch runs there: tests/test_gpu_kmeans.py)
    E = dyadic_mixture(90, 4, 3, 0.25, 3)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        KMeans(3, n_init=1, random_state=0).fit(E)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        KMeans(3, n_init=1, random_state=0).fit_predict(E)
    eng = object.__new__(KgeEngine)   # the engine's kmeans over the real library, with host tensors in place of device memory
    eng.lib, eng.device, eng._bufs = _ffi.lib(), torch.device("cpu"), {}
    eng.unpack, eng.rel = (lambda rows: rows), torch.as_tensor(E)
    with pytest.raises(RuntimeError):   # (torch's "No HIP GPUs are available", or the library's AMDKGE_EHIP as an AmdKgeError)
        find_clusters(np.arange(len(E)).astype(str), _Model(E, eng), KMeans(3, n_init=1, random_state=0))
