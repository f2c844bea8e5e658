"""find_clusters' DBSCAN on the MI355X (amdkge_join_dbscan, kge_join.hip): engine.dbscan against sklearn.cluster.DBSCAN on the
downloaded matrix (labels and core mask equal as arrays, twice), a 20 000-row chain (the longest label paths), 100 000 rows with
planted dense clusters in O(n) memory, and find_clusters end to end against sklearn on get_embeddings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT32_MAX = 0x7FFFFFFF


def _engine():
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("DistMult", 4, 4, 2)


def _table(n, d, seed):
    """Gaussian mixture with integer-valued rows (exact ties, exact integer distances) and exact duplicate rows mixed in: the
    style of test_gpu_duplicates._table, with a few centres so that there are clusters to find."""
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.normal(size=(4, d))
    X = (centres[rng.integers(0, 4, n)] + rng.normal(size=(n, d)) * rng.choice([0.05, 0.3, 1.0], size=(n, 1))).astype(np.float32)
    X[::3] = rng.integers(-2, 3, size=X[::3].shape)
    if n > 5:
        X[5::17] = X[4::17][:len(X[5::17])]
    return X


def _pair_d2(X, device="cuda"):
    """Sorted fp64 squared distances of the pairs i < j (direct form, a few rows at a time)."""
    t = torch.as_tensor(X, dtype=torch.float64, device=device)
    n, d = t.shape
    step = max(1, (1 << 26) // (n * d))
    out = []
    for i in range(0, n, step):
        D = ((t[i:i + step, None, :] - t[None, :, :]) ** 2).sum(-1)
        out.append(D[torch.triu(torch.ones_like(D, dtype=torch.bool), i + 1)])
    return torch.sort(torch.cat(out)).values.cpu().numpy() if n > 1 else np.zeros(0)


def _gap_threshold(v, q):
    """A threshold in a gap of the sorted values v, near their q-quantile: no value within 1e-4 (relative) of it -- the fp32 chain's
    bound (d + 2) 2^-24 is below that for d <= 1200.  Moves to the next gap upwards; the gap above the largest value always exists."""
    if len(v) == 0:
        return 1.0
    w = np.concatenate([v, [4.0 * v[-1] + 1.0]])
    k = int(q * (len(v) - 1))
    while (w[k + 1] - w[k]) <= 4e-4 * w[k + 1]:
        k += 1   # (ends at the appended value at the latest)
    thr = 0.5 * (w[k] + w[k + 1])
    assert not np.any(np.abs(v - thr) <= 1e-4 * thr)
    return float(thr)


QUANTILES = (0.0005, 0.004, 0.03, 0.3)
NS, DS = (1, 2, 63, 64, 65, 1000, 4097), (1, 3, 4, 10, 400, 1200)


def _case(n, d, device="cuda"):
    """The table of grid point (n, d) and its three (eps, min_samples): eps in a gap of the fp64 pair distances."""
    X = _table(n, d, n * 7 + d)
    v = _pair_d2(X, device)
    return X, [(float(np.sqrt(_gap_threshold(v, QUANTILES[(qi + n + d) % len(QUANTILES)]))), ms) for qi, ms in enumerate((1, 2, 5))]


def _sklearn(X, eps, min_samples):
    from sklearn.cluster import DBSCAN

    want = DBSCAN(eps=eps, min_samples=min_samples).fit(X.astype(np.float64))
    core = np.zeros(len(X), dtype=bool)
    core[want.core_sample_indices_] = True
    return want.labels_, core


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_dbscan_matches_sklearn(gpu_lib, n, d):
    eng = _engine()
    X, params = _case(n, d)
    Xd = torch.as_tensor(X).cuda()
    for eps, min_samples in params:
        want, want_core = _sklearn(X, eps, min_samples)
        labels, core, ncl = eng.dbscan(Xd, eps * eps, min_samples)
        assert labels.dtype == torch.int32 and core.dtype == torch.bool and labels.is_cuda and core.is_cuda and ncl.is_cuda
        got, got_core = labels.cpu().numpy(), core.cpu().numpy()
        print("n %d d %d min_samples %d eps %.6g: clusters %d, noise %d, border %d; label mismatches %d, core mismatches %d" % (
            n, d, min_samples, eps, want.max() + 1, (want < 0).sum(), ((want >= 0) & ~want_core).sum(), (got != want).sum(), (got_core != want_core).sum()))
        assert np.array_equal(got_core, want_core)
        assert np.array_equal(got, want)
        assert int(ncl.item()) == want.max() + 1
        again = eng.dbscan(Xd, eps * eps, min_samples)
        assert torch.equal(again[0], labels) and torch.equal(again[1], core) and torch.equal(again[2], ncl)


def test_dbscan_grid_contains_noise_border_and_clusters(gpu_lib):
    """The grid above as a whole holds noise rows, border rows and at least three clusters: shown on its points up to n = 1000
    (the same tables and parameters, sklearn's side only)."""
    noise = border = clusters = 0
    for n in NS[:-1]:
        for d in DS:
            X, params = _case(n, d)
            for eps, min_samples in params:
                want, core = _sklearn(X, eps, min_samples)
                noise += int((want < 0).sum())
                border += int(((want >= 0) & ~core).sum())
                clusters = max(clusters, int(want.max()) + 1)
    assert noise > 0 and border > 0 and clusters >= 3, (noise, border, clusters)


def test_workspace_state_matches_the_labelling_rule(gpu_lib):
    """The three arrays the passes leave in the workspace (include/amdkge.h), through discovery.dbscan_labels, give the kernel's labels."""
    from ampligraph_amd.discovery import dbscan_labels

    eng = _engine()
    n = 3000
    X = _table(n, 3, 5)
    thr = _gap_threshold(_pair_d2(X), 0.002)
    labels, core, ncl = eng.dbscan(torch.as_tensor(X).cuda(), thr, 4)
    work = eng._bufs["join_dbscan"]
    parent, border = work[n:2 * n], work[2 * n:3 * n]
    assert torch.equal(dbscan_labels(core, parent, border), labels.to(torch.int64))
    assert bool((core & (labels >= 0)).any()) and bool((~core & (labels >= 0)).any()) and bool((labels < 0).any()) and int(ncl.item()) >= 3
    roots = parent[core]
    assert bool((roots <= torch.nonzero(core).reshape(-1)).all()) and bool(core[roots.to(torch.int64)].all())


def test_chain_cluster(gpu_lib):
    """20 000 rows on a line, 0.9 eps apart, in shuffled order: one cluster whose union-find paths are as long as they get."""
    eng = _engine()
    n, eps = 20_000, 1.0
    rng = np.random.default_rng(1)
    order = rng.permutation(n)
    X = np.zeros((n, 2), dtype=np.float32)
    X[:, 0] = (0.9 * eps * order).astype(np.float32)   # (0.9 k is within 1e-3 of its fp32 value up to 18 000: neighbours 0.9, next 1.8)
    X[:, 1] = 0.25
    Xd = torch.as_tensor(X).cuda()
    labels, core, ncl = eng.dbscan(Xd, eps * eps, 3)   # inner rows have three neighbours (themselves included), the two ends two
    ends = np.isin(order, [0, n - 1])
    assert int(ncl.item()) == 1 and np.array_equal(labels.cpu().numpy(), np.zeros(n, dtype=np.int32))
    assert np.array_equal(core.cpu().numpy(), ~ends)
    labels, core, ncl = eng.dbscan(Xd, eps * eps, 2)
    assert int(ncl.item()) == 1 and bool((labels == 0).all()) and bool(core.all())
    labels, core, ncl = eng.dbscan(Xd, 0.5 * eps * eps, 1)   # below the spacing: every row its own cluster, numbered in row order
    assert int(ncl.item()) == n and torch.equal(labels.cpu(), torch.arange(n, dtype=torch.int32))


def test_large_n_planted_clusters_in_linear_memory(gpu_lib):
    """n = 100 000, d = 64: 20 planted clusters of 4 000 rows (1.6e8 pairs within eps: 400 times a 4 n pair buffer) plus 20 000
    isolated rows.  The labels are the planted partition, numbered by lowest row; the peak allocation grows by O(n) only."""
    eng = _engine()
    rng = np.random.default_rng(0)
    n, d, k, per = 100_000, 64, 20, 4_000
    planted = np.concatenate([np.repeat(np.arange(k), per), np.full(n - k * per, -1)])
    planted = planted[rng.permutation(n)]
    centres = 3.0 * rng.normal(size=(k, d))
    X = 3.0 * rng.normal(size=(n, d))                       # isolated rows: d2 ~ 2 * 64 * 9 between any two
    m = planted >= 0
    X[m] = centres[planted[m]] + 0.05 * rng.normal(size=(int(m.sum()), d))   # within a cluster: d2 ~ 2 * 64 * 0.0025 = 0.32
    X = X.astype(np.float32)
    thr = 0.6
    # host union-find over the planted ids: rows of one id are one component, numbered by their lowest row
    parent = np.arange(n)
    first = {}
    for i in np.flatnonzero(m):
        parent[i] = first.setdefault(int(planted[i]), i)
    roots = np.flatnonzero(m & (parent == np.arange(n)))
    want = np.where(m, np.searchsorted(roots, parent), -1)
    Xd = torch.as_tensor(X).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, core, ncl = eng.dbscan(Xd, thr, 5)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print("peak allocation beside the input matrix: %d bytes = %.1f n" % (grown, grown / n))
    assert grown < 64 * n   # (the matrix itself is in `base`: below the input matrix plus 64 n bytes)
    assert int(ncl.item()) == k
    assert np.array_equal(core.cpu().numpy(), m)
    assert np.array_equal(labels.cpu().numpy(), want)
    sample = rng.choice(np.flatnonzero(planted == 0), 200, replace=False)   # the planted geometry is what the comments say
    D = ((X[sample, None, :].astype(np.float64) - X[None, sample, :]) ** 2).sum(-1)
    assert D.max() < thr


# ------------------------------------------------------------------------------------------------------------- public API
def _planted_model(seed, fitted=None):
    """test_gpu_duplicates._planted_model's tables without its zero-norm row (that row sends a cosine call to sklearn)."""
    from test_gpu_discovery import _fit_model

    m, X = fitted or _fit_model()
    eng = m._engine
    rng = np.random.default_rng(seed)
    ent = rng.normal(size=(eng.n_ents, eng.K)).astype(np.float32)
    rel = rng.normal(size=(eng.n_rels, eng.K)).astype(np.float32)
    p = rng.choice(eng.n_ents, 24, replace=False)
    ent[p[12:]] = ent[p[:12]] + 3e-3 * rng.normal(size=(12, eng.K)).astype(np.float32)
    rel[1] = rel[0] + 3e-3 * rng.normal(size=eng.K).astype(np.float32)
    eng.set_tables(ent, rel)
    m._planted_rows = p
    return m, X


def _spy(m):
    calls = []
    real = m._engine.dbscan

    def dbscan(X, thr, min_samples):
        calls.append((float(thr), int(min_samples)))
        return real(X, thr, min_samples)

    m._engine.dbscan = dbscan
    return calls


def _distances(emb, metric):
    from sklearn.metrics import pairwise_distances

    D = pairwise_distances(emb.astype(np.float64), metric=metric)
    return np.sort(D[np.triu_indices(len(emb), 1)])


@pytest.mark.parametrize("mode", ["e", "r", "t"])
@pytest.mark.parametrize("algo", ["none", "euclidean", "cosine"])
def test_find_clusters_matches_sklearn(gpu_lib, mode, algo):
    from sklearn.cluster import DBSCAN
    from test_gpu_duplicates import _inputs

    from ampligraph_amd.discovery import find_clusters

    fitted = None
    for seed in range(20):   # planted tables whose distances keep the margin at DBSCAN()'s own eps = 0.5
        m, X = fitted = _planted_model(seed, fitted)
        Xin, emb, _ = _inputs(m, X, mode)
        v = _distances(emb, "euclidean" if algo == "none" else algo)
        if algo != "none" or not np.any(np.abs(v - 0.5) <= 1e-4 * 0.5):
            break
    else:
        pytest.fail("no planted table keeps the margin")
    calls = _spy(m)
    if algo == "none":
        want = DBSCAN().fit(emb)
        got = find_clusters(Xin, m, mode=mode)
        assert calls == [(0.25, 5)]
    else:
        # a gap of the pair distances wide enough for fp32 unit rows as well: near the 3 % quantile, far from the planted 1e-2 pairs
        eps = _gap_threshold(v, 0.03)
        given = DBSCAN(eps=eps, min_samples=3, metric=algo)
        want = DBSCAN(eps=eps, min_samples=3, metric=algo).fit(emb)
        got = find_clusters(Xin, m, given, mode=mode)
        assert calls == [(2 * eps if algo == "cosine" else eps * eps, 3)]
        assert got is given.labels_ and given.labels_.dtype == np.int64
        assert np.array_equal(given.core_sample_indices_, want.core_sample_indices_)
        assert np.array_equal(given.components_, want.components_) and given.n_features_in_ == emb.shape[1]
    print("mode %s algo %s: clusters %d, noise %d, label mismatches %d" % (mode, algo, want.labels_.max() + 1, (want.labels_ < 0).sum(), (got != want.labels_).sum()))
    assert np.array_equal(got, want.labels_)


def test_other_objects_and_parameters_stay_on_the_host(gpu_lib):
    from sklearn.cluster import DBSCAN, KMeans
    from test_gpu_duplicates import _inputs
    from test_gpu_duplicates import _planted_model as _with_zero_row

    from ampligraph_amd.discovery import find_clusters

    class Recorder:
        def fit_predict(self, X):
            self.seen = X
            return np.arange(len(X))

    m, X = _planted_model(0)
    Xin, emb, _ = _inputs(m, X, "e")
    calls = _spy(m)
    rec = Recorder()
    assert np.array_equal(find_clusters(Xin, m, rec), np.arange(len(emb)))
    assert isinstance(rec.seen, np.ndarray) and np.array_equal(rec.seen, emb)
    km = find_clusters(Xin, m, KMeans(n_clusters=3, n_init=2, random_state=0))
    assert np.array_equal(km, KMeans(n_clusters=3, n_init=2, random_state=0).fit_predict(emb))
    for kw in ({"metric": "manhattan", "eps": 3.0}, {"metric": "minkowski", "p": 1, "eps": 3.0}, {"metric": "euclidean", "metric_params": {}}):
        assert np.array_equal(find_clusters(Xin, m, DBSCAN(min_samples=2, **kw)), DBSCAN(min_samples=2, **kw).fit_predict(emb))
    assert calls == []
    m, X = _with_zero_row(0, (m, X))   # a zero-norm row: cosine distance 1 to every other row in sklearn, on the host
    Xin, emb, _ = _inputs(m, X, "e")
    calls = _spy(m)
    got = find_clusters(Xin, m, DBSCAN(eps=0.3, min_samples=2, metric="cosine"))
    assert calls == [] and np.array_equal(got, DBSCAN(eps=0.3, min_samples=2, metric="cosine").fit_predict(emb))


def test_find_clusters_row_sharded(gpu_lib):
    """Two row-sharded engines (in-process rendezvous) return the labels of the gathered table on both ranks."""
    from sklearn.cluster import DBSCAN
    from test_gpu_discovery import _fit_model
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.discovery import find_clusters

    def body(dist):
        m, X = _fit_model(dist, sharding=True)
        ents = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
        emb = m.get_embeddings(ents, "e")
        eps = _gap_threshold(_distances(emb, "euclidean"), 0.03)
        calls = _spy(m)
        algo = DBSCAN(eps=eps, min_samples=3)
        got = find_clusters(ents, m, algo)
        return got, DBSCAN(eps=eps, min_samples=3).fit(emb).labels_, len(calls)

    res = ThreadedWorld(2).run(body)
    for got, want, n_calls in res:
        assert n_calls == 1 and np.array_equal(got, want)
    assert np.array_equal(res[0][0], res[1][0])
