"""Host side of find_clusters' device DBSCAN (ampligraph_amd/discovery.py, kge_join.hip) without a GPU: the two C-ABI symbols and
their argument validation, the labelling rule (discovery.dbscan_labels, the torch restatement of the label kernels) against
sklearn.cluster.DBSCAN on count / union / border results built by fp64 brute force, and the routing of find_clusters: which
clustering objects take the device path, and that the device path is never computed on the host."""
import ctypes as C

import numpy as np
import pytest
import torch
from sklearn.cluster import DBSCAN

INT32_MAX = 0x7FFFFFFF


def test_library_exports_the_dbscan_symbols_and_validates_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    assert {"amdkge_join_dbscan_workspace_bytes", "amdkge_join_dbscan"} <= set(_ffi.ABI["amdkge.h"])
    assert hasattr(lib, "amdkge_join_dbscan") and hasattr(lib, "amdkge_join_dbscan_workspace_bytes")
    buf = C.c_void_p(16)   # never dereferenced: every call below returns before touching the device
    ok = (buf, 5, 4, 1.0, 2, buf, buf, buf, buf, None)

    def call(**kw):
        names = ("x", "n", "d", "thr", "ms", "labels", "core", "ncl", "work", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.amdkge_join_dbscan(*[a[k] for k in names])

    assert call(n=-1) == -1 and b"bad sizes" in lib.amdkge_last_error()
    assert call(n=1 << 31) == -1 and b"bad sizes" in lib.amdkge_last_error()
    assert call(d=0) == -1 and b"bad sizes" in lib.amdkge_last_error()
    assert call(ms=0) == -1 and b"bad sizes" in lib.amdkge_last_error()
    assert call(ms=-3) == -1
    assert call(thr=float("nan")) == -1 and b"NaN" in lib.amdkge_last_error()
    for name in ("x", "labels", "core", "ncl", "work"):
        assert call(**{name: None}) == -1 and b"NULL" in lib.amdkge_last_error(), name
    assert call(n=0, x=None, labels=None, core=None, work=None, ncl=None) == -1   # n == 0 still writes *d_n_clusters


def test_workspace_bytes_is_positive_and_linear():
    from ampligraph_amd import _ffi

    ws = _ffi.lib().amdkge_join_dbscan_workspace_bytes
    assert ws(0) == 0 and ws(-1) == -1 and ws(1 << 31) == -1
    per_row = ws(1)
    assert per_row > 0 and per_row == 12   # three int32 arrays of n: O(n), whatever the pair count
    for n in (2, 63, 4097, 100_000, (1 << 31) - 1):
        assert ws(n) == per_row * n


# ------------------------------------------------------------------------------------------------------------ labelling rule
def _mixture(rng, n, d, k, spread, noise):
    """k Gaussian blobs plus uniform background rows, shuffled (so that a cluster's lowest core row is anywhere)."""
    centres = rng.uniform(-4, 4, size=(k, d))
    m = n - int(noise * n)
    X = np.concatenate([centres[rng.integers(0, k, m)] + spread * rng.normal(size=(m, d)), rng.uniform(-5, 5, size=(n - m, d))])
    return X[rng.permutation(n)]


def _brute_passes(X, eps, min_samples):
    """What the three device passes leave, by fp64 brute force: core [n] bool, parent [n] (core rows: the lowest core row of their
    component; others: themselves), border [n] (non-core rows: the lowest such root among the core rows within eps, else INT32_MAX)."""
    n = len(X)
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    hit = D2 <= eps * eps
    core = hit.sum(1) >= min_samples
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(hit, 1))):
        if core[i] and core[j]:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    parent = np.array([find(i) for i in range(n)])
    border = np.full(n, INT32_MAX, dtype=np.int64)
    for i in np.flatnonzero(~core):
        near = np.flatnonzero(hit[i] & core)
        if len(near):
            border[i] = parent[near].min()
    return core, parent, border, hit


def test_labelling_rule_reproduces_sklearn():
    from ampligraph_amd.discovery import dbscan_labels

    rng = np.random.default_rng(0)
    n_border = n_multi = n_noise = 0
    for case in range(60):
        n = int(rng.integers(20, 160))
        d = int(rng.integers(1, 5))
        X = _mixture(rng, n, d, int(rng.integers(1, 6)), rng.uniform(0.1, 0.5), rng.uniform(0.0, 0.4))
        eps, ms = float(rng.uniform(0.2, 0.9)), int(rng.integers(1, 7))
        D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
        if np.any(np.abs(D - eps) <= 1e-9 * eps):   # (sklearn's own fp64 distances differ from these in the last bits)
            eps *= 1.0 + 1e-6
        core, parent, border, _ = _brute_passes(X, eps, ms)
        for algorithm in ("auto", "brute"):
            ref = DBSCAN(eps=eps, min_samples=ms, algorithm=algorithm).fit(X)
            got = dbscan_labels(torch.as_tensor(core), torch.as_tensor(parent.astype(np.int32)), torch.as_tensor(border.astype(np.int32)))
            assert got.dtype == torch.int64
            assert np.array_equal(got.numpy(), ref.labels_), (case, algorithm)
            assert np.array_equal(np.flatnonzero(core), ref.core_sample_indices_)
        n_border += int(((ref.labels_ >= 0) & ~core).sum())
        n_noise += int((ref.labels_ < 0).sum())
        n_multi += int(ref.labels_.max() >= 1)
    assert n_border > 50 and n_multi > 10 and n_noise > 50, (n_border, n_multi, n_noise)


def test_labelling_rule_edge_cases():
    from ampligraph_amd.discovery import dbscan_labels

    t = torch.as_tensor
    # nothing is core: all noise
    assert dbscan_labels(t([False, False]), t([0, 1]), t([INT32_MAX, INT32_MAX])).tolist() == [-1, -1]
    # row 0 is a border row of the cluster rooted at row 2; rows 1 and 3 form the cluster rooted at 1, which is numbered first
    assert dbscan_labels(t([False, True, True, True]), t([0, 1, 2, 1]), t([2, INT32_MAX, INT32_MAX, INT32_MAX])).tolist() == [1, 0, 1, 0]
    assert dbscan_labels(t([True]), t([0]), t([INT32_MAX])).tolist() == [0]
    assert dbscan_labels(torch.zeros(0, dtype=torch.bool), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)).shape == (0,)


# ------------------------------------------------------------------------------------------------------------ routing
class _Indexer:
    def get_indexes(self, labels, kind, order="raw2ind"):
        return np.arange(len(labels))


class _Placement:
    def __init__(self, table):
        self.table = table

    def entity_table(self):
        return self.table


class _RecordingEngine:
    """Stands in for KgeEngine: records dbscan calls and answers them from fp64 brute force (CPU tensors)."""

    def __init__(self, rel):
        self.rel, self.calls = rel, []

    def unpack(self, rows):
        return rows

    def dbscan(self, X, thr, min_samples):
        self.calls.append((tuple(X.shape), float(thr), int(min_samples)))
        Xn = X.double().numpy()
        hit = ((Xn[:, None, :] - Xn[None, :, :]) ** 2).sum(-1) <= thr
        core = hit.sum(1) >= min_samples
        labels = DBSCAN(eps=0.5, min_samples=min_samples, metric="precomputed").fit(np.where(hit, 0.0, 1.0)).labels_
        return torch.as_tensor(labels.astype(np.int32)), torch.as_tensor(core), torch.as_tensor([int(labels.max()) + 1], dtype=torch.int32)


class _Model:
    is_fitted = True

    def __init__(self, E, engine=None):
        self.data_indexer = _Indexer()
        self._placement = _Placement(torch.as_tensor(E))
        self._engine = engine or _RecordingEngine(torch.as_tensor(E))


class _Recorder:
    """A clustering object that is not a DBSCAN: must get the downloaded embeddings through fit_predict."""

    def __init__(self):
        self.seen = None

    def fit_predict(self, X):
        self.seen = X
        return np.zeros(len(X), dtype=np.int64)


def _rows(seed=3, n=90, d=4):
    rng = np.random.default_rng(seed)
    return _mixture(rng, n, d, 3, 0.25, 0.2).astype(np.float32)


def test_find_clusters_routes_supported_dbscan_to_the_engine(monkeypatch):
    from ampligraph_amd.discovery import find_clusters

    E = _rows()
    names = np.array(["e%d" % i for i in range(len(E))])
    monkeypatch.setattr(DBSCAN, "fit_predict", lambda self, X, y=None, sample_weight=None: pytest.fail("host fit_predict on the device path"))
    m = _Model(E)
    labels = find_clusters(names, m)                                 # None: DBSCAN() = eps 0.5, min_samples 5, euclidean
    assert m._engine.calls == [(E.shape, 0.25, 5)] and labels.dtype == np.int64 and labels.shape == (len(E),)
    for kw, thr in (({"eps": 0.7, "min_samples": 3}, 0.7 * 0.7), ({"eps": 0.7, "metric": "l2", "algorithm": "kd_tree", "leaf_size": 3, "n_jobs": 2}, 0.7 * 0.7),
                    ({"eps": 0.6, "metric": "minkowski"}, 0.36), ({"eps": 0.6, "metric": "minkowski", "p": 2}, 0.36),
                    ({"eps": 0.05, "metric": "cosine", "min_samples": 2}, 2 * 0.05)):
        m = _Model(E)
        algo = DBSCAN(**kw)
        out = find_clusters(names, m, algo)
        assert m._engine.calls == [(E.shape, thr, algo.min_samples)], kw
        assert out is algo.labels_ and out.dtype == np.int64
        assert algo.n_features_in_ == E.shape[1]
        core = np.zeros(len(E), dtype=bool)
        core[algo.core_sample_indices_] = True
        assert np.array_equal(algo.components_, E[core]) and algo.components_.dtype == np.float32


def test_cosine_runs_on_unit_rows():
    from ampligraph_amd.discovery import find_clusters

    E = _rows()
    seen = {}

    class Eng(_RecordingEngine):
        def dbscan(self, X, thr, min_samples):
            seen["norms"] = torch.linalg.vector_norm(X, dim=1)
            return super().dbscan(X, thr, min_samples)

    algo = DBSCAN(eps=0.05, metric="cosine", min_samples=2)
    got = find_clusters(np.arange(len(E)).astype(str), _Model(E, Eng(torch.as_tensor(E))), algo)
    assert torch.allclose(seen["norms"], torch.ones(len(E)), atol=1e-6)
    want = DBSCAN(eps=0.05, metric="cosine", min_samples=2).fit(E.astype(np.float64))
    D = 1.0 - (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float64) @ (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float64).T
    if not np.any(np.abs(D - 0.05) <= 1e-5):   # (fp32 unit rows against sklearn's fp64: compare away from the boundary)
        assert np.array_equal(got, want.labels_)


def test_find_clusters_keeps_the_host_path_for_everything_else():
    from ampligraph_amd.discovery import find_clusters

    E = _rows()
    names = np.arange(len(E)).astype(str)

    class MyDBSCAN(DBSCAN):
        pass

    unsupported = [DBSCAN(metric="manhattan"), DBSCAN(metric="minkowski", p=1), DBSCAN(metric="minkowski", p=3.0),
                   DBSCAN(metric="euclidean", metric_params={}), DBSCAN(metric="precomputed"), MyDBSCAN(), DBSCAN(metric=lambda a, b: 0.0)]
    for algo in unsupported:
        m = _Model(E if algo.metric != "precomputed" else np.zeros((4, 4), np.float32))
        got = find_clusters(names[:len(m._placement.table)], m, algo)
        assert m._engine.calls == [], algo
        assert np.array_equal(got, algo.labels_)
    rec = _Recorder()
    m = _Model(E)
    assert np.array_equal(find_clusters(names, m, rec), np.zeros(len(E)))
    assert m._engine.calls == [] and np.array_equal(rec.seen, E) and isinstance(rec.seen, np.ndarray)
    # parameters sklearn itself rejects: its error, not a device call
    for algo in (DBSCAN(eps=0.0), DBSCAN(eps=-1.0), DBSCAN(min_samples=0), DBSCAN(min_samples=2.5), DBSCAN(eps="x")):
        m = _Model(E)
        with pytest.raises(Exception):
            find_clusters(names, m, algo)
        assert m._engine.calls == []
    # no rows: sklearn's own error
    m = _Model(E)
    with pytest.raises(ValueError):
        find_clusters(np.array([], dtype=str), m)
    assert m._engine.calls == []
    # a cosine call with a zero row: sklearn's convention for it, on the host
    Z = E.copy()
    Z[7] = 0.0
    m = _Model(Z)
    algo = DBSCAN(eps=0.05, metric="cosine", min_samples=2)
    got = find_clusters(names, m, algo)
    assert m._engine.calls == [] and np.array_equal(got, DBSCAN(eps=0.05, metric="cosine", min_samples=2).fit_predict(Z))


def test_device_branch_is_never_computed_on_the_host(monkeypatch):
    """Without a GPU the device branch raises: a real KgeEngine.dbscan has no device to run on, and find_clusters has no fallback
    that would hand the same rows to sklearn instead."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.discovery import find_clusters
    from ampligraph_amd.engine import KgeEngine

    if torch.cuda.is_available():
        return   # (with a GPU the branch runs there: tests/test_gpu_clusters.py)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        KgeEngine("DistMult", 4, 4, 2)
    E = _rows()
    eng = object.__new__(KgeEngine)   # the engine's dbscan over the real library, with host tensors in place of device memory
    eng.lib, eng.device, eng._bufs = _ffi.lib(), torch.device("cpu"), {}
    eng.unpack, eng.rel = (lambda rows: rows), torch.as_tensor(E)
    called = []
    monkeypatch.setattr(DBSCAN, "fit_predict", lambda self, X, y=None, sample_weight=None: called.append(1))
    with pytest.raises(RuntimeError):   # (torch's "No HIP GPUs are available", or the library's AMDKGE_EHIP as an AmdKgeError)
        find_clusters(np.arange(len(E)).astype(str), _Model(E, eng))
    assert called == []
