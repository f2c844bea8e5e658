"""Host side of find_duplicates (ampligraph_amd/discovery.py) without a GPU: the tolerance bisection over one nearest distance per
row and the result sets from a sorted pair list, against the reference's procedure restated on numpy embeddings (sklearn
NearestNeighbors(radius=...).radius_neighbors per tolerance, scipy.optimize.bisect on [0, largest pair distance]); and the argument
validation of the two join entry points of the C ABI."""
import numpy as np
import pytest
from scipy import optimize
from sklearn.neighbors import NearestNeighbors

from ampligraph_amd.discovery import duplicate_sets, duplicate_tolerance


def ref_dups(emb, labels, tol):
    """The reference's get_dups: every row whose radius neighbourhood (itself included) has more than one row."""
    nb = NearestNeighbors(metric="euclidean", radius=tol).fit(emb).radius_neighbors(emb)[1]
    return {frozenset(labels[j] for j in row) for row in nb if len(row) > 1}


def ref_auto(emb, labels, expected):
    max_d = np.sqrt(((emb[:, None, :] - emb[None, :, :]) ** 2).sum(-1)).max()
    tol = optimize.bisect(lambda t: len(set().union(*ref_dups(emb, labels, t))) / len(emb) - expected, 0.0, max_d, xtol=1e-3, maxiter=50)
    return tol, max_d


def join(emb):
    """fp64 brute force of what the device join returns: nearest other row (squared) and sorted pairs i < j within a radius."""
    D2 = ((emb[:, None, :] - emb[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D2, np.inf)
    return D2


def ours(emb, labels, tol=None, expected=0.1):
    D2 = join(emb)
    n = len(emb)
    if tol is None:
        tol = duplicate_tolerance(D2.min(1), labels, lambda t: t * t, expected, float(np.sqrt(D2[np.isfinite(D2)].max())))
    i, j = np.nonzero(np.triu(D2 <= tol * tol, 1))
    return duplicate_sets(np.stack([i, j], 1), labels, n), tol


def planted(rng, n, d, groups, eps=1e-3):
    emb = rng.normal(size=(n, d))
    for g in range(groups):
        src = rng.integers(0, n)
        for k in rng.choice(n, size=rng.integers(1, 4), replace=False):
            if k != src:
                emb[k] = emb[src] + eps * rng.normal(size=d)
    return emb


@pytest.mark.parametrize("seed", range(4))
def test_random_tables_numeric_and_auto(seed):
    rng = np.random.default_rng(seed)
    emb = rng.normal(size=(60, 5))
    labels = ["e%d" % i for i in range(60)]
    for tol in (0.3, 0.8, 1.5):
        assert ours(emb, labels, tol)[0] == ref_dups(emb, labels, tol)
    for expected in (0.1, 0.3, 0.7):
        want, _ = ref_auto(emb, labels, expected)
        got_sets, got = ours(emb, labels, None, expected)
        assert got == pytest.approx(want, rel=1e-12)
        assert got_sets == ref_dups(emb, labels, got)


def test_planted_groups():
    rng = np.random.default_rng(7)
    emb = planted(rng, 200, 16, 12)
    labels = ["n%d" % i for i in range(200)]
    want, _ = ref_auto(emb, labels, 0.05)
    sets, tol = ours(emb, labels, None, 0.05)
    assert tol == pytest.approx(want, rel=1e-12) and sets == ref_dups(emb, labels, tol)
    sets, _ = ours(emb, labels, 0.05)
    assert sets == ref_dups(emb, labels, 0.05) and all(len(s) >= 2 for s in sets) and len(sets) > 0


def test_repeated_labels_give_one_element_sets():
    """A label repeated in X (identical embeddings) pairs with itself: the reference's code returns a one-element set."""
    rng = np.random.default_rng(3)
    base = rng.normal(size=(20, 4))
    idx = np.concatenate([np.arange(20), [2, 2, 5]])
    emb = base[idx]
    labels = ["r%d" % i for i in idx]
    sets, _ = ours(emb, labels, 1e-6)
    assert sets == ref_dups(emb, labels, 1e-6) == {frozenset(["r2"]), frozenset(["r5"])}
    for expected in (0.1, 0.4):
        want, _ = ref_auto(emb, labels, expected)
        s, tol = ours(emb, labels, None, expected)
        assert tol == pytest.approx(want, rel=1e-12) and s == ref_dups(emb, labels, tol)


def test_triple_labels():
    rng = np.random.default_rng(11)
    X = np.stack([rng.integers(0, 9, 40), rng.integers(0, 3, 40), rng.integers(0, 9, 40)], 1)
    X = np.char.add(np.array(["e", "r", "e"]), X.astype(str))
    E, R = rng.normal(size=(9, 3)), rng.normal(size=(3, 3))
    ids = np.char.lstrip(X, "er").astype(int)
    emb = np.hstack([E[ids[:, 0]], R[ids[:, 1]], E[ids[:, 2]]])
    labels = [tuple(r) for r in X.tolist()]
    for tol in (0.5, 1.2):
        assert ours(emb, labels, tol)[0] == ref_dups(emb, labels, tol)
    want, _ = ref_auto(emb, labels, 0.3)
    s, tol = ours(emb, labels, None, 0.3)
    assert tol == pytest.approx(want, rel=1e-12) and s == ref_dups(emb, labels, tol)


def test_bisection_errors_like_the_reference():
    """Same scipy routine: f(0) and f(max) of one sign raise the same ValueError."""
    emb = np.random.default_rng(0).normal(size=(10, 3))
    labels = list(range(10))
    with pytest.raises(ValueError):
        ours(emb, labels, None, 1.5)


def test_sets_from_unsorted_and_empty_pairs():
    assert duplicate_sets(np.zeros((0, 2), np.int64), ["a"], 1) == set()
    s = duplicate_sets(np.array([[0, 3], [1, 2], [0, 1]]), ["a", "b", "c", "d"], 4)
    assert s == {frozenset("abd"), frozenset("abc"), frozenset("bc"), frozenset("ad")}


def test_join_abi_argument_validation_without_gpu():
    import ctypes as C

    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    buf = C.c_void_p(16)   # never dereferenced: every call below returns before touching the device
    assert lib.amdkge_join_nearest(None, -1, 4, None, None, None, None, None) == -1
    assert b"bad sizes" in lib.amdkge_last_error()
    assert lib.amdkge_join_nearest(buf, 5, 0, buf, buf, buf, buf, None) == -1                   # d < 1
    assert lib.amdkge_join_nearest(buf, 1 << 31, 4, buf, buf, buf, buf, None) == -1             # n > 2^31 - 1
    assert lib.amdkge_join_nearest(buf, 5, 4, buf, None, buf, buf, None) == -1                  # NULL index output
    assert b"NULL" in lib.amdkge_last_error()
    assert lib.amdkge_join_nearest(buf, 5, 4, buf, buf, buf, None, None) == -1                  # NULL workspace
    assert lib.amdkge_join_radius(None, 3, 4, 1.0, None, 0, None, None) == -1                   # NULL count
    assert b"NULL" in lib.amdkge_last_error()
    assert lib.amdkge_join_radius(buf, 3, 4, 1.0, None, 8, buf, None) == -1                     # cap > 0, no buffer
    assert lib.amdkge_join_radius(buf, 3, 4, 1.0, buf, -1, buf, None) == -1                     # cap < 0
    assert lib.amdkge_join_radius(buf, 3, 4, float("nan"), buf, 8, buf, None) == -1             # NaN threshold
    assert b"NaN" in lib.amdkge_last_error()
    assert lib.amdkge_join_radius(buf, 3, -2, 1.0, buf, 8, buf, None) == -1
