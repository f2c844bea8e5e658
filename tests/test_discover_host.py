"""discover_facts / generate_candidates on the host (no GPU): generate_candidates and _setdiff2d against recorded outputs of the
reference's functions (tests/golden/discovery_candidates_v1.json: graphs by recipe, arguments, returned rows), the scalable set
difference against the quadratic form it replaces, and discover_facts' own logic against a stub model with a canned evaluate()."""
import json
import os

import numpy as np
import pytest

from ampligraph_amd.datasets.indexer import DataIndexer
from ampligraph_amd.discovery import _setdiff2d, discover_facts, generate_candidates

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "discovery_candidates_v1.json")

DOC8 = np.array([["a", "y", "b"], ["b", "y", "a"], ["a", "y", "c"], ["c", "y", "a"], ["a", "y", "d"], ["c", "y", "d"], ["b", "y", "c"],
                 ["f", "y", "e"]])


def graph(name):
    if name == "docstring8":
        return DOC8
    n_rel = {"mod50": 5, "mod50_two_relations": 2}[name]
    return np.stack([["entity_{}".format(x % 15) for x in range(50)], ["rel_{}".format(x % n_rel) for x in range(50)],
                     ["entity_{}".format(x % 20) for x in range(50)]], axis=1)


with open(GOLDEN) as fh:
    CASES = json.load(fh)["cases"]


@pytest.mark.parametrize("case", CASES, ids=["{}-{}-{}".format(i, c["graph"], c["args"]["strategy"]) for i, c in enumerate(CASES)])
def test_generate_candidates_equals_the_recorded_reference_rows(case):
    got = generate_candidates(graph(case["graph"]), **case["args"])
    want = np.array(case["rows"], dtype=object).reshape(-1, 3)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


def test_generate_candidates_reference_assertions():
    """tests/ampligraph/discovery/test_discovery.py test_generate_candidates of the reference, restated."""
    X = graph("mod50")
    assert generate_candidates(X, strategy="random_uniform", target_rel="rel_0", max_candidates=15, consolidate_sides=False, seed=1916).shape == (15, 3)
    C = generate_candidates(X, strategy="random_uniform", target_rel="rel_1", max_candidates=20, consolidate_sides=True, seed=1916)
    assert C.shape == (20, 3) and C[0, 0] == "entity_16" and np.all(C[:, 1] == "rel_1")
    C = generate_candidates(X, strategy="random_uniform", target_rel="rel_0", max_candidates=20, consolidate_sides=False, seed=0)
    assert np.all(np.isin(C[:, 0], np.unique(X[:, 0]))) and np.all(np.isin(C[:, 2], np.unique(X[:, 2])))
    C = generate_candidates(X, strategy="random_uniform", target_rel="rel_0", max_candidates=100, consolidate_sides=True, seed=1)
    assert np.any(np.isin(C[:, 2], np.unique(X[:, 0]))) or np.all(np.isin(C[:, 0], np.unique(X[:, 2])))
    for strategy, n, seed in (("entity_frequency", 20, 1), ("graph_degree", 30, 1), ("cluster_coefficient", 30, 2), ("cluster_triangles", 50, 1),
                              ("cluster_squares", 60, 1)):
        assert generate_candidates(X, strategy=strategy, target_rel="rel_0", max_candidates=n, consolidate_sides=False, seed=seed).shape == (n, 3)
    # the docstring graph: the recorded answer, not the docstring's text (and the row is in X: the first-copy-only quirk)
    C = generate_candidates(DOC8, strategy="graph_degree", target_rel="y", max_candidates=3)
    assert C.tolist() == [["b", "y", "c"]] * 3


def test_generate_candidates_argument_checks():
    X = graph("mod50")
    with pytest.raises(ValueError, match="not a valid candidate generation strategy"):
        generate_candidates(X, "exhaustive", "rel_0", 10)
    with pytest.raises(ValueError, match="must be a float or int"):
        generate_candidates(X, "random_uniform", "rel_0", "10")
    with pytest.raises(ValueError, match="positive integer"):
        generate_candidates(X, "random_uniform", "rel_0", 0)
    assert generate_candidates(np.concatenate([X, X[:, :1]], 1), "random_uniform", "rel_0", 0.2, seed=3).shape == (10, 3)   # weights column, float


def test_setdiff2d_reference_answers_and_quirk():
    Y = DOC8.copy()
    Y[:4, 1] = "z"
    assert np.array_equal(_setdiff2d(DOC8, Y), DOC8[:4])
    assert np.array_equal(_setdiff2d(Y, DOC8), Y[:4])
    with pytest.raises(RuntimeError):
        _setdiff2d(np.array([1, 2, 3, 4, 5, 6]), np.array([1, 2, 3, 7, 8, 9]))
    A = np.array([["a", "y", "b"], ["a", "y", "b"], ["q", "y", "b"]])
    assert _setdiff2d(A, DOC8).tolist() == [["a", "y", "b"], ["q", "y", "b"]]   # only the first copy of a row of X goes


def _setdiff2d_quadratic(A, B):
    """What the reference computes, one pair of rows at a time: row i of A goes iff it equals some row of B and no earlier row of A
    equals that row."""
    keep = []
    for i in range(len(A)):
        in_b = any((A[i] == B[j]).all() for j in range(len(B)))
        earlier = any((A[i] == A[h]).all() for h in range(i))
        keep.append(not (in_b and not earlier))
    return A[np.array(keep, dtype=bool)]


@pytest.mark.parametrize("seed", range(6))
def test_setdiff2d_equals_the_quadratic_form(seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, size=(int(rng.integers(1, 60)), 3))
    B = rng.integers(0, 4, size=(int(rng.integers(1, 60)), 3))
    if seed % 2:
        A, B = np.char.add("e", A.astype(str)), np.char.add("e", B.astype(str)).astype(object)
    got = _setdiff2d(A, B)
    assert np.array_equal(got, _setdiff2d_quadratic(A, B))
    assert len(got) < len(A)   # (4^3 distinct rows at most: some row of A is in B)


# ------------------------------------------------------------------------------------------------ discover_facts on a stub
class StubModel:
    """is_fitted, data_indexer and a canned evaluate(): rank (i + 1, i + 2) for the i-th candidate it is shown."""

    def __init__(self, X, fitted=True, ranks=None):
        self.is_fitted = fitted
        self.data_indexer = DataIndexer(X)
        self.calls = []
        self._ranks = ranks

    def evaluate(self, x, use_filter=False, corrupt_side="s,o", verbose=True):
        assert corrupt_side == "s,o" and verbose is False and set(use_filter) == {"test"}
        x = np.asarray(x)
        assert self.data_indexer.valid_row_mask(x).all()   # nothing evaluate() would drop reaches it
        self.calls.append((x.copy(), np.asarray(use_filter["test"])))
        n = len(x)
        if self._ranks is not None:
            return np.asarray(self._ranks(x))
        return np.stack([np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.int32)


def test_discover_facts_reference_errors():
    with pytest.raises(ValueError, match="Model is not fitted."):
        discover_facts(DOC8, StubModel(DOC8, fitted=False))
    with pytest.raises(ValueError, match="error is not a valid strategy."):
        discover_facts(DOC8, StubModel(DOC8), strategy="error")
    with pytest.raises(ValueError, match="Target relation\\(s\\) not found in model: \\['error'\\]"):
        discover_facts(DOC8, StubModel(DOC8), strategy="random_uniform", target_rel="error")

    class Wrapper:   # 1.x compat wrappers hold the model
        is_backward = True

    w = Wrapper()
    w.model = StubModel(DOC8, fitted=False)
    with pytest.raises(ValueError, match="Model is not fitted."):
        discover_facts(DOC8, w)


def test_discover_facts_float_max_candidates_and_inclusive_cut():
    X = graph("mod50")
    m = StubModel(X)
    got, ranks = discover_facts(X, m, top_n=3.5, strategy="random_uniform", max_candidates=0.3, target_rel="rel_0", seed=5)
    want = generate_candidates(X, "random_uniform", ["rel_0"], int(0.3 * len(X)), seed=5)   # the reference hands the wrapped list on
    assert len(want) == 15 and len(m.calls) == 1 and np.array_equal(m.calls[0][0], want) and np.array_equal(m.calls[0][1], X)
    # canned mean ranks 1.5, 2.5, 3.5, 4.5, ...: the cut at 3.5 is inclusive
    assert np.array_equal(ranks, [1.5, 2.5, 3.5]) and np.array_equal(got, want[:3])
    assert got.shape == (3, 3) and ranks.shape == (3,)


def test_discover_facts_stacks_relations_vertically():
    X = graph("mod50_two_relations")
    m = StubModel(X)
    got, ranks = discover_facts(X, m, top_n=2.5, strategy="entity_frequency", max_candidates=20, target_rel=None, seed=2)
    assert len(m.calls) == 2                                    # target_rel=None: one round per relation of the model, in id order
    assert (m.calls[0][0][:, 1] == "rel_0").all() and (m.calls[1][0][:, 1] == "rel_1").all()
    assert got.shape == (4, 3) and ranks.shape == (4,)          # two per relation, stacked vertically (np.hstack would give (2, 6))
    assert got[:, 1].tolist() == ["rel_0", "rel_0", "rel_1", "rel_1"] and np.array_equal(ranks, [1.5, 2.5, 1.5, 2.5])
    for call, part in zip(m.calls, (got[:2], got[2:])):
        assert np.array_equal(part, call[0][:2])
    # a given LIST goes to generate_candidates in one call, as the reference's rel_list = [target_rel] does
    m2 = StubModel(X)
    got2, _ = discover_facts(X, m2, top_n=100, strategy="random_uniform", max_candidates=20, target_rel=["rel_0", "rel_1"], seed=7)
    assert len(m2.calls) == 1 and np.array_equal(got2, generate_candidates(X, "random_uniform", ["rel_0", "rel_1"], 20, seed=7))
    assert set(got2[:, 1]) == {"rel_0", "rel_1"}


def test_discover_facts_drops_unseen_candidates_before_ranking():
    X = graph("mod50")
    seen = X[(X[:, 0] != "entity_3") & (X[:, 2] != "entity_3")]     # the model never saw entity_3; X still holds it
    score = lambda rows: np.stack([[int(s.split("_")[1]) + 1 for s in rows[:, 0]], [int(o.split("_")[1]) + 1 for o in rows[:, 2]]], 1)   # noqa: E731
    m = StubModel(seen, ranks=score)
    cands = generate_candidates(X, "random_uniform", ["rel_0"], 20, seed=11)
    unseen = (cands[:, 0] == "entity_3") | (cands[:, 2] == "entity_3")
    assert unseen.any() and not unseen.all()
    kept = cands[~unseen]
    mean = score(kept).mean(1)
    cut = float(np.median(mean))
    got, ranks = discover_facts(X, m, top_n=cut, strategy="random_uniform", max_candidates=20, target_rel="rel_0", seed=11)
    assert np.array_equal(m.calls[0][0], kept)
    assert np.array_equal(got, kept[mean <= cut]) and np.array_equal(ranks, mean[mean <= cut]) and 0 < len(got) < len(kept)
    assert np.array_equal(score(got).mean(1), ranks)               # rows and ranks are aligned


def test_discover_facts_empty_result_shapes():
    X = graph("mod50")
    got, ranks = discover_facts(X, StubModel(X), top_n=1, strategy="random_uniform", max_candidates=10, target_rel="rel_0")
    assert got.shape == (0, 3) and ranks.shape == (0,)


def test_exhaustive_refuses_sharded_placements():
    from ampligraph_amd.placement import Columns, Rows

    for cls in (Rows, Columns):
        m = StubModel(DOC8)
        m._placement = cls.__new__(cls)
        with pytest.raises(NotImplementedError, match="exhaustive"):
            discover_facts(DOC8, m, strategy="exhaustive", target_rel="y")
    with pytest.raises(ValueError, match="not found in model"):   # the reference's checks come first
        discover_facts(DOC8, StubModel(DOC8), strategy="exhaustive", target_rel="nope")
