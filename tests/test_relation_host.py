"""Relation prediction without a GPU: PairFilterIndex's host build against a brute-force dict of sets, the validation of
query_topn_relations / evaluate_relations (they raise before they touch a device), the new entry points' argument checks on the
loaded library (they return before any launch) and the new kernels' resources from the built code object."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_decl import declarations

ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ampligraph_amd", "lib", "libamdkge.so")
NEW_SYMBOLS = ("amdkge_relation_workspace_bytes", "amdkge_relation_scores", "amdkge_relation_rank_counts", "amdkge_pair_filter_build",
               "amdkge_pair_filter_ranges")


# ---------------------------------------------------------------------------------------------- PairFilterIndex (host build)
def _brute(datasets):
    known = {}
    for d in datasets:
        for s, p, o in np.asarray(d).reshape(-1, 3).tolist():
            known.setdefault((s, o), set()).add(p)
    return known


def test_pair_filter_index_host_build_against_dict_of_sets():
    from ampligraph_amd.datasets.filters import PairFilterIndex

    rng = np.random.default_rng(5)
    N, R = 23, 7
    a = np.stack([rng.integers(0, N, 300), rng.integers(0, R, 300), rng.integers(0, N, 300)], 1)
    a = np.concatenate([a, a[:40]])                                      # repeated rows inside a dataset
    b = np.concatenate([a[100:180], np.stack([rng.integers(0, N, 90), rng.integers(0, R, 90), rng.integers(0, N, 90)], 1)])   # overlap
    empty = np.zeros((0, 3), dtype=np.int64)
    datasets = [a, empty, b]
    known = _brute(datasets)
    fi = PairFilterIndex(datasets, N, R)
    pairs = sorted(known, key=lambda so: so[0] * N + so[1])
    assert fi.so_keys.dtype == np.int64 and fi.so_start.dtype == np.int64 and fi.r_ids.dtype == np.int32
    assert fi.so_keys.tolist() == [s * N + o for s, o in pairs]
    assert fi.so_start.shape == (len(pairs) + 1,) and fi.so_start[0] == 0 and fi.so_start[-1] == fi.r_ids.size == sum(len(v) for v in known.values())
    for g, so in enumerate(pairs):
        ids = fi.r_ids[fi.so_start[g]:fi.so_start[g + 1]].tolist()
        assert ids == sorted(known[so]), so                              # the SET, ascending
    # ranges: every present pair, every absent pair of the grid, whatever the predicate column says
    q = np.array([[s, 0, o] for s in range(N) for o in range(N)])
    q[:, 1] = rng.integers(0, R, q.shape[0])
    assert any((s, o) not in known for s, _, o in q.tolist())
    lo, hi = fi.relation_ranges(q)
    assert lo.dtype == np.int64 and hi.dtype == np.int64
    for (s, _, o), a_, b_ in zip(q.tolist(), lo.tolist(), hi.tolist()):
        assert fi.r_ids[a_:b_].tolist() == sorted(known.get((s, o), ())), (s, o)
        if (s, o) not in known:
            assert (a_, b_) == (0, 0)
    lo, hi = fi.relation_ranges(np.zeros((0, 3), dtype=np.int64))
    assert lo.shape == (0,) and hi.shape == (0,)


def test_pair_filter_index_empty_and_overflow():
    from ampligraph_amd.datasets.filters import PairFilterIndex

    for datasets in ([], [np.zeros((0, 3), dtype=np.int64)]):
        fi = PairFilterIndex(datasets, 5, 3)
        assert fi.so_keys.size == 0 and fi.so_start.tolist() == [0] and fi.r_ids.size == 0
        lo, hi = fi.relation_ranges(np.array([[1, 2, 3], [0, 0, 0]]))
        assert lo.tolist() == [0, 0] and hi.tolist() == [0, 0]
    with pytest.raises(ValueError, match="packed int64"):
        PairFilterIndex([], 2 ** 31 - 1, 2 ** 10)


# ---------------------------------------------------------------------------------------------- validation of the public functions
class _StubModel:
    """What query_topn_relations reads before it reaches the device: the fitted flag and the label maps."""

    def __init__(self, fitted=True):
        from ampligraph_amd.datasets.indexer import DataIndexer

        self.is_fitted = fitted
        self.data_indexer = DataIndexer(np.array([["a", "likes", "b"], ["b", "likes", "c"], ["c", "knows", "a"]]))
        self._n_ents, self._n_rels = 3, 2

    def __getattr__(self, name):   # _engine, _placement, _pair_filter_index: validation must fail before it needs any of them
        if not name.startswith("_"):
            raise AttributeError(name)
        raise AssertionError("query_topn_relations touched model.{} before validating its arguments".format(name))


def test_query_topn_relations_validation():
    from ampligraph_amd import discovery
    from ampligraph_amd.discovery import query_topn_relations

    assert "query_topn_relations" in discovery.__all__ and "query_topn_relations" in discovery.__doc__
    m = _StubModel()
    ok = np.array([["a", "b"], ["c", "a"]])
    for bad in (np.array(["a", "b"]), np.array([["a", "likes", "b"]]), np.zeros((2, 2, 2)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="pairs"):
            query_topn_relations(m, bad)
    with pytest.raises(ValueError, match="top_n"):
        query_topn_relations(m, ok, top_n=0)
    with pytest.raises(ValueError, match="1024"):
        query_topn_relations(m, ok, top_n=1025)
    with pytest.raises(ValueError, match="use_filter"):
        query_topn_relations(m, ok, use_filter=True)
    with pytest.raises(ValueError, match="use_filter"):
        query_topn_relations(m, ok, use_filter=np.array([["a", "likes"]]))
    with pytest.raises(ValueError, match="rels_to_consider"):
        query_topn_relations(m, ok, rels_to_consider="likes")
    with pytest.raises(ValueError, match="rels_to_consider"):
        query_topn_relations(m, ok, rels_to_consider=["likes", "hates"])
    with pytest.raises(ValueError, match=r"Entities not seen by the model: \['zed', 'yan'\]"):
        query_topn_relations(m, np.array([["zed", "a"], ["a", "b"], ["yan", "b"], ["zed", "c"]]))
    with pytest.raises(ValueError, match=r"Entities not seen by the model: \['likes'\]"):
        query_topn_relations(m, np.array([["a", "likes"]]))                # the object column
    with pytest.raises(ValueError, match="not fitted"):
        query_topn_relations(_StubModel(fitted=False), ok)

    class Wrapper:   # a 1.x compat wrapper is unwrapped: the inner model's state decides
        is_backward = True
        is_fitted = True

        def __init__(self, inner):
            self.model = inner

    with pytest.raises(ValueError, match="not fitted"):
        query_topn_relations(Wrapper(_StubModel(fitted=False)), ok)
    with pytest.raises(ValueError, match=r"\['zed'\]"):
        query_topn_relations(Wrapper(_StubModel()), np.array([["zed", "a"]]))


def test_evaluate_relations_validation():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    m = ScoringBasedEmbeddingModel(eta=1, k=4, scoring_type="ComplEx")
    x = np.array([["a", "likes", "b"]])
    with pytest.raises(ValueError, match="not fitted"):
        m.evaluate_relations(x)
    with pytest.raises(ValueError, match="ranking_strategy"):
        m.evaluate_relations(x, ranking_strategy="median")
    # a fitted model's argument checks run before anything touches the placement or the engine
    stub = _StubModel()
    call = ScoringBasedEmbeddingModel.evaluate_relations
    with pytest.raises(ValueError, match="ranking_strategy"):
        call(stub, x, ranking_strategy=None)
    with pytest.raises(ValueError, match="use_filter"):
        call(stub, x, use_filter=np.array([["a", "likes", "b"]]))
    # evaluate() keeps its signature
    import inspect

    assert list(inspect.signature(ScoringBasedEmbeddingModel.evaluate).parameters)[1:] == [
        "x", "batch_size", "verbose", "use_filter", "corrupt_side", "entities_subset", "ranking_strategy", "callbacks", "dataset_type"]
    assert list(inspect.signature(call).parameters)[1:] == ["x", "use_filter", "relations_subset", "ranking_strategy", "verbose"]


# ---------------------------------------------------------------------------------------------- ABI argument checks
def _buf(n=64, t=ctypes.c_int64):
    return ctypes.cast((t * n)(), ctypes.c_void_p)


def test_new_symbols_declared_bound_and_exported():
    from ampligraph_amd import _ffi

    declared = set(declarations("amdkge.h"))   # the parsed declarations: a mention in a comment does not count
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _ffi.ABI["amdkge.h"] and hasattr(lib, name), name
    assert lib.amdkge_abi_version() == 5 == _ffi.ABI_VERSION


def test_relation_entry_points_argument_validation_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    m = _ffi.Model(2, 10, 50, 7, 0, 12)
    rot = _ffi.Model(4, 10, 50, 7, 7, 12)
    bad = _ffi.Model(9, 10, 50, 7, 0, 0)
    by = ctypes.byref
    b = _buf
    # workspace: only RotatE needs one
    assert lib.amdkge_relation_workspace_bytes(by(m), 7) == 0
    assert lib.amdkge_relation_workspace_bytes(by(rot), 7) >= 7 * 24 * 4
    assert lib.amdkge_relation_workspace_bytes(by(rot), -1) == -1 and lib.amdkge_relation_workspace_bytes(by(bad), 7) == -1
    assert lib.amdkge_relation_workspace_bytes(None, 7) == -1
    # scores
    sc = lib.amdkge_relation_scores
    assert sc(by(bad), b(), b(), b(), 1, None, 0, 7, b(), 7, None, None) == -1 and b"scoring_type" in lib.amdkge_last_error()
    assert sc(by(m), None, None, None, 0, None, 0, 7, None, 7, None, None) == 0            # n == 0 is a no-op
    assert sc(by(m), b(), b(), b(), 3, None, 2, 2, None, 0, None, None) == 0               # no candidates: nothing to write
    assert sc(by(m), b(), b(), b(), -1, None, 0, 7, b(), 7, None, None) == -1 and b"relation_scores" in lib.amdkge_last_error()
    assert sc(by(m), b(), b(), b(), 3, None, -1, 7, b(), 8, None, None) == -1              # rel_lo < 0
    assert sc(by(m), b(), b(), b(), 3, None, 5, 4, b(), 7, None, None) == -1               # rel_hi < rel_lo
    assert sc(by(m), b(), b(), b(), 3, None, 0, 7, b(), 6, None, None) == -1               # ld < m
    assert sc(by(m), b(), b(), b(), 3, None, 0, 8, b(), 8, None, None) == -1               # beyond the relation table
    assert sc(by(m), None, b(), b(), 3, None, 0, 7, b(), 7, None, None) == -1              # NULL pointers
    assert sc(by(m), b(), b(), b(), 3, None, 0, 7, None, 7, None, None) == -1
    assert sc(by(rot), b(), b(), b(), 3, None, 0, 7, b(), 7, None, None) == -1 and b"workspace" in lib.amdkge_last_error()
    # rank counts
    rc = lib.amdkge_relation_rank_counts
    assert rc(None, 0, 7, 7, None, None, 0, None, None, None, None, None, None, None) == 0   # n == 0
    assert rc(b(), -1, 7, 7, b(), None, 0, None, None, None, None, b(), None, None) == -1 and b"relation_rank_counts" in lib.amdkge_last_error()
    assert rc(b(), 2, -1, 0, b(), None, 0, None, None, None, None, b(), None, None) == -1
    assert rc(b(), 2, 7, 6, b(), None, 0, None, None, None, None, b(), None, None) == -1     # ld < m
    for lo, hi, ids in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):   # a range array without its siblings
        args = [b() if f else None for f in (lo, hi, ids)]
        assert rc(b(), 2, 7, 7, b(), None, 0, *args, None, b(), b(), None) == -1, (lo, hi, ids)
        assert b"three NULLs" in lib.amdkge_last_error()
    assert rc(b(), 2, 7, 7, None, None, 0, None, None, None, None, b(), None, None) == -1    # NULL positives
    assert rc(b(), 2, 7, 7, b(), None, 0, None, None, None, None, None, None, None) == -1    # NULL counts
    assert rc(None, 2, 7, 7, b(), None, 0, None, None, None, None, b(), None, None) == -1    # NULL block with m > 0
    assert rc(b(), 2, 7, 7, b(), None, 0, b(), b(), b(), None, b(), None, None) == -1        # a filter without d_sub
    # pair filter
    pb, pr = lib.amdkge_pair_filter_build, lib.amdkge_pair_filter_ranges
    assert pb(b(), -1, 10, 2, b(), b(), b(), b(), b(), None) == -1 and b"pair_filter_build" in lib.amdkge_last_error()
    assert pb(b(), 3, 0, 2, b(), b(), b(), b(), b(), None) == -1 and pb(b(), 3, 10, 0, b(), b(), b(), b(), b(), None) == -1
    assert pb(b(), 3, 2 ** 31 - 1, 2 ** 10, b(), b(), b(), b(), b(), None) == -5             # keys do not fit 64 bits
    assert pb(b(), 3, 10, 2, b(), None, b(), b(), b(), None) == -1                           # NULL start / counts
    assert pb(None, 3, 10, 2, b(), b(), b(), b(), b(), None) == -1                           # NULL triples
    assert pr(None, None, 0, None, 0, 10, None, None, None) == 0                             # empty batch
    assert pr(None, None, 0, None, -1, 10, None, None, None) == -1 and b"pair_filter_ranges" in lib.amdkge_last_error()
    assert pr(None, None, -1, b(), 2, 10, b(), b(), None) == -1 and pr(None, None, 0, b(), 2, 0, b(), b(), None) == -1
    assert pr(None, None, 0, None, 2, 10, b(), b(), None) == -1                              # NULL triples
    assert pr(None, None, 3, b(), 2, 10, b(), b(), None) == -1                               # keys announced, none given
    # the existing two still refuse any side other than S / O
    assert lib.amdkge_filter_ranges(None, None, 0, None, 5, 3, 10, 2, None, None, None) == -1
    assert lib.amdkge_filter_build(None, 0, 4, 10, 2, None, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- resources of the new kernels
def test_relation_kernels_use_no_scratch():
    from ampligraph_amd.utils.codeobj import kernel_resources

    assert os.path.exists(LIB), "library not built: run build() first"
    res = kernel_resources(LIB)
    new = {n: k for n, k in res.items() if re.match(r"_ZN3kge\d+(relation_|pair_filter_)", n) or n.startswith("_ZN3kge20filter_ranges_kernel")}
    main = [n for n in new if "relation_scores_kernel" in n]
    reload_ = [n for n in new if "relation_scores_reload_kernel" in n]
    # four model families x (four lane-iteration counts of the register form + three vector widths of the reload form)
    assert len(main) == 16 and len(reload_) == 12, sorted(new)
    assert any("relation_prep_kernel" in n for n in new) and any("relation_counts_kernel" in n for n in new)
    assert any("filter_ranges_kernel" in n for n in new)
    for n, k in new.items():
        assert k["scratch"] == 0, (n, k)
        assert k["vgpr"] <= 256 and k["waves_per_simd"] >= 2, (n, k)
    # the headline shapes (ComplEx / TransE, k = 200: one lane iteration, four queries per wave) at three waves per SIMD or more
    for name in ("_ZN3kge22relation_scores_kernelILi2ELi1ELi4EEEvNS_7RelArgsE", "_ZN3kge22relation_scores_kernelILi0ELi1ELi4EEEvNS_7RelArgsE"):
        assert name in new and new[name]["waves_per_simd"] >= 3, new.get(name)
