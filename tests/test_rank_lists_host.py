"""evaluate_candidates without a GPU: the list normalisation (evaluation/candidates.py), what is the extension header's own
(include/amdkge_lists.h; names and types: tests/test_abi_host.py), amdkge_rank_lists' argument validation, and the
sharded placements' refusal."""
import ctypes as C

import numpy as np
import pytest

import abi_decl


def test_as_csr_two_forms_give_the_same_csr():
    from ampligraph_amd.evaluation.candidates import as_csr

    block = np.arange(12, dtype=np.int64).reshape(4, 3)
    off, ids, max_len = as_csr(block, 4)
    assert off.dtype == np.int64 and ids.dtype == np.int32 and ids.flags.c_contiguous
    np.testing.assert_array_equal(off, [0, 3, 6, 9, 12])
    np.testing.assert_array_equal(ids, np.arange(12))
    assert max_len == 3
    for ragged in ([block[i] for i in range(4)], [list(map(int, block[i])) for i in range(4)], tuple(block)):
        off2, ids2, max2 = as_csr(ragged, 4)
        np.testing.assert_array_equal(off2, off)
        np.testing.assert_array_equal(ids2, ids)
        assert max2 == 3 and off2.dtype == np.int64 and ids2.dtype == np.int32
    # a 1-D object array of arrays is the ragged form too
    obj = np.empty(3, dtype=object)
    obj[0], obj[1], obj[2] = np.array([5, 6], np.int32), np.zeros(0, np.int32), np.array([7], np.int64)
    off, ids, max_len = as_csr(obj, 3)
    np.testing.assert_array_equal(off, [0, 2, 2, 3])
    np.testing.assert_array_equal(ids, [5, 6, 7])
    assert max_len == 2 and ids.dtype == np.int32


def test_as_csr_ragged_empty_lists_and_max_len():
    from ampligraph_amd.evaluation.candidates import as_csr

    lists = [np.array([3, 1, 1], np.int32), np.zeros(0, np.int64), np.arange(7), np.array([-1, 9])]
    off, ids, max_len = as_csr(lists, 4)
    np.testing.assert_array_equal(off, [0, 3, 3, 10, 12])
    np.testing.assert_array_equal(ids, [3, 1, 1, 0, 1, 2, 3, 4, 5, 6, -1, 9])   # repeats and the -1 padding stay what they are
    assert max_len == 7
    off, ids, max_len = as_csr([[], []], 2)                                      # only empty lists
    np.testing.assert_array_equal(off, [0, 0, 0])
    assert ids.shape == (0,) and ids.dtype == np.int32 and max_len == 0
    off, ids, max_len = as_csr([], 0)                                            # no triples
    np.testing.assert_array_equal(off, [0])
    assert ids.shape == (0,) and max_len == 0
    off, ids, max_len = as_csr(np.zeros((3, 0), np.int32), 3)                    # a dense block of width 0
    np.testing.assert_array_equal(off, [0, 0, 0, 0])
    assert ids.shape == (0,) and max_len == 0


def test_as_csr_refuses_what_is_not_n_integer_lists():
    from ampligraph_amd.evaluation.candidates import as_csr

    with pytest.raises(ValueError, match="3 candidate lists for 4 triples"):
        as_csr(np.zeros((3, 5), np.int32), 4)
    with pytest.raises(ValueError, match="2 candidate lists for 3 triples"):
        as_csr([[1], [2]], 3)
    with pytest.raises(ValueError, match="integers"):
        as_csr(np.array([["e1", "e2"]]), 1)           # labels: index them first
    with pytest.raises(ValueError, match="integers"):
        as_csr([np.array([0.0, 1.0])], 1)
    with pytest.raises(ValueError, match="integers"):
        as_csr([np.array([True, False])], 1)
    with pytest.raises(ValueError, match="int32"):
        as_csr([np.array([2 ** 31])], 1)
    with pytest.raises(ValueError, match="not 1-D"):
        as_csr([np.zeros((2, 2), np.int32)], 1)
    with pytest.raises(ValueError, match="not 1-D"):
        as_csr(np.arange(3), 3)                        # a flat id array is neither form
    with pytest.raises(ValueError):
        as_csr(np.zeros((2, 2, 2), np.int32), 2)


def test_extension_header_and_its_signature_table():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    assert abi_decl.text("amdkge.h").count('#include "amdkge_lists.h"') == 1
    m = _ffi.Model(2, 10, 50, 5, 0, 12)
    assert lib.amdkge_rank_lists_workspace_bytes(C.byref(m), 100) == lib.amdkge_rank_workspace_bytes(C.byref(m), 100) > 0
    assert lib.amdkge_rank_lists_workspace_bytes(C.byref(m), -1) == -1


def test_rank_lists_argument_validation_without_gpu():
    """Every error below is returned before any device work: the pointers that are set are never dereferenced."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    m = _ffi.Model(2, 10, 50, 5, 0, 12)
    X = C.c_void_p(4096)   # "set": the value is never used

    def call(model=m, ent=X, rel=X, n_ents=50, tri=X, n=3, side=_ffi.SIDE_S, lo=X, hi=X, ids=X, max_len=8, flo=None, fhi=None, fids=None,
             counts=X, sub=None, scores=None, work=X):
        return lib.amdkge_rank_lists(C.byref(model), ent, rel, n_ents, tri, n, side, lo, hi, ids, max_len, flo, fhi, fids, counts, sub, scores,
                                     work, None)

    EINVAL = _ffi.EINVAL
    assert call(tri=None) == EINVAL and b"NULL" in lib.amdkge_last_error()
    for missing in ("ent", "rel", "lo", "hi", "ids", "counts", "work"):
        assert call(**{missing: None}) == EINVAL, missing
    for part in (dict(flo=X), dict(fhi=X, fids=X), dict(flo=X, fhi=X), dict(fids=X)):            # a filter given in part
        assert call(sub=X, **part) == EINVAL and b"together" in lib.amdkge_last_error(), part
    assert call(flo=X, fhi=X, fids=X, sub=None) == EINVAL                                        # a filter needs d_sub
    assert call(side=7) == EINVAL and b"side" in lib.amdkge_last_error()
    assert call(side=0) == EINVAL
    assert call(n=-1) == EINVAL and b"sizes" in lib.amdkge_last_error()
    assert call(max_len=-1) == EINVAL and call(n_ents=0) == EINVAL and call(n_ents=-5) == EINVAL
    assert call(model=_ffi.Model(9, 10, 50, 5, 0, 12)) == EINVAL
    # nothing to do: OK, whatever the pointers
    assert call(n=0) == 0 and call(max_len=0) == 0
    assert call(n=0, ent=None, rel=None, tri=None, lo=None, hi=None, ids=None, counts=None, work=None) == 0
    # RotatE's exact mode on rows that are not stored padded: refused like amdkge_rank_filter, before any launch
    assert call(model=_ffi.Model(4, 25, 50, 5, 5, 0)) == -5 and b"padded" in lib.amdkge_last_error()


def test_sharded_placements_refuse_rank_candidates():
    from ampligraph_amd.placement import Columns, Replicated, Rows

    off, ids = np.array([0, 1], np.int64), np.array([0], np.int32)
    for cls in (Rows, Columns):
        pl = cls.__new__(cls)
        with pytest.raises(NotImplementedError, match="sharded"):
            pl.rank_candidates(np.zeros((1, 3), np.int32), [("s", (off, ids, 1))], None, "worst")
    assert Rows.rank_candidates is not Replicated.rank_candidates and Columns.rank_candidates is not Replicated.rank_candidates


def test_evaluate_candidates_validates_before_any_device_work():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    m = ScoringBasedEmbeddingModel(eta=1, k=2)
    with pytest.raises(ValueError, match="ranking_strategy"):
        m.evaluate_candidates(np.array([["a", "b", "c"]]), candidates_s=[["a"]], ranking_strategy="median")
    with pytest.raises(ValueError, match="not fitted"):
        m.evaluate_candidates(np.array([["a", "b", "c"]]), candidates_s=[["a"]])
