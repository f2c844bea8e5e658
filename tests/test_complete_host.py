"""query_topn_batch without a GPU: amdkge_topk_rows_excluding's argument checks on the loaded library (they return before any
launch) and the public function's validation against a stub model (it raises before it touches a device)."""
import ctypes

import numpy as np
import pytest


def _call(lib, n=1, m=8, ld=8, k=4, vals=1, col_ids=None, lo=None, hi=None, ids=None, own=None, out_idx=1, out_val=1):
    """amdkge_topk_rows_excluding with small host buffers standing in for device memory: no checked path reads them."""
    keep = [(ctypes.c_float * 64)(), (ctypes.c_int32 * 64)(), (ctypes.c_float * 64)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)(),
            (ctypes.c_int32 * 8)()]
    p = lambda buf: ctypes.cast(buf, ctypes.c_void_p)   # noqa: E731
    return lib.amdkge_topk_rows_excluding(p(keep[0]) if vals else None, n, m, ld, col_ids, 0,
                                          p(keep[3]) if lo else None, p(keep[4]) if hi else None, p(keep[5]) if ids else None, own, k,
                                          p(keep[1]) if out_idx else None, p(keep[2]) if out_val else None, None)


def test_topk_rows_excluding_argument_validation_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    assert "amdkge_topk_rows_excluding" in _ffi.ABI["amdkge.h"] and lib.amdkge_abi_version() == 5
    assert _call(lib, n=0) == 0                                           # an empty batch is a no-op
    assert _call(lib, n=0, vals=0, out_idx=0, out_val=0) == 0
    assert _call(lib, k=0) == -1 and b"topk_rows_excluding" in lib.amdkge_last_error()
    assert _call(lib, k=1025) == -1
    assert _call(lib, k=1024, n=0) == 0                                   # the limit itself is a valid size
    assert _call(lib, m=8, ld=7) == -1                                    # ld < m
    assert _call(lib, n=-1) == -1 and _call(lib, m=-1, ld=0) == -1
    for lo, hi, ids in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):   # a range array without its siblings
        assert _call(lib, lo=lo, hi=hi, ids=ids) == -1, (lo, hi, ids)
        assert b"three NULLs" in lib.amdkge_last_error()
    assert _call(lib, out_idx=0) == -1 and _call(lib, out_val=0) == -1    # NULL outputs
    assert _call(lib, vals=0) == -1                                       # NULL score block with m > 0


def test_topk_rows_refuse_columns_beyond_int32():
    """amdkge_topk_rows and amdkge_topk_rows_excluding return int32 column indices (-1 = missing): m, like n, is at most 2^31 - 1 and a
    wider block is refused with AMDKGE_EUNSUPPORTED before any launch (a block that wide is selected in column chunks, the chunks' winners
    merged through d_payload).  The limit itself passes the size checks: the call then fails on the NULL pointer behind them."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    top = 2 ** 31 - 1
    buf = [(ctypes.c_int32 * 8)(), (ctypes.c_float * 8)()]
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)   # noqa: E731
    for m in (top + 1, 2 ** 32 - 2, 2 ** 32):
        assert _call(lib, m=m, ld=m) == -5 and b"int32" in lib.amdkge_last_error(), m
        assert lib.amdkge_topk_rows(p(buf[1]), 1, m, m, None, None, None, 4, 1, p(buf[0]), p(buf[1]), None) == -5 and b"int32" in lib.amdkge_last_error(), m
    assert _call(lib, n=top + 1) == -5 and lib.amdkge_topk_rows(p(buf[1]), top + 1, 8, 8, None, None, None, 4, 1, p(buf[0]), p(buf[1]), None) == -5
    assert _call(lib, m=top, ld=top, vals=0) == -1 and b"NULL" in lib.amdkge_last_error()
    assert lib.amdkge_topk_rows(None, 1, top, top, None, None, None, 4, 1, p(buf[0]), p(buf[1]), None) == -1 and b"NULL" in lib.amdkge_last_error()


class _StubModel:
    """What query_topn_batch reads before it reaches the device: the fitted flag and the label maps."""

    def __init__(self, fitted=True):
        from ampligraph_amd.datasets.indexer import DataIndexer

        self.is_fitted = fitted
        self.data_indexer = DataIndexer(np.array([["a", "likes", "b"], ["b", "likes", "c"], ["c", "knows", "a"]]))
        self._n_ents, self._n_rels = 3, 2

    def __getattr__(self, name):   # _engine, _placement, _filter_index: validation must fail before it needs any of them
        if not name.startswith("_"):
            raise AttributeError(name)
        raise AssertionError("query_topn_batch touched model.{} before validating its arguments".format(name))


def test_query_topn_batch_validation():
    from ampligraph_amd import discovery
    from ampligraph_amd.discovery import query_topn_batch

    assert "query_topn_batch" in discovery.__all__
    m = _StubModel()
    ok = np.array([["a", "likes"], ["b", "knows"]])
    for side in ("s,o", "x", None, "r"):
        with pytest.raises(ValueError, match="corrupt_side"):
            query_topn_batch(m, ok, corrupt_side=side)
    for bad in (np.array(["a", "likes"]), np.array([["a", "likes", "b"]]), np.zeros((2, 2, 2)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="queries"):
            query_topn_batch(m, bad)
    with pytest.raises(ValueError, match="use_filter"):
        query_topn_batch(m, ok, use_filter=True)
    with pytest.raises(ValueError, match="use_filter"):
        query_topn_batch(m, ok, use_filter=np.array([["a", "likes"]]))
    with pytest.raises(ValueError, match="1024"):
        query_topn_batch(m, ok, top_n=1025)
    with pytest.raises(ValueError, match="top_n"):
        query_topn_batch(m, ok, top_n=0)
    with pytest.raises(ValueError, match="ents_to_consider"):
        query_topn_batch(m, ok, ents_to_consider="a")
    with pytest.raises(ValueError, match="ents_to_consider"):
        query_topn_batch(m, ok, ents_to_consider=["a", "nobody"])
    # unseen labels are named, not dropped: entity and relation column, both sides
    with pytest.raises(ValueError, match=r"Entities not seen by the model: \['zed', 'yan'\]"):
        query_topn_batch(m, np.array([["zed", "likes"], ["a", "likes"], ["yan", "knows"], ["zed", "knows"]]))
    with pytest.raises(ValueError, match=r"Relations not seen by the model: \['hates'\]"):
        query_topn_batch(m, np.array([["a", "likes"], ["b", "hates"]]))
    with pytest.raises(ValueError, match=r"Entities not seen by the model: \['likes', 'knows'\]"):
        query_topn_batch(m, ok, corrupt_side="s")                         # [predicate, object] order: "likes" is no entity
    with pytest.raises(ValueError, match=r"Relations not seen by the model: \['b'\]"):
        query_topn_batch(m, np.array([["likes", "a"], ["b", "a"]]), corrupt_side="s")
    with pytest.raises(ValueError, match="not fitted"):
        query_topn_batch(_StubModel(fitted=False), ok)


def test_query_topn_batch_unwraps_compat_models():
    """A 1.x wrapper (is_backward, .model) is unwrapped as in find_duplicates: the inner model's state decides."""
    from ampligraph_amd.discovery import query_topn_batch

    class Wrapper:
        is_backward = True
        is_fitted = True

        def __init__(self, inner):
            self.model = inner

    with pytest.raises(ValueError, match="not fitted"):
        query_topn_batch(Wrapper(_StubModel(fitted=False)), np.array([["a", "likes"]]))
    with pytest.raises(ValueError, match=r"\['zed'\]"):
        query_topn_batch(Wrapper(_StubModel()), np.array([["zed", "likes"]]))
