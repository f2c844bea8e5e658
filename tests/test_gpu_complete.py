"""Batched, known-fact-filtered completion on the device: amdkge_topk_rows_excluding through the C ABI against numpy (exact: ids
and value bits), its agreement with amdkge_topk_rows when nothing is excluded, and discovery.query_topn_batch end to end
against query_topn and a numpy brute force over downloaded scores."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

SHAPES = [(3, 10, 4), (4, 7, 7), (1, 3, 5), (5, 3001, 10), (2, 5000, 1024), (6, 14505, 100), (1, 257, 1)]
ID_BASE = 7


# ------------------------------------------------------------------------------------------------------------ kernel vs numpy
def _engine():
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("DistMult", 4, 8, 3)


def _blocks(n, m, seed):
    """The score blocks of one shape: 16 distinct values (ties next to every excluded column; no zero, whose two signs numpy
    calls equal and the order-preserving key does not), and normal draws holding NaN, +inf and -inf."""
    rng = np.random.default_rng(seed)
    ties = np.linspace(-2.0, 2.0, 16).astype(np.float32)[rng.integers(0, 16, (n, m))]
    wild = rng.normal(size=(n, m)).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf):
        hit = rng.random((n, m)) < 0.02
        hit[:, rng.integers(0, m)] = True
        wild[hit] = v
    return {"ties": ties, "nonfinite": wild}


def _order(row):
    """Columns of one fp32 row, best first: stable descending, a NaN below everything (-inf included)."""
    nan = np.isnan(row)
    return np.lexsort((np.arange(row.shape[0]), -np.where(nan, 0.0, row.astype(np.float64)), nan))


def _reference(V, k, col_id, ex_sets, own):
    """Per row: drop the excluded columns, stable descending argsort of the same fp32 block, first k."""
    n, m = V.shape
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.full((n, k), -np.inf, dtype=np.float32)
    for i in range(n):
        gone = np.zeros(m, dtype=bool)
        if ex_sets is not None:
            gone |= np.isin(col_id, ex_sets[i])
        if own is not None:
            gone |= col_id == own[i]
        order = _order(V[i])
        order = order[~gone[order]][:k]
        idx[i, :len(order)] = order
        val[i, :len(order)] = V[i, order]
    return idx, val


def _csr(ex_sets, rng):
    """(lo, hi, ids) as amdkge_filter_ranges hands them over: one shared id array, ascending inside a range, the rows' ranges
    in arbitrary order behind a prefix no row owns; an empty set is the range lo == hi == 0."""
    n = len(ex_sets)
    parts, lo, hi = [np.array([3, 1, 2], dtype=np.int32)], np.zeros(n, np.int64), np.zeros(n, np.int64)
    at = 3
    for i in rng.permutation(n):
        s = np.unique(np.asarray(ex_sets[i], dtype=np.int32))
        if len(s):
            lo[i], hi[i] = at, at + len(s)
            parts.append(s)
            at += len(s)
    return dev(lo), dev(hi), dev(np.concatenate(parts))


def _patterns(V, col_id, foreign, rng):
    """name -> (excluded id sets per row or None, own ids or None).  L beyond the row length excludes the whole row."""
    n, m = V.shape
    best = [_order(V[i]) for i in range(n)]
    top = lambda L: [col_id[best[i][:L]] for i in range(n)]   # noqa: E731  (the case that matters: known facts score highest)
    out = {"none": (None, None)}
    for L in (1, 50, 1500):
        out["top%d" % L] = (top(L), None)
    out["random 1%"] = ([col_id[rng.choice(m, max(1, m // 100), replace=False)] for _ in range(n)], None)
    out["every column"] = ([col_id.copy() for _ in range(n)], None)
    out["ids that are no column"] = ([foreign[rng.choice(len(foreign), min(len(foreign), 40), replace=False)] for _ in range(n)], None)
    out["empty ranges on some rows"] = ([top(50)[i] if i % 2 == 0 else np.zeros(0, np.int32) for i in range(n)], None)
    own = np.array([col_id[best[i][0]] if i % 2 == 0 else foreign[i % len(foreign)] for i in range(n)], dtype=np.int32)
    out["own alone"] = (None, own)
    L = min(50, m - 1)
    out["own and a range"] = (top(L), np.array([col_id[best[i][L]] for i in range(n)], dtype=np.int32))   # the best column the range leaves
    return out


def _same(got_i, got_v, ref_i, ref_v, what):
    assert np.array_equal(got_i, ref_i), (what, got_i[0, :8], ref_i[0, :8])
    nan = np.isnan(ref_v)
    assert np.array_equal(np.isnan(got_v), nan), what
    assert np.array_equal(got_v.view(np.uint32)[~nan], ref_v.view(np.uint32)[~nan]), what


@pytest.mark.parametrize("n,m,k", SHAPES)
def test_topk_rows_excluding_against_numpy(gpu_lib, n, m, k):
    eng = _engine()
    rng = np.random.default_rng(1000 * m + k)
    shuffled = (rng.permutation(m) * 3 + 11).astype(np.int32)
    col_modes = {"id_base": (None, ID_BASE + np.arange(m, dtype=np.int32), np.arange(ID_BASE + m + 5, ID_BASE + m + 105, dtype=np.int32)),
                 "col_ids": (dev(shuffled), shuffled, (np.arange(m + 60, dtype=np.int32) * 3 + 12))}
    seen = set()
    for bname, V in _blocks(n, m, m + k).items():
        Vd = dev(V)
        for cname, (cd, col_id, foreign) in col_modes.items():
            for pname, (ex, own) in _patterns(V, col_id, foreign, rng).items():
                flt = None if ex is None else _csr(ex, rng)
                gi, gv = eng.topk_rows_excluding(Vd, k, cd, ID_BASE, flt, None if own is None else dev(own))
                ri, rv = _reference(V, k, col_id, ex, own)
                _same(gi.cpu().numpy(), gv.cpu().numpy(), ri, rv, (bname, cname, pname))
                if pname == "every column":
                    assert (ri == -1).all() and np.isneginf(rv).all()
                seen.add(pname)
    assert len(seen) == 10


def test_topk_rows_excluding_equals_topk_rows_without_exclusions(gpu_lib):
    """Three NULL range pointers and a NULL d_own: amdkge_topk_rows' output on the same block, bit for bit (a NaN's bits too)."""
    eng = _engine()
    for n, m, k in SHAPES:
        for bname, V in _blocks(n, m, m + k).items():
            Vd = dev(V)
            gi, gv = eng.topk_rows_excluding(Vd, k)
            ti, tv = eng.topk_rows(Vd, k)
            assert torch.equal(gi, ti) and torch.equal(gv.view(torch.int32), tv.view(torch.int32)), (n, m, k, bname)


def test_topk_rows_excluding_strided_block(gpu_lib):
    """ld > m: the rows of a wider buffer."""
    eng = _engine()
    rng = np.random.default_rng(3)
    W = rng.normal(size=(4, 700)).astype(np.float32)
    V = W[:, :611]
    col_id = ID_BASE + np.arange(611, dtype=np.int32)
    ex = [col_id[_order(V[i])[:20]] for i in range(4)]
    gi, gv = eng.topk_rows_excluding(dev(W)[:, :611], 9, None, ID_BASE, _csr(ex, rng), None)
    _same(gi.cpu().numpy(), gv.cpu().numpy(), *_reference(V, 9, col_id, ex, None), "strided")


# ------------------------------------------------------------------------------------------------------------ end to end
N_ENTS, N_RELS = 500, 5


def _fit(scoring_type):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    rng = np.random.default_rng(7)
    X = np.stack([rng.integers(0, N_ENTS, 4000), rng.integers(0, N_RELS, 4000), rng.integers(0, N_ENTS, 4000)], 1)
    X[:N_ENTS, 0] = np.arange(N_ENTS)   # every entity is seen
    X = np.char.add(np.array(["e", "r", "e"]), X.astype(str))
    m = ScoringBasedEmbeddingModel(eta=3, k=32, scoring_type=scoring_type, seed=3)
    m.compile(optimizer="adam", loss="nll")
    m.fit(X, batch_size=1000, epochs=2, verbose=False)
    return m, X


@pytest.fixture(scope="module", params=["ComplEx", "TransE"])   # the dot-product and the L1 mode of amdkge_corruption_scores' tile kernel
def fitted(request, gpu_lib):
    return _fit(request.param)


def _queries(X, side, count, rng):
    """(count, 2) label pairs: half of them the fixed elements of training statements (so they have known completions)."""
    cols = [0, 1] if side == "o" else [1, 2]
    seen = X[rng.integers(0, len(X), count // 2)][:, cols]
    ent = np.char.add("e", rng.integers(0, N_ENTS, count - count // 2).astype(str))
    rel = np.char.add("r", rng.integers(0, N_RELS, count - count // 2).astype(str))
    return np.concatenate([seen, np.stack([ent, rel] if side == "o" else [rel, ent], 1)])


def _device_scores(m, q_ids, side, cand=None):
    """The 1-vs-all scores of the id queries, downloaded: amdkge_corruption_scores in one call."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import _ptr, _stream

    eng = m._engine
    n = len(q_ids)
    ids = None if cand is None else dev(cand.astype(np.int32))
    cols = N_ENTS if cand is None else len(cand)
    blk = torch.empty(n, cols, dtype=torch.float32, device=eng.device)
    qd, work = dev(q_ids), eng._workspace(n)
    _ffi.check(eng.lib.amdkge_corruption_scores(C.byref(eng.model), _ptr(eng.ent), _ptr(eng.rel), _ptr(qd), n,
                                                _ffi.SIDE_O if side == "o" else _ffi.SIDE_S, _ptr(ids), 0, cols, _ptr(blk), cols,
                                                _ptr(work), _stream()))
    return blk.cpu().numpy()


def _id_queries(m, Q, side):
    ix = m.data_indexer
    ent = ix.get_indexes(Q[:, 0 if side == "o" else 1], "e")
    rel = ix.get_indexes(Q[:, 1 if side == "o" else 0], "r")
    return np.stack([ent, rel, ent], 1).astype(np.int32)


def _brute_force(m, X, Q, side, top_n, cand_labels=None, reflexive=False):
    """Labels / scores per query from the downloaded scores and the HOST filter index (FilterIndex.as_lists)."""
    from ampligraph_amd.datasets.filters import FilterIndex

    ix = m.data_indexer
    q = _id_queries(m, Q, side)
    cand = np.arange(N_ENTS) if cand_labels is None else np.asarray(ix.get_indexes(np.asarray(cand_labels), "e"), dtype=np.int64)
    S = _device_scores(m, q, side, None if cand_labels is None else cand)
    known = FilterIndex([ix.get_indexes(X)], N_ENTS, N_RELS).as_lists(q)[0 if side == "s" else 1] if X is not None else None
    labels = np.empty((len(Q), top_n), dtype=object)
    scores = np.full((len(Q), top_n), -np.inf, dtype=np.float32)
    raw = ix.get_indexes(cand, "e", "ind2raw")
    for i in range(len(Q)):
        gone = np.zeros(len(cand), dtype=bool)
        if known is not None:
            gone |= np.isin(cand, known[i])
        if reflexive:
            gone |= cand == q[i, 0]
        order = _order(S[i])
        order = order[~gone[order]][:top_n]
        labels[i, :len(order)] = raw[order]
        scores[i, :len(order)] = S[i, order]
    return labels, scores


def _equal(got, want):
    (gl, gs), (wl, ws) = got, want
    assert gl.shape == wl.shape and gl.dtype == object and gs.dtype == np.float32
    assert np.array_equal(gl, wl), np.argwhere(gl != wl)[:5]
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))


@pytest.mark.parametrize("side", ["o", "s"])
def test_batch_rows_equal_query_topn(fitted, side):
    """(a) unfiltered: row i is query_topn of query i, labels and score bits, with and without ents_to_consider."""
    from ampligraph_amd.discovery import query_topn, query_topn_batch

    m, X = fitted
    rng = np.random.default_rng(11)
    Q = _queries(X, side, 12, rng)
    subset = list(np.char.add("e", rng.choice(N_ENTS, 60, replace=False).astype(str)))
    for cons in (None, subset):
        L, S = query_topn_batch(m, Q, top_n=7, corrupt_side=side, ents_to_consider=cons)
        assert L.shape == (12, 7) and S.shape == (12, 7)
        for i, (a, b) in enumerate(Q):
            kw = dict(head=a, relation=b) if side == "o" else dict(relation=a, tail=b)
            Y, sc = query_topn(m, top_n=7, ents_to_consider=cons, **kw)
            assert np.array_equal(L[i], Y[:, 2 if side == "o" else 0]), (i, L[i], Y)
            assert np.array_equal(S[i].view(np.uint32), sc.view(np.uint32)), (i, S[i], sc)


@pytest.mark.parametrize("side", ["o", "s"])
def test_filtered_batch_against_brute_force(fitted, side):
    """(b) every row equals the numpy brute force over that query's scores without the host index's known ids; (c) no returned
    statement is a training statement."""
    from ampligraph_amd.discovery import query_topn_batch

    m, X = fitted
    rng = np.random.default_rng(12)
    Q = _queries(X, side, 400, rng)
    subset = list(np.char.add("e", rng.choice(N_ENTS, 150, replace=False).astype(str)))
    train = set(map(tuple, X.tolist()))
    for cons, flt in ((None, {"train": X}), (subset, {"train": X}), (None, X), (None, {"a": X[:1500], "b": X[1000:]})):
        got = query_topn_batch(m, Q, top_n=10, corrupt_side=side, use_filter=flt, ents_to_consider=cons)
        _equal(got, _brute_force(m, X, Q, side, 10, cons))
        for (a, b), row in zip(Q.tolist(), got[0].tolist()):
            for e in row:
                assert e is not None and ((a, b, e) if side == "o" else (e, a, b)) not in train
    unfiltered = query_topn_batch(m, Q, top_n=100, corrupt_side=side)   # (the filter had something to do)
    assert any(((a, b, e) if side == "o" else (e, a, b)) in train for (a, b), row in zip(Q.tolist(), unfiltered[0].tolist()) for e in row)


def test_all_candidates_known(fitted):
    """(d) a query whose known objects are all of ents_to_consider returns only None / -inf; one candidate more, and it is the
    only one returned."""
    from ampligraph_amd.discovery import query_topn_batch

    m, X = fitted
    s, p = X[0, 0], X[0, 1]
    known = sorted(set(X[(X[:, 0] == s) & (X[:, 1] == p), 2].tolist()))
    train = set(map(tuple, X.tolist()))
    other = next(e for e in np.unique(X[:, 2]).tolist() if e not in known and not any((e, p, o) in train for o in known))
    L, S = query_topn_batch(m, np.array([[s, p], [other, p]]), top_n=5, use_filter={"train": X}, ents_to_consider=known)
    assert all(e is None for e in L[0]) and np.isneginf(S[0]).all()
    assert L[1, 0] is not None                                   # (a row of its own query: the exclusion is per row)
    L, S = query_topn_batch(m, np.array([[s, p]]), top_n=5, use_filter={"train": X}, ents_to_consider=known + [other])
    assert L[0, 0] == other and all(e is None for e in L[0, 1:]) and np.isfinite(S[0, 0]) and np.isneginf(S[0, 1:]).all()


@pytest.mark.parametrize("side", ["o", "s"])
def test_exclude_reflexive_removes_exactly_the_own_entity(fitted, side):
    """(e) over the whole ranking (top_n beyond the entity count): the unrestricted list without the query's own entity."""
    from ampligraph_amd.discovery import query_topn_batch

    m, X = fitted
    Q = _queries(X, side, 20, np.random.default_rng(13))
    own = Q[:, 0 if side == "o" else 1]
    full_l, full_s = query_topn_batch(m, Q, top_n=N_ENTS + 12, corrupt_side=side)
    got_l, got_s = query_topn_batch(m, Q, top_n=N_ENTS + 12, corrupt_side=side, exclude_reflexive=True)
    for i in range(len(Q)):
        keep = full_l[i] != own[i]
        assert keep.sum() == N_ENTS + 11 and (full_l[i, N_ENTS:] == None).all()   # noqa: E711
        assert np.array_equal(got_l[i, :-1], full_l[i][keep]) and got_l[i, -1] is None and own[i] not in got_l[i].tolist()
        assert np.array_equal(got_s[i, :-1].view(np.uint32), full_s[i][keep].view(np.uint32)) and np.isneginf(got_s[i, -1])
    _equal(query_topn_batch(m, Q, top_n=10, corrupt_side=side, use_filter={"train": X}, exclude_reflexive=True),
           _brute_force(m, X, Q, side, 10, reflexive=True))


def test_chunked_equals_unchunked(fitted):
    """(f) 70 000 queries against 500 entities with the engine's score-block bound lowered so that the chunk loop runs four
    times: the result of the single-chunk run."""
    from ampligraph_amd.discovery import query_topn_batch

    m, X = fitted
    eng = m._engine
    Q = _queries(X, "o", 70000 - 2000, np.random.default_rng(14))
    Q = np.concatenate([Q, X[:2000, :2]])
    n = len(Q)
    assert n == 70000 and eng.SCORE_CHUNK_BYTES // (4 * N_ENTS) >= n      # one chunk by default
    kw = dict(top_n=10, use_filter={"train": X}, exclude_reflexive=True)
    whole = query_topn_batch(m, Q, **kw)
    try:
        eng.SCORE_CHUNK_BYTES = 4 * N_ENTS * 20000                       # instance attribute: this engine only
        parts = query_topn_batch(m, Q, **kw)
    finally:
        del eng.SCORE_CHUNK_BYTES
    _equal(parts, whole)
    _equal((whole[0][-300:], whole[1][-300:]), _brute_force(m, X, Q[-300:], "o", 10, reflexive=True))


def test_empty_batch(fitted):
    from ampligraph_amd.discovery import query_topn_batch

    m, X = fitted
    L, S = query_topn_batch(m, np.zeros((0, 2), dtype=str), top_n=4, use_filter={"train": X})
    assert L.shape == (0, 4) and L.dtype == object and S.shape == (0, 4) and S.dtype == np.float32


def test_sharded_placements_are_refused(gpu_lib):
    """Two in-process row-sharded engines: NotImplementedError on every rank (the per-shard column-to-id mapping is not built)."""
    from test_gpu_discovery import _fit_model
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.discovery import query_topn_batch

    def body(dist):
        m, X = _fit_model(dist, sharding=True)
        with pytest.raises(NotImplementedError, match="sharded"):
            query_topn_batch(m, X[:5, :2], top_n=3, use_filter={"train": X})
        return True

    assert ThreadedWorld(2).run(body) == [True, True]
