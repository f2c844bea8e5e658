"""Relation prediction on the device: amdkge_relation_scores bit for bit against amdkge_score on the materialised triples,
amdkge_relation_rank_counts / relation_rank against a numpy restatement, the device pair index against the host build, and
evaluate_relations / query_topn_relations against brute force over predict() -- single GPU and row-sharded.  Every comparison
is exact."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as O
from test_gpu_kernels import check_filter_range_case, dev, filter_range_case, make_engine, rand_triples

pytestmark = pytest.mark.gpu

N_ENT, N_REL = 500, 237
QUERY_COUNTS = (1, 7, 33, 257)         # no multiple of any queries-per-wave (4 / 2 / 1) or per-workgroup (16 / 8 / 4) choice
REL_COUNTS = (1, 7, 8, 9, 237)         # both sides of the eight-wide reduction


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def materialised(X, rel_ids):
    """[n * m, 3]: row i * m + j = (s_i, rel_ids[j], o_i)"""
    n, m = X.shape[0], len(rel_ids)
    T = np.empty((n, m, 3), dtype=np.int32)
    T[:, :, 0] = X[:, 0:1]
    T[:, :, 1] = np.asarray(rel_ids, dtype=np.int32)[None, :]
    T[:, :, 2] = X[:, 2:3]
    return T.reshape(-1, 3)


def reference_block(eng, X, rel_ids):
    """the yardstick: amdkge_score on the materialised triples, as a [n, m] array"""
    return eng.score(dev(materialised(X, rel_ids))).cpu().numpy().reshape(X.shape[0], len(rel_ids))


# (model, k, padded stored layout?)  -- which path each width takes is noted beside it
WIDTHS = [(mdl, 20, True) for mdl in ("TransE", "DistMult", "ComplEx", "HolE", "RotatE")] + \
         [(mdl, 200, True) for mdl in ("TransE", "DistMult", "ComplEx", "HolE", "RotatE")] + [   # nq < 64; the headline width
    ("DistMult", 256, True),     # nq == 64: every lane holds a group
    ("ComplEx", 300, True),      # two lane iterations, two queries per wave
    ("TransE", 300, True),       # two lane iterations, four queries per wave
    ("RotatE", 300, True),
    ("DistMult", 700, True),     # three lane iterations
    ("ComplEx", 1024, True),     # four lane iterations, one query per wave
    ("DistMult", 1024, True),    # four lane iterations, two queries per wave
    ("ComplEx", 1100, True),     # five lane iterations: the reload form on the padded layout
    ("DistMult", 37, False), ("ComplEx", 101, False), ("HolE", 25, False), ("TransE", 37, False), ("RotatE", 25, False),   # VEC = 1
    ("DistMult", 50, False), ("ComplEx", 202, False), ("RotatE", 50, False),                                                 # VEC = 2
]


@pytest.mark.parametrize("model,k,pad", WIDTHS, ids=["{}-{}{}".format(m_, k_, "" if p_ else "-unpadded") for m_, k_, p_ in WIDTHS])
def test_relation_scores_bits_equal_amdkge_score(gpu_lib, model, k, pad):
    eng, _, _ = make_engine(model, k, N_ENT, N_REL, seed=k, scale=0.3, pad=pad)
    rng = np.random.default_rng(k)
    X = rand_triples(rng, max(QUERY_COUNTS), N_ENT, N_REL)
    X[3] = X[2]                                                           # a repeated query
    Xd = dev(X)
    ref = reference_block(eng, X, np.arange(N_REL))                       # computed once, shared by every case below
    assert np.isfinite(ref).all() and len(np.unique(ref)) > ref.size // 2
    for n in QUERY_COUNTS:
        for m in REL_COUNTS:
            got = eng.relation_scores(Xd[:n], rel_hi=m)
            assert got.shape == (n, m)
            assert np.array_equal(bits(got), bits(ref[:n, :m])), (n, m)
    # a sub-range of the table
    got = eng.relation_scores(Xd[:33], rel_lo=5, rel_hi=118)
    assert np.array_equal(bits(got), bits(ref[:33, 5:118]))
    # a permuted id list with a repeated id, whole and as a sub-range of the list
    ids = rng.permutation(N_REL)[:41].astype(np.int32)
    ids[17] = ids[3]
    got = eng.relation_scores(Xd[:33], rel_ids=dev(ids))
    assert np.array_equal(bits(got), bits(ref[:33][:, ids]))
    got = eng.relation_scores(Xd[:7], rel_ids=dev(ids), rel_lo=2, rel_hi=19)
    assert np.array_equal(bits(got), bits(ref[:7][:, ids[2:19]]))
    # a strided block: ld > m, the padding columns are left untouched
    sentinel = np.float32(-12345.5)
    blk = torch.full((33, 24), float(sentinel), dtype=torch.float32, device=eng.device)
    out = eng.relation_scores(Xd[:33], rel_hi=9, out=blk)
    assert out.data_ptr() == blk.data_ptr()
    got = blk.cpu().numpy()
    assert np.array_equal(bits(got[:, :9]), bits(ref[:33, :9])) and (got[:, 9:] == sentinel).all()
    # empty batch, no candidates
    assert eng.relation_scores(Xd[:0]).shape == (0, N_REL) and eng.relation_scores(Xd[:3], rel_lo=4, rel_hi=4).shape == (3, 0)


# ------------------------------------------------------------------------------------------------ counts and ranks
def numpy_counts(S, pos, known_cols):
    """S [n, m] candidate scores, pos [n] positives' scores, known_cols[i] = the columns whose relation row i's filter holds"""
    qS, qp = O.quantise(S), O.quantise(pos)
    gt = (qp[:, None] < qS).sum(1)
    eq = (qp[:, None] == qS).sum(1)
    sub = np.array([sum(1 for j in cols if qp[i] <= qS[i, j]) for i, cols in enumerate(known_cols)], dtype=np.int64)
    return gt, eq, sub


def compose(gt, eq, sub, strategy):
    r = gt if strategy == "best" else (gt + (eq + 1) // 2 if strategy == "middle" else gt + eq)
    return (r - sub + 1).astype(np.int32)


def dyadic_engine(model, k, N, R, seed):
    """tables with entries j / 8: every product and sum is exact, so equal scores occur"""
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    rng = np.random.default_rng(seed)
    ent = (rng.integers(-4, 5, (N, eng.K)) / 8).astype(np.float32)
    rel = (rng.integers(-4, 5, (R, eng.K)) / 8).astype(np.float32)
    rel[R - 1] = rel[0]                                                   # two relations that always tie
    eng.set_tables(ent, rel)
    return eng


@pytest.mark.parametrize("model", ["TransE", "DistMult", "ComplEx"])
def test_relation_rank_against_numpy(gpu_lib, model):
    from ampligraph_amd.datasets.filters import PairFilterIndex

    N, R, n = 40, 19, 203
    eng = dyadic_engine(model, 6, N, R, seed=3)
    rng = np.random.default_rng(11)
    X = rand_triples(rng, n, N, R)
    Xd = dev(X)
    ref = reference_block(eng, X, np.arange(R))
    pos = eng.score(Xd).cpu().numpy()
    assert np.array_equal(bits(pos), bits(ref[np.arange(n), X[:, 1]]))
    known = np.concatenate([X[::2], rand_triples(rng, 600, N, R)])        # half of the test triples and unrelated statements
    sets = {}
    for s, p, o in known.tolist():
        sets.setdefault((s, o), set()).add(p)
    pfi = PairFilterIndex([known], N, R)
    flt = pfi.device_filter(eng, Xd)
    has_true = np.array([7, 0, 3, 18, 11, 5], dtype=np.int32)
    subsets = [None, has_true, np.array([2, 9, 4, 2, 16], dtype=np.int32)]   # the last: a repeated id, not every true relation inside
    assert not set(X[:, 1].tolist()) <= set(subsets[2].tolist())
    tied = 0
    for ids in subsets:
        cols = np.arange(R) if ids is None else ids
        S = ref[:, cols]
        col_of = {}
        for j, r in enumerate(cols.tolist()):
            col_of[r] = j                                                    # a repeated id: the last column
        for filtered in (False, True):
            kc = [[col_of[r] for r in sets.get((s, o), ()) if r in col_of] if filtered else [] for s, _, o in X.tolist()]
            gt, eq, sub = numpy_counts(S, pos, kc)
            tied += int((eq > 1).sum())
            for strategy in ("worst", "best", "middle"):
                ranks, counts, dsub = eng.relation_rank(Xd, strategy, flt if filtered else None, None if ids is None else dev(ids))
                counts = counts.cpu().numpy()
                assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq)
                if filtered:
                    assert np.array_equal(dsub.cpu().numpy(), sub)
                    assert sub.max() > 0
                else:
                    assert dsub is None
                assert np.array_equal(ranks.cpu().numpy(), compose(gt, eq, sub, strategy)), (strategy, filtered)
    assert tied > 0, "the dyadic tables must produce exact ties (eq > 1)"
    # the counts kernel ADDS: a second call over the same block doubles them
    blk = eng.relation_scores(Xd)
    counts = torch.zeros(n, 2, dtype=torch.int32, device=eng.device)
    for _ in range(2):
        rc = gpu_lib.amdkge_relation_rank_counts(blk.data_ptr(), n, R, R, dev(pos).data_ptr(), None, 0, None, None, None, None, counts.data_ptr(), None, None)
        assert rc == 0
    gt, eq, _ = numpy_counts(ref, pos, [[]] * n)
    assert np.array_equal(counts.cpu().numpy(), 2 * np.stack([gt, eq], 1))


# ------------------------------------------------------------------------------------------------ pair index
def test_pair_filter_index_device_build_equals_host_build(gpu_lib):
    from ampligraph_amd.datasets.filters import PairFilterIndex

    eng, _, _ = make_engine("DistMult", 4, 57, 9)
    rng = np.random.default_rng(8)
    a = rand_triples(rng, 3000, 57, 9)
    b = np.concatenate([a[500:900], rand_triples(rng, 700, 57, 9)])
    datasets = [a, np.zeros((0, 3), dtype=np.int32), b, a[:100]]
    host = PairFilterIndex(datasets, 57, 9)
    device = PairFilterIndex(datasets, 57, 9, engine=eng)
    for name in ("so_keys", "so_start", "r_ids"):
        got, want = getattr(device, name), getattr(host, name)
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    q = np.array([[s, 0, o] for s in range(57) for o in range(57)], dtype=np.int32)   # present and absent pairs
    lo, hi = host.relation_ranges(q)
    assert (hi == 0).any() and (hi > lo).any()
    for index in (device, host):                                                     # (the host-built one uploads itself)
        dlo, dhi, ids = index.device_filter(eng, dev(q))
        assert np.array_equal(dlo.cpu().numpy(), lo) and np.array_equal(dhi.cpu().numpy(), hi)
        assert np.array_equal(ids.cpu().numpy()[:host.r_ids.size], host.r_ids)
    dlo, dhi, _ = device.device_filter(eng, dev(q[:0]))
    assert dlo.shape == (0,) and dhi.shape == (0,)
    empty = PairFilterIndex([], 57, 9, engine=eng)
    assert empty.so_keys.size == 0 and empty.so_start.tolist() == [0] and empty.r_ids.size == 0
    dlo, dhi, _ = empty.device_filter(eng, dev(q[:5]))
    assert not dlo.any().item() and not dhi.any().item()
    # the one lookup kernel against the host ranges in the pair form (the entity-side forms: test_gpu_kernels.py): misses, keys
    # outside the index, the first and the last group, and an index with no keys
    X, T, N, R = filter_range_case()
    host, device = PairFilterIndex([X], N, R), PairFilterIndex([X], N, R, engine=eng)
    lo, hi = host.relation_ranges(T)
    check_filter_range_case(host.so_keys, T[:, 0].astype(np.int64) * N + T[:, 2], lo, hi)
    dlo, dhi, _ = device.device_filter(eng, dev(T))
    assert np.array_equal(dlo.cpu().numpy(), lo) and np.array_equal(dhi.cpu().numpy(), hi)
    dlo, dhi, ids = PairFilterIndex([], N, R, engine=eng).device_filter(eng, dev(T))
    assert dlo.shape == (200,) and not dlo.any().item() and not dhi.any().item() and ids.numel() >= 1


# ------------------------------------------------------------------------------------------------ the public surface
N_E, N_R = 60, 9
RELS = np.array(["r{}".format(j) for j in range(N_R)])


def _data():
    rng = np.random.default_rng(0)
    X = np.stack([rng.integers(0, N_E, 1200), rng.integers(0, N_R, 1200), rng.integers(0, N_E, 1200)], 1)
    X = np.unique(X, axis=0)
    rng.shuffle(X)
    L = np.char.add(np.array(["e", "r", "e"]), X.astype(str))
    return L[:900], L[900:1000], L[1000:]                                 # train, valid, test


def _fit(scoring, dist=None, sharding=False):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    train, _, _ = _data()
    m = ScoringBasedEmbeddingModel(eta=2, k=10, scoring_type=scoring, seed=4)
    if dist is not None:
        m._dist_override = dist
    kw = dict(entity_sharding="rows", sharded_negatives="global") if sharding else {}
    m.compile(optimizer="adam", loss="nll", **kw)
    m.fit(train, batch_size=300, epochs=2, verbose=False)
    return m


def _all_relation_scores(m, pairs):
    """predict() over the materialised label triples: [n, N_R] in the model's relation id order"""
    rel_labels = m.data_indexer.get_indexes(np.arange(N_R), "r", "ind2raw")
    T = np.stack([np.repeat(pairs[:, 0], N_R), np.tile(rel_labels, len(pairs)), np.repeat(pairs[:, 1], N_R)], 1)
    return m.predict(T).reshape(len(pairs), N_R), rel_labels


def _known_sets(datasets):
    sets = {}
    for d in datasets:
        for s, p, o in np.asarray(d).tolist():
            sets.setdefault((s, o), set()).add(p)
    return sets


def _brute_ranks(m, test, datasets, strategy, subset=None):
    S, rel_labels = _all_relation_scores(m, test[:, [0, 2]])
    col = {r: j for j, r in enumerate(rel_labels.tolist())}
    pos = S[np.arange(len(test)), [col[p] for p in test[:, 1].tolist()]]
    cand = list(range(N_R)) if subset is None else [col[r] for r in subset]
    sets = _known_sets(datasets)
    kc = [[cand.index(col[r]) for r in sets.get((s, o), ()) if col[r] in cand] for s, _, o in test.tolist()]
    gt, eq, sub = numpy_counts(S[:, cand], pos, kc)
    return compose(gt, eq, sub, strategy).reshape(-1, 1)


@pytest.mark.parametrize("scoring", ["ComplEx", "TransE", "RotatE"])
def test_evaluate_relations_against_brute_force(gpu_lib, scoring):
    from ampligraph_amd.evaluation import hits_at_n_score, mrr_score

    m = _fit(scoring)
    train, valid, test = _data()
    for use_filter, datasets in ((False, []), (True, [test]), ({"train": train, "valid": valid, "test": test}, [train, valid, test])):
        for strategy in ("worst", "middle"):
            got = m.evaluate_relations(test, use_filter=use_filter, ranking_strategy=strategy)
            assert got.dtype == np.int32 and got.shape == (len(test), 1)
            assert np.array_equal(got, _brute_ranks(m, test, datasets, strategy)), (use_filter is not False, strategy)
    sub = ["r3", "r0", "r7", "r5"]
    got = m.evaluate_relations(test, use_filter={"train": train, "test": test}, relations_subset=sub, ranking_strategy="best")
    assert np.array_equal(got, _brute_ranks(m, test, [train, test], "best", sub))
    assert not set(test[:, 1].tolist()) <= set(sub)
    # filtered with everything known, the true relation never loses to a known one: ranks are within the unknown candidates + 1
    full = m.evaluate_relations(test, use_filter={"train": train, "valid": valid, "test": test})
    assert 1 <= full.min() and full.max() <= N_R and 0 < mrr_score(full) <= 1 and 0 <= hits_at_n_score(full, 3) <= 1
    # rows with unseen labels are dropped, an empty batch works, chunked equals unchunked
    odd = np.concatenate([test[:5], np.array([["e1", "nope", "e2"], ["ghost", "r1", "e2"]]), test[5:9]])
    assert np.array_equal(m.evaluate_relations(odd), m.evaluate_relations(test[:9]))
    assert m.evaluate_relations(test[:0]).shape == (0, 1)
    want = m.evaluate_relations(test, use_filter=True)
    m._engine.SCORE_CHUNK_BYTES = 4 * N_R * 7                             # seven queries per chunk
    try:
        assert len(m._engine._score_chunks(len(test), N_R)) > 3
        assert np.array_equal(m.evaluate_relations(test, use_filter=True), want)
    finally:
        del m._engine.SCORE_CHUNK_BYTES


def _brute_topn(m, pairs, top_n, datasets, cand_labels=None):
    S, rel_labels = _all_relation_scores(m, pairs)
    col = {r: j for j, r in enumerate(rel_labels.tolist())}
    cand = list(range(N_R)) if cand_labels is None else [col[r] for r in cand_labels]
    sets = _known_sets(datasets)
    labels = np.empty((len(pairs), top_n), dtype=object)
    scores = np.full((len(pairs), top_n), -np.inf, dtype=np.float32)
    for i, (s, o) in enumerate(pairs.tolist()):
        live = [(c, j) for c, j in enumerate(cand) if rel_labels[j] not in sets.get((s, o), ())]
        live.sort(key=lambda cj: (-float(S[i, cj[1]]), cj[0]))            # best first, equal scores by candidate position
        for t, (c, j) in enumerate(live[:top_n]):
            labels[i, t], scores[i, t] = rel_labels[j], S[i, j]
    return labels, scores


@pytest.mark.parametrize("scoring", ["ComplEx", "TransE"])
def test_query_topn_relations_against_brute_force(gpu_lib, scoring):
    from ampligraph_amd.discovery import query_topn, query_topn_relations

    m = _fit(scoring)
    train, valid, test = _data()
    pairs = np.concatenate([test[:40, [0, 2]], train[:30, [0, 2]]])
    # unfiltered: row i is query_topn(head, tail), triples and score bits
    L, S = query_topn_relations(m, pairs, top_n=4)
    assert L.shape == (70, 4) and S.shape == (70, 4) and S.dtype == np.float32 and L.dtype == object
    for i in (0, 13, 41, 69):
        Y, sc = query_topn(m, top_n=4, head=pairs[i, 0], tail=pairs[i, 1])
        assert (Y[:, 0] == pairs[i, 0]).all() and (Y[:, 2] == pairs[i, 1]).all()
        assert np.array_equal(Y[:, 1], L[i].astype(Y.dtype)) and np.array_equal(bits(sc), bits(S[i]))
    bl, bs = _brute_topn(m, pairs, 4, [])
    assert np.array_equal(L, bl) and np.array_equal(bits(S), bits(bs))
    # filtered (dict and bare array), more wanted than there are candidates, a candidate list
    for top_n in (3, N_R + 2):
        L, S = query_topn_relations(m, pairs, top_n=top_n, use_filter={"train": train, "valid": valid})
        bl, bs = _brute_topn(m, pairs, top_n, [train, valid])
        assert np.array_equal(L, bl) and np.array_equal(bits(S), bits(bs))
    assert (L[:, -1] == None).all() and np.isneginf(S[:, -1]).all()       # noqa: E711  (fewer than top_n remain: None / -inf)
    cands = ["r6", "r1", "r8", "r2", "r1"]
    L, S = query_topn_relations(m, pairs, top_n=5, use_filter=train, rels_to_consider=cands)
    bl, bs = _brute_topn(m, pairs, 5, [train], cands)
    assert np.array_equal(L, bl) and np.array_equal(bits(S), bits(bs))
    # every relation of a pair known: an all-None / -inf row, the other rows unaffected
    s0, o0 = pairs[0]
    everything = np.stack([np.full(N_R, s0), RELS, np.full(N_R, o0)], 1)
    L, S = query_topn_relations(m, pairs[:3], top_n=4, use_filter={"all": everything})
    assert (L[0] == None).all() and np.isneginf(S[0]).all()               # noqa: E711
    bl, bs = _brute_topn(m, pairs[:3], 4, [everything])
    assert np.array_equal(L, bl) and np.array_equal(bits(S), bits(bs))
    # an empty batch; chunked equals unchunked
    L, S = query_topn_relations(m, pairs[:0], top_n=3)
    assert L.shape == (0, 3) and S.shape == (0, 3)
    want = query_topn_relations(m, pairs, top_n=5, use_filter=train)
    m._engine.SCORE_CHUNK_BYTES = 4 * N_R * 9
    try:
        got = query_topn_relations(m, pairs, top_n=5, use_filter=train)
    finally:
        del m._engine.SCORE_CHUNK_BYTES
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    with pytest.raises(ValueError, match=r"\['nobody'\]"):
        query_topn_relations(m, np.array([["e1", "nobody"]]))


def test_relation_prediction_row_sharded(gpu_lib):
    """Two engines on the one GPU (in-process rendezvous): both functions return on each rank exactly what the single-GPU model
    with the same tables returns; the queries span two (lowered) sharded chunks."""
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.discovery import query_topn_relations

    train, valid, test = _data()
    pairs = np.concatenate([test[:, [0, 2]], train[:50, [0, 2]]])
    flt = {"train": train, "valid": valid}

    def run(m):
        return (m.evaluate_relations(test, use_filter=flt), m.evaluate_relations(test, relations_subset=["r2", "r5", "r3"], ranking_strategy="middle"),
                query_topn_relations(m, pairs, top_n=4, use_filter=flt), query_topn_relations(m, pairs[:7], top_n=N_R + 1))

    def body(dist):
        m = _fit("ComplEx", dist, sharding=True)
        m.EVAL_CHUNK_SHARDED = 96                                         # (the scratch rows were sized for the default: larger)
        assert len(test) > 96 and len(pairs) > 96
        ent = m._placement.entity_table().cpu().numpy()                   # collective
        return run(m), ent, m._engine.rel.cpu().numpy(), m.data_indexer

    res = ThreadedWorld(2).run(body)
    single = _fit("ComplEx")
    assert np.array_equal(single.data_indexer.get_indexes(train), res[0][3].get_indexes(train))
    single._engine.ent.copy_(torch.as_tensor(res[0][1]).to(single._engine.device))    # the sharded model's tables (stored layout)
    single._engine.rel.copy_(torch.as_tensor(res[0][2]).to(single._engine.device))
    want = run(single)
    for rank in (0, 1):
        got = res[rank][0]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for g, w in zip(got[2:], want[2:]):
            assert np.array_equal(g[0], w[0]) and np.array_equal(bits(g[1]), bits(w[1]))
