"""discover_facts on the MI355X: the selection kernel of strategy="exhaustive" (amdkge_discover_select, kge_discover.hip) against numpy,
the exhaustive strategy against brute force -- model.evaluate over EVERY candidate of a relation, cut at top_n -- for the five
models, with tied and with large scores, and the sampled strategies end to end on a fitted model."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_kernels import dev, make_engine, rand_triples

pytestmark = pytest.mark.gpu

INT32_MIN = -(1 << 31)


# ------------------------------------------------------------------------------------------------ the selection kernel alone
def quantise64(V):
    """trunc(fp32(v * 1000)) as the kernels compute it, in int64 (finite values inside the int32 range)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.trunc(np.nan_to_num((V.astype(np.float32) * np.float32(1000.0)).astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)).astype(np.int64)


def select_numpy(V, own, flt, R, margin_q):
    """(sorted keys row * m + column of the emitted pairs, thresholds) of amdkge_discover_select's contract, one row at a time."""
    n, m = V.shape
    q = quantise64(V)
    keys, thr = [], np.empty(n, dtype=np.int64)
    for i in range(n):
        counted = np.ones(m, dtype=bool)
        ids = flt[i]
        counted[ids[(ids >= 0) & (ids < m)]] = False
        vals = np.sort(q[i][counted])[::-1]
        whole = len(vals) < R or not np.isfinite(V[i]).all()
        thr[i] = INT32_MIN if whole else vals[R - 1]
        emit = counted & (q[i] >= thr[i] - margin_q)
        if 0 <= own[i] < m:
            emit[own[i]] = False
        keys.append(i * m + np.flatnonzero(emit).astype(np.int64))
    return np.concatenate(keys), thr


def pair_keys(pairs, m, row_base=0):
    p = pairs.cpu().numpy().astype(np.int64)
    return np.sort((p[:, 0] - row_base) * m + p[:, 1])


def make_block(n, m, seed):
    rng = np.random.default_rng(seed)
    V = rng.normal(size=(n, m)).astype(np.float32) * 3
    V[:, : m // 2] = np.round(V[:, : m // 2], 2)                 # many exact ties after quantisation
    V[: n // 2] = np.round(V[: n // 2], 1)
    if n > 1 and m > 3:
        V[1, 2] = np.nan                                          # a row with a non-finite score is emitted whole
    own = rng.integers(0, m, n).astype(np.int32)
    flt = []
    for i in range(n):                                            # empty, partial and full filter ranges
        kind = i % 4
        cnt = 0 if kind == 0 else m if kind == 3 else int(rng.integers(1, max(2, m // 3)))
        flt.append(np.sort(rng.choice(m, cnt, replace=False)).astype(np.int32))
    return V, own, flt


def csr(flt):
    lens = np.array([len(f) for f in flt], dtype=np.int64)
    hi = np.cumsum(lens) + 5                                      # (ranges into a shared id array, not starting at 0)
    ids = np.concatenate([np.full(5, 1, np.int32)] + flt + [np.zeros(1, np.int32)])
    return dev(hi - lens), dev(hi), dev(ids)


@pytest.mark.parametrize("n,m,R,margin_q", [(9, 500, 1, 0), (9, 500, 19, 1), (8, 14541, 19, 3), (5, 3000, 1024, 1), (5, 3000, 1500, 2), (6, 12, 19, 1),
                                            (3, 300000, 19, 1),      # bitmap beyond the default dynamic-LDS limit
                                            (2, 1100000, 59, 1)])    # no bitmap: binary search in the id list
@pytest.mark.parametrize("side", [1, 2])
def test_select_rows_against_numpy(gpu_lib, n, m, R, margin_q, side):
    eng, _, _ = make_engine("DistMult", 4, 8, 3)
    V, own, flt = make_block(n, m, 1000 * R + m % 997 + side)
    queries = np.zeros((n, 3), dtype=np.int32)
    queries[:, 2 if side == 1 else 0] = own                       # the row's own entity: the object of a subject-side query
    queries[:, 0 if side == 1 else 2] = (own + 1) % m
    want, want_thr = select_numpy(V, own, flt, R, margin_q)
    pairs, thr = eng.select_rows(dev(V), dev(queries), side, R, margin_q, csr(flt), row_base=0)
    assert np.array_equal(pair_keys(pairs, m), want)              # (as a set: the order is free; no pair twice)
    assert np.array_equal(thr.cpu().numpy().astype(np.int64), want_thr)
    assert len(want) > 0


def test_select_rows_count_beyond_cap_and_retry(gpu_lib):
    from ampligraph_amd import _ffi

    eng, _, _ = make_engine("DistMult", 4, 8, 3)
    n, m, R = 7, 2000, 19
    V, own, flt = make_block(n, m, 5)
    queries = np.zeros((n, 3), dtype=np.int32)
    queries[:, 0] = own
    want, _ = select_numpy(V, own, flt, R, 1)
    lo, hi, ids = csr(flt)
    Vd, qd = dev(V), dev(queries)
    thr = torch.empty(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    small = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    _ffi.check(gpu_lib.amdkge_discover_select(p(Vd), n, m, m, p(qd), _ffi.SIDE_O, p(lo), p(hi), p(ids), R, 1, p(thr), 0, 100, p(small),
                                              3, p(count), None))
    torch.cuda.synchronize()
    assert int(count.item()) == len(want) > 3                      # the true count, whatever the capacity
    assert (small[3] == -7).all() and np.isin(pair_keys(small[:3], m, row_base=100), want).all()   # nothing beyond cap; row_base added
    pairs, _ = eng.select_rows(Vd, qd, _ffi.SIDE_O, R, 1, (lo, hi, ids), cap=3)   # the engine retries with the reported count
    assert np.array_equal(pair_keys(pairs, m), want)
    # argument checks of the entry point
    assert gpu_lib.amdkge_discover_select(p(Vd), n, m, m - 1, p(qd), 2, p(lo), p(hi), p(ids), R, 1, p(thr), 0, 0, p(small), 3, p(count), None) == -1      # ld < m
    assert gpu_lib.amdkge_discover_select(p(Vd), n, m, m, p(qd), 2, p(lo), p(hi), p(ids), 1025, 1, p(thr), 0, 0, p(small), 3, p(count), None) == -1       # R > 1024, no thresholds
    assert gpu_lib.amdkge_discover_select(p(Vd), n, m, m, p(qd), 3, p(lo), p(hi), p(ids), R, 1, p(thr), 0, 0, p(small), 3, p(count), None) == -1          # side
    assert gpu_lib.amdkge_discover_select(p(Vd), n, m, m, p(qd), 2, p(lo), None, p(ids), R, 1, p(thr), 0, 0, p(small), 3, p(count), None) == -1           # half a filter
    assert gpu_lib.amdkge_discover_select(p(Vd), n, m, m, p(qd), 2, p(lo), p(hi), p(ids), R, 1, p(thr), 0, 0, None, 3, p(count), None) == -1              # cap > 0, no buffer


# ------------------------------------------------------------------------------------------------ exhaustive == brute force
N_ENT, N_REL, N_TRI = 300, 4, 3000


def planted_model(model, k, tables, seed=0):
    """A ScoringBasedEmbeddingModel over N_ENT entities / N_REL relations (every one of them in X) whose tables are then SET:
    tables(rng, N, R, K) -> (ent, rel) dense fp32.  -> (model, X labels)."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    rng = np.random.default_rng(seed)
    Xi = np.stack([rng.integers(0, N_ENT, N_TRI), rng.integers(0, N_REL, N_TRI), rng.integers(0, N_ENT, N_TRI)], 1)
    X = np.char.add(np.array(["e", "r", "e"]), Xi.astype(str))
    m = ScoringBasedEmbeddingModel(eta=2, k=k, scoring_type=model, seed=1)
    m.compile(optimizer="adam", loss="nll")
    m.fit(X, batch_size=1000, epochs=1, verbose=False)
    assert m._n_ents == N_ENT and m._n_rels == N_REL
    ent, rel = tables(rng, N_ENT, N_REL, m._engine.K)
    m._engine.set_tables(ent.astype(np.float32), rel.astype(np.float32))
    m._placement.tables_written()
    return m, X


def normal_tables(scale):
    return lambda rng, N, R, K: (rng.normal(size=(N, K)) * scale, rng.normal(size=(R, K)) * scale)


def brute_force(m, X, rel_label):
    """Every candidate of the relation -- (s, r, o), s != o, not in X, all entities of the model -- in (subject id, object id) order
    with evaluate()'s mean rank: the definition of strategy="exhaustive"."""
    ix = m.data_indexer
    N = m._n_ents
    r = int(ix.get_indexes(np.asarray([rel_label]), "r")[0])
    s, o = np.divmod(np.arange(N * N, dtype=np.int64), N)
    Xi = ix.get_indexes(X).astype(np.int64)
    known = np.unique(Xi[Xi[:, 1] == r][:, 0] * N + Xi[Xi[:, 1] == r][:, 2])
    keep = (s != o) & ~np.isin(s * N + o, known)
    cand = ix.get_indexes(np.stack([s[keep], np.full(int(keep.sum()), r), o[keep]], 1), "t", "ind2raw")
    ranks = m.evaluate(cand, use_filter={"test": X}, corrupt_side="s,o", verbose=False)
    assert ranks.shape == (len(cand), 2)
    return cand, ranks.mean(1)


def check_exhaustive(m, X, rels, top_ns, brute=None):
    from ampligraph_amd.discovery import discover_facts

    brute = brute or {r: brute_force(m, X, r) for r in rels}
    found = {}
    for top_n in top_ns:
        got, ranks = discover_facts(X, m, top_n=top_n, strategy="exhaustive", target_rel=list(rels), max_candidates=3)
        want = np.concatenate([brute[r][0][brute[r][1] <= top_n] for r in rels])
        want_r = np.concatenate([brute[r][1][brute[r][1] <= top_n] for r in rels])
        print("exhaustive", m.scoring_type, "top_n", top_n, "found", len(want), "of", sum(len(brute[r][0]) for r in rels))
        assert got.shape == want.shape and ranks.shape == want_r.shape
        assert np.array_equal(got, want) and np.array_equal(ranks, want_r)
        found[top_n] = (len(want), sum(len(brute[r][0]) for r in rels))
    return found


@pytest.mark.parametrize("model,k,scale", [("TransE", 16, 0.3), ("DistMult", 16, 0.3), ("ComplEx", 50, 0.5), ("HolE", 16, 0.3), ("RotatE", 16, 0.3)])
def test_exhaustive_equals_brute_force(gpu_lib, model, k, scale):
    from ampligraph_amd.discovery import discover_facts

    m, X = planted_model(model, k, normal_tables(scale))
    rels = ["r0", "r1"]
    found = check_exhaustive(m, X, rels, (1, 5, 30))
    assert found[1][0] == 0                                        # a candidate counts among its own corruptions: every rank >= 2
    for top_n in (5, 30):
        assert 0 < found[top_n][0] < found[top_n][1]
    got, ranks = discover_facts(X, m, top_n=1, strategy="exhaustive", target_rel="r0")
    assert got.shape == (0, 3) and ranks.shape == (0,)
    if model == "DistMult":                                         # target_rel=None: every relation of the model, in id order
        ix = m.data_indexer
        order = ix.get_indexes(np.arange(N_REL), "r", "ind2raw").tolist()
        brute = {r: brute_force(m, X, r) for r in order}
        got, ranks = discover_facts(X, m, top_n=5, strategy="exhaustive")
        want = np.concatenate([brute[r][0][brute[r][1] <= 5] for r in order])
        assert np.array_equal(got, want) and np.array_equal(ranks, np.concatenate([brute[r][1][brute[r][1] <= 5] for r in order]))


@pytest.mark.parametrize("model", ["DistMult", "TransE"])
def test_exhaustive_with_tied_scores(gpu_lib, model):
    """Integer-valued tables: every fp32 sum is exact and the quantised scores take a few dozen values, so ranks are decided by ties."""
    from ampligraph_amd import _ffi

    m, X = planted_model(model, 8, lambda rng, N, R, K: (rng.integers(-2, 3, size=(N, K)), rng.integers(-2, 3, size=(R, K))), seed=1)
    found = check_exhaustive(m, X, ["r0", "r1"], (1, 5, 30))
    assert found[1][0] == 0 and 0 < found[5][0] < found[5][1] and 0 < found[30][0] < found[30][1]
    # the tie / margin path ran: some query row emitted more than R columns
    eng, ix = m._engine, m.data_indexer
    R = 9
    r_id = int(ix.get_indexes(np.asarray(["r0"]), "r")[0])
    ents = torch.arange(N_ENT, dtype=torch.int32, device=eng.device)
    q = torch.stack([ents, torch.full_like(ents, r_id), torch.zeros_like(ents)], 1).contiguous()
    fi = m._filter_index({"test": X}, None)
    pairs, thr = eng.corruption_select(q, _ffi.SIDE_O, R, eng.select_margin(r_id), fi.device_filter(eng, q, "o"))
    per_row = np.bincount(pairs[:, 0].cpu().numpy(), minlength=N_ENT)
    print("tied scores", model, "largest emission of a row", per_row.max(), "R", R)
    assert per_row.max() > R and (thr.cpu().numpy() > INT32_MIN).all()


def test_corruption_select_chunk_invariance(gpu_lib):
    """corruption_select walks the queries in chunks of SCORE_CHUNK_BYTES: 40 filtered queries against 300 entities, R = 8, seven
    queries per chunk, give the pairs (as a set: their order is free) and the thresholds of the one-chunk run exactly."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex

    N, n_rels, R = 300, 4, 8
    eng, _, _ = make_engine("ComplEx", 16, N, n_rels, scale=0.5)
    rng = np.random.default_rng(12)
    X = rand_triples(rng, 2000, N, n_rels)
    q = dev(X[:40])
    flt = FilterIndex([X], N, n_rels, engine=eng).device_filter(eng, q, "o")
    assert eng._score_chunks(40, N) == [(0, 40)]
    one = eng.corruption_select(q, _ffi.SIDE_O, R, 1, flt)
    eng.SCORE_CHUNK_BYTES = 4 * N * 7                                     # instance attribute: this engine only
    try:
        assert len(eng._score_chunks(40, N)) == 6
        many = eng.corruption_select(q, _ffi.SIDE_O, R, 1, flt)
    finally:
        del eng.SCORE_CHUNK_BYTES
    as_set = lambda pairs: np.sort(pairs[:, 0].cpu().numpy().astype(np.int64) * N + pairs[:, 1].cpu().numpy())   # noqa: E731
    assert len(one[0]) >= 40 * (R - 1) and np.array_equal(as_set(one[0]), as_set(many[0]))
    assert torch.equal(one[1], many[1]) and (one[1].cpu().numpy() > INT32_MIN).all()


@pytest.mark.parametrize("model,scale", [("DistMult", 6.0), ("ComplEx", 5.0), ("TransE", 300.0)])
def test_exhaustive_with_large_scores(gpu_lib, model, scale):
    """Tables scaled until the derived margin exceeds one quantum."""
    m, X = planted_model(model, 16, normal_tables(scale), seed=2)
    margins = [m._engine.select_margin(r) for r in range(N_REL)]
    print("large scores", model, "margin_q", margins)
    assert min(margins) > 1
    found = check_exhaustive(m, X, ["r0", "r1"], (5, 30))
    assert 0 < found[5][0] < found[5][1]


# ------------------------------------------------------------------------------------------------ end to end
def test_discover_facts_on_a_fitted_model(gpu_lib):
    from ampligraph_amd.discovery import discover_facts, generate_candidates
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    rng = np.random.default_rng(0)
    N, R = 120, 4
    X = np.stack([rng.integers(0, N, 900), rng.integers(0, R, 900), rng.integers(0, N, 900)], 1)
    X = np.char.add(np.array(["e", "r", "e"]), X.astype(str))
    m = ScoringBasedEmbeddingModel(eta=3, k=10, scoring_type="ComplEx", seed=2)
    m.compile(optimizer="adam", loss="multiclass_nll")
    with pytest.raises(ValueError, match="Model is not fitted."):
        discover_facts(X, m)
    m.fit(X, batch_size=300, epochs=3, verbose=False)
    with pytest.raises(ValueError, match="error is not a valid strategy."):
        discover_facts(X, m, strategy="error")
    with pytest.raises(ValueError, match="not found in model"):
        discover_facts(X, m, strategy="random_uniform", target_rel="error")
    for strategy, rel in (("random_uniform", "r1"), ("entity_frequency", ["r0", "r2"]), ("graph_degree", "r3")):
        got, ranks = discover_facts(X, m, top_n=40, strategy=strategy, max_candidates=200, target_rel=rel, seed=3)
        cand = generate_candidates(X, strategy, [rel] if isinstance(rel, str) else rel, 200, seed=3)
        mean = m.evaluate(cand, use_filter={"test": X}, corrupt_side="s,o", verbose=False).mean(1)
        assert len(mean) == len(cand)
        assert np.array_equal(got, cand[mean <= 40]) and np.array_equal(ranks, mean[mean <= 40]) and 0 < len(got) < len(cand)
    # and the exhaustive strategy on the same fitted model contains every sampled discovery of its relation
    got_x, ranks_x = discover_facts(X, m, top_n=40, strategy="exhaustive", target_rel="r1")
    got_s, ranks_s = discover_facts(X, m, top_n=40, strategy="random_uniform", max_candidates=200, target_rel="r1", seed=3)
    have = {tuple(t): r for t, r in zip(got_x.tolist(), ranks_x.tolist())}
    inX = {tuple(t) for t in X.tolist()}
    assert all(tuple(t) in inX or have.get(tuple(t)) == r for t, r in zip(got_s.tolist(), ranks_s.tolist()))
