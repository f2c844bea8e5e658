"""amdkge_rank_lists / KgeEngine.rank_lists / evaluate_candidates: ranks against PER-TRIPLE candidate lists.  Every comparison is
exact.  The yardstick is the declared-order oracle (oracle/rank_ordered.py) called one triple at a time with that triple's list as
the candidate rows; dyadic tables (entries j / 8, j in -4 .. 4) make equal scores and filter hits occur by the hundred."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_decl import declared_names
from oracle import kge_oracle as O
from oracle import rank_ordered as RO
from test_gpu_kernels import dev, dyadic_tables, make_engine, rand_triples

pytestmark = pytest.mark.gpu

N_ENT, N_REL, NQ = 3000, 11, 67          # 67 queries: no multiple of any queries-per-workgroup choice
LENS = (0, 1, 63, 64, 65, 500, 9000)     # 9000 > N_ENT: drawn with repeats, and long enough for several workgroups per query
SIDES = (("s", 1), ("o", 2))
MODELS5 = ("TransE", "DistMult", "ComplEx", "HolE", "RotatE")


def make_lists(rng, n, N, lens=LENS, dupfree=False):
    """per-query id lists whose lengths cycle through `lens`: permutation prefixes (duplicate-free) up to N entries, beyond that
    drawn with repeats -- or, dupfree, a permutation of the whole table"""
    out = []
    for i in range(n):
        L = lens[i % len(lens)]
        if L <= N or dupfree:
            out.append(rng.permutation(N)[:min(L, N)].astype(np.int32))
        else:
            out.append(rng.integers(0, N, L).astype(np.int32))
    return out


def tables(model, k, pad, kind, seed=3):
    """(engine, dense ent, dense rel): random tables of scale 0.3 or dyadic ones"""
    if kind == "random":
        return make_engine(model, k, N_ENT, N_REL, seed=seed, scale=0.3, pad=pad)
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(model, k, N_ENT, N_REL, max_rel_size=N_REL, pad=pad)
    ent, rel = dyadic_tables(np.random.default_rng(seed), N_ENT, N_REL, eng.K)
    eng.set_tables(ent, rel)
    return eng, ent, rel


def csr(lists):
    from ampligraph_amd.evaluation.candidates import as_csr

    return as_csr(lists, len(lists))


def cand_of(lists, max_len=None):
    off, ids, ml = csr(lists)
    return (dev(off[:-1].copy()), dev(off[1:].copy()), dev(ids), ml if max_len is None else max_len)


def oracle_counts(model, side, ent, rel, X, lists):
    """RO.side_counts one triple at a time, each against its own list -> (counts [n, 2], contexts)"""
    out, ctxs = np.zeros((len(lists), 2), np.int32), []
    for i, ids in enumerate(lists):
        c, ctx = RO.side_counts(model, side, ent, rel, X[i:i + 1], N_REL, ent_ids=ids)
        out[i] = c[0]
        ctxs.append(ctx)
    return out, ctxs


def device_filter(eng, F, X, N, R):
    """{side name: (lo, hi, ids)} from the DEVICE index (amdkge_filter_build + amdkge_filter_ranges) over the filter triples F"""
    Fd, Xd = dev(F), dev(X)
    flt = {}
    for nm, side in SIDES:
        keys, start, ids = eng.filter_build(Fd, nm, N, R)
        lo, hi = eng.filter_ranges(keys, start, Xd, side, N, R)
        flt[nm] = (lo, hi, ids)
    return flt


def intersecting_filter_set(rng, X, N, extra=2000):
    """the test triples plus `extra` random triples sharing their (p, o) / (s, p) keys: lists and filters do intersect"""
    j = rng.integers(0, X.shape[0], extra)
    A = X[j].copy()
    half = extra // 2
    A[:half, 0] = rng.integers(0, N, half)            # same (p, o), another subject
    A[half:, 2] = rng.integers(0, N, extra - half)    # same (s, p), another object
    return np.concatenate([X, A]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ 1. counts
PADDED = [(m, k) for m in MODELS5 for k in (20, 200)]
UNPADDED = [("DistMult", 37), ("ComplEx", 101), ("HolE", 25), ("TransE", 37)]


@pytest.mark.parametrize("kind", ["random", "dyadic"])
@pytest.mark.parametrize("model,k,pad", [(m, k, True) for m, k in PADDED] + [(m, k, False) for m, k in UNPADDED])
def test_counts_equal_the_ordered_oracle(gpu_lib, model, k, pad, kind):
    """(greater, equal) of both sides, lists of 0 .. 9000 entries: the chunked-gather kernel on padded rows, the lane-per-row
    fall-back on rows whose unit count is no multiple of 4.  Dyadic tables: the oracle must have seen ties."""
    eng, ent, rel = tables(model, k, pad, kind)
    assert (eng.Ks % 4 == 0) == pad
    rng = np.random.default_rng(100 + k)
    X = rand_triples(rng, NQ, N_ENT, N_REL)
    lists = make_lists(rng, NQ, N_ENT)
    Xd, cand = dev(X), cand_of(lists)
    assert cand[3] == 9000
    for nm, side in SIDES:
        ref, _ = oracle_counts(model, nm, ent, rel, X, lists)
        got = eng.rank_lists(Xd, side, cand)[1].cpu().numpy()
        print(model, k, pad, kind, nm, "gt", int(ref[:, 0].sum()), "eq", int(ref[:, 1].sum()), "differing", int((got != ref).sum()))
        if kind == "dyadic":
            assert ref[:, 1].sum() > 0, "no equal scores: ties were not exercised"
        assert np.array_equal(got, ref), (model, k, nm, np.argwhere(got != ref)[:5])
        assert np.array_equal(ref.sum(1) <= [len(x) for x in lists], np.ones(NQ, bool))


def test_max_len_only_plans(gpu_lib):
    """max_len smaller than the longest list (and 1): every list is still walked completely"""
    eng, ent, rel = tables("ComplEx", 20, True, "dyadic")
    rng = np.random.default_rng(5)
    X = rand_triples(rng, NQ, N_ENT, N_REL)
    lists = make_lists(rng, NQ, N_ENT)
    Xd = dev(X)
    for nm, side in SIDES:
        ref, _ = oracle_counts("ComplEx", nm, ent, rel, X, lists)
        for ml in (9000, 100, 1):
            got = eng.rank_lists(Xd, side, cand_of(lists, max_len=ml))[1].cpu().numpy()
            assert np.array_equal(got, ref), (nm, ml)


def test_rotate_exact_mode_needs_padded_rows(gpu_lib):
    from ampligraph_amd import _ffi

    eng, _, _ = make_engine("RotatE", 25, 300, 5, pad=False)
    X = rand_triples(np.random.default_rng(1), 5, 300, 5)
    with pytest.raises(_ffi.AmdKgeError) as e:
        eng.rank_lists(dev(X), 1, cand_of([np.arange(10, dtype=np.int32)] * 5))
    assert e.value.code == -5 and "padded" in str(e.value)   # AMDKGE_EUNSUPPORTED, as amdkge_rank_filter


# ------------------------------------------------------------------------------------------------------------------ 2. padding
@pytest.mark.parametrize("model,k,pad", [("ComplEx", 20, True), ("TransE", 37, False)])
def test_padded_dense_block_equals_ragged_lists(gpu_lib, model, k, pad):
    """a dense [n, 70] block whose rows are filled up with -1 and one id >= N_ENT: the counts of the ragged lists"""
    eng, ent, rel = tables(model, k, pad, "dyadic")
    rng = np.random.default_rng(9)
    X = rand_triples(rng, NQ, N_ENT, N_REL)
    lists = make_lists(rng, NQ, N_ENT, lens=(0, 1, 63, 64, 65, 69))
    block = np.full((NQ, 70), -1, np.int32)
    for i, ids in enumerate(lists):
        block[i, :len(ids)] = ids
        block[i, len(ids)] = N_ENT + (i % 3) * 1000 if i % 2 else -1 - i      # the first padding slot: past the table, or negative
    block[3, -1] = np.iinfo(np.int32).max
    from ampligraph_amd.evaluation.candidates import as_csr

    off, ids, ml = as_csr(block, NQ)
    assert ml == 70
    Xd = dev(X)
    for nm, side in SIDES:
        ref, _ = oracle_counts(model, nm, ent, rel, X, lists)
        ragged = eng.rank_lists(Xd, side, cand_of(lists))[1].cpu().numpy()
        dense = eng.rank_lists(Xd, side, (dev(off[:-1].copy()), dev(off[1:].copy()), dev(ids), ml))[1].cpu().numpy()
        assert np.array_equal(ragged, ref) and np.array_equal(dense, ref), nm


# ------------------------------------------------------------------------------------------------------------------ 3. filtered ranks
@pytest.mark.parametrize("model", MODELS5)
def test_filtered_ranks_equal_the_ordered_oracle(gpu_lib, model):
    """Duplicate-free lists, the filter ranges of the DEVICE index over (test triples + 2000 triples sharing their keys): the ranks
    of RO.evaluate_ranks(x[i:i+1], entities_subset=list_i), three strategies, both sides.  (An EMPTY list has no candidate: rank
    1; the oracle, like the reference, reads an empty entities_subset as "no subset", so that expectation is written out.)"""
    eng, ent, rel = tables(model, 20, True, "dyadic")
    rng = np.random.default_rng(17)
    X = rand_triples(rng, NQ, N_ENT, N_REL)
    lists = make_lists(rng, NQ, N_ENT, dupfree=True)
    assert all(len(np.unique(x)) == len(x) for x in lists) and max(map(len, lists)) == N_ENT
    F = intersecting_filter_set(rng, X, N_ENT)
    flt = device_filter(eng, F, X, N_ENT, N_REL)
    fs, fo = O.filter_sets(X, [F])
    Xd, cand = dev(X), cand_of(lists)
    keep = np.zeros(N_ENT, bool)
    for (nm, side), fl in zip(SIDES, (fs, fo)):
        # the oracle's subtraction, for the "filters were exercised" check and against the device's own
        ref_counts, ctxs = oracle_counts(model, nm, ent, rel, X, lists)
        ref_sub = np.zeros(NQ, np.int32)
        for i, ids in enumerate(lists):
            keep[:] = False
            keep[ids] = True
            ref_sub[i] = RO.filter_sub(ctxs[i], [fl[i]], keep)[0]
        assert ref_sub.sum() > 0, "no filter hit: the subtraction was not exercised"
        for strategy in ("worst", "best", "middle"):
            ranks, counts, sub = eng.rank_lists(Xd, side, cand, strategy, flt[nm])
            assert np.array_equal(counts.cpu().numpy(), ref_counts) and np.array_equal(sub.cpu().numpy(), ref_sub), (nm, strategy)
            ref = np.ones(NQ, np.int32)
            for i, ids in enumerate(lists):
                if len(ids):
                    kw = dict(filters_s=[fl[i]]) if nm == "s" else dict(filters_o=[fl[i]])
                    ref[i] = RO.evaluate_ranks(model, ent, rel, X[i:i + 1], corrupt_side=nm, ranking_strategy=strategy,
                                               entities_subset=ids, max_rel_size=N_REL, **kw)[0, 0]
            assert np.array_equal(ranks.cpu().numpy(), ref), (model, nm, strategy)
        print(model, nm, "sub total", int(ref_sub.sum()), "eq total", int(ref_counts[:, 1].sum()))


def test_known_positive_listed_twice_is_subtracted_twice(gpu_lib):
    """The documented duplicate rule.  Setup: DistMult, dyadic tables, side s; triple i's list is 40 distinct entities that are no
    known positive of it, with its OWN subject s_i put in at positions 7 and 23.  The filter set is the test triples, so s_i is a
    known positive of triple i; its corruption IS the triple, so its quantised score equals q(pos) and both occurrences
    outrank ("<=").  Then sub = 2 = (gt + eq over the list) - (gt + eq over the list without its known occurrences), where the
    reference, whose subset is a set, would subtract 1."""
    eng, ent, rel = tables("DistMult", 20, True, "dyadic")
    rng = np.random.default_rng(23)
    n = 9
    X = rand_triples(rng, n, N_ENT, N_REL)
    X[:, 1] = np.arange(n) % N_REL
    X[:, 2] = rng.permutation(N_ENT)[:n]               # distinct (p, o) keys: triple i's only known subject is s_i
    lists, bare = [], []
    for i in range(n):
        others = np.setdiff1d(rng.permutation(N_ENT)[:41], [X[i, 0]])[:40].astype(np.int32)
        bare.append(others)
        lists.append(np.insert(others, [7, 22], X[i, 0]).astype(np.int32))
        assert (lists[-1] == X[i, 0]).sum() == 2 and lists[-1][7] == X[i, 0] and lists[-1][23] == X[i, 0]
    flt = device_filter(eng, X, X, N_ENT, N_REL)["s"]
    ranks, counts, sub = eng.rank_lists(dev(X), 1, cand_of(lists), "worst", flt)
    full, _ = oracle_counts("DistMult", "s", ent, rel, X, lists)
    without, _ = oracle_counts("DistMult", "s", ent, rel, X, bare)
    want = full.sum(1) - without.sum(1)
    assert np.array_equal(want, np.full(n, 2))
    assert np.array_equal(counts.cpu().numpy(), full) and np.array_equal(sub.cpu().numpy(), want)
    assert np.array_equal(ranks.cpu().numpy(), without.sum(1) + 1)


# ------------------------------------------------------------------------------------------------------------------ 4. whole-table lists
@pytest.mark.parametrize("model", ["ComplEx", "TransE", "RotatE"])
def test_whole_table_lists_equal_rank_side(gpu_lib, model):
    """every list = arange(N): the ranks of the existing 1-vs-all path (screened / early exit at this size), filtered and not"""
    N, R, n, k = 700, 7, 130, 64
    eng, ent, rel = make_engine(model, k, N, R, seed=4, scale=0.3)
    rng = np.random.default_rng(31)
    X = rand_triples(rng, n, N, R)
    flt = device_filter(eng, intersecting_filter_set(rng, X, N, extra=600), X, N, R)
    Xd = dev(X)
    block = np.tile(np.arange(N, dtype=np.int32), (n, 1))
    off = np.arange(n + 1, dtype=np.int64) * N
    cand = (dev(off[:-1].copy()), dev(off[1:].copy()), dev(block.reshape(-1)), N)
    for nm, side in SIDES:
        for f in (None, flt[nm]):
            for strategy in ("worst", "middle"):
                want, wc, ws = eng.rank_side(Xd, side, strategy, f)
                got, gc, gs = eng.rank_lists(Xd, side, cand, strategy, f)
                assert torch.equal(gc, wc) and (f is None or torch.equal(gs, ws)) and torch.equal(got, want), (model, nm, f is not None, strategy)


# ------------------------------------------------------------------------------------------------------------------ 5. scores
@pytest.mark.parametrize("model,k,pad", [("ComplEx", 20, True), ("TransE", 20, True), ("RotatE", 20, True), ("HolE", 200, True), ("DistMult", 37, False)])
def test_scores_have_the_bits_of_corruption_scores(gpu_lib, model, k, pad):
    from ampligraph_amd import _ffi

    eng, ent, rel = tables(model, k, pad, "random")
    rng = np.random.default_rng(41)
    n = 7
    X = rand_triples(rng, n, N_ENT, N_REL)
    lists = make_lists(rng, n, N_ENT, lens=(1, 63, 64, 65, 500, 130, 9000))
    for i in (1, 3, 4):                                    # ids that are no candidates, in the middle of a list
        lists[i][5] = -1
        lists[i][len(lists[i]) // 2] = N_ENT
    Xd, cand = dev(X), cand_of(lists)
    off = csr(lists)[0]
    for nm, side in SIDES:
        plain = eng.rank_lists(Xd, side, cand)[1]
        _, counts, _, scores = eng.rank_lists(Xd, side, cand, want_scores=True)
        assert torch.equal(counts, plain)                  # asking for the scores changes no count
        scores = scores.cpu().numpy()
        for i, ids in enumerate(lists):
            got = scores[off[i]:off[i + 1]]
            ok = (ids >= 0) & (ids < N_ENT)
            assert np.all(np.isneginf(got[~ok]))
            good = np.ascontiguousarray(ids[ok])
            ref = torch.empty(len(good), dtype=torch.float32, device="cuda")
            work, gd = eng._workspace(1), dev(good)
            _ffi.check(eng.lib.amdkge_corruption_scores(C.byref(eng.model), C.c_void_p(eng.ent.data_ptr()), C.c_void_p(eng.rel.data_ptr()),
                                                        C.c_void_p(Xd[i:i + 1].data_ptr()), 1, side, C.c_void_p(gd.data_ptr()), 0,
                                                        len(good), C.c_void_p(ref.data_ptr()), len(good), C.c_void_p(work.data_ptr()), None))
            torch.cuda.synchronize()
            assert np.array_equal(got[ok].view(np.int32), ref.cpu().numpy().view(np.int32)), (model, nm, i)


# ------------------------------------------------------------------------------------------------------------------ 6. guard bands
def case_rank_lists(ar, model, k, flt, scores, n=37, N=130, R=5):
    """every device argument between bands, the workspace at offset 16; ragged lists (one empty, one with ids outside the table, the
    last one ending with the last row), the filter ranges ascending as the index build leaves them"""
    from test_gpu_guard_bands import P, Tables, _lib, edge_triples

    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad=k % 4 == 0 or model != "TransE")
    rng = np.random.default_rng(2)
    X = edge_triples(2, n, N, R)
    lens = rng.integers(0, 150, n)
    lens[0], lens[-1] = 0, 67
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    ids = rng.integers(0, N, int(off[-1])).astype(np.int32)
    ids[off[5]:off[5] + 2] = (-1, N)
    ids[-1] = N - 1
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    lo, hi, cid = ar.put("cand_lo", off[:-1].copy()), ar.put("cand_hi", off[1:].copy()), ar.put("cand_ids", ids)
    flo = fhi = fid = sub = sc = None
    if flt:
        cnt = rng.integers(0, 6, n)
        cnt[-1] = 5
        start = np.zeros(n + 1, np.int64)
        start[1:] = np.cumsum(cnt)
        fids = np.concatenate([np.sort(rng.permutation(N)[:c]) for c in cnt]).astype(np.int32)
        fids[-1] = N - 1
        flo, fhi, fid = ar.put("flt_lo", start[:-1].copy()), ar.put("flt_hi", start[1:].copy()), ar.put("flt_ids", fids)
        sub = ar.out("sub", (n,), np.int32, 0)
    if scores:
        sc = ar.out("scores", (int(off[-1]),), np.float32, 7.0)
    counts = ar.out("counts", (n, 2), np.int32, 0)
    work = ar.work("work", lib.amdkge_rank_lists_workspace_bytes(C.byref(T.m), n))
    _ffi.check(lib.amdkge_rank_lists(C.byref(T.m), P(ent), P(rel), N, P(tri), n, _ffi.SIDE_O, P(lo), P(hi), P(cid), int(lens.max()),
                                     P(flo), P(fhi), P(fid), P(counts), P(sub), P(sc), P(work), None))
    valid = np.array([((ids[a:b] >= 0) & (ids[a:b] < N)).sum() for a, b in zip(off[:-1], off[1:])])
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["counts"].sum(1) <= valid, True))
    if flt:
        ar.expects.append(lambda o: np.testing.assert_array_equal((o["sub"] >= 0) & (o["sub"] <= o["counts"].sum(1)), True))
    if scores:
        ar.expects.append(lambda o: np.testing.assert_array_equal(np.isneginf(o["scores"]), ~((ids >= 0) & (ids < N))))


# entry point of include/amdkge_lists.h -> [(case function, its arguments), ...] / the reason it has none
LIST_CASES = {
    "amdkge_rank_lists": [(case_rank_lists, dict(model=m, k=k, flt=f, scores=s))
                          for m, k in (("ComplEx", 50), ("TransE", 7), ("RotatE", 50)) for f, s in ((False, False), (True, True))],
}
LIST_EXEMPT = {
    "amdkge_rank_lists_workspace_bytes": "size function: the rank-lists cases allocate exactly what it returns",
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id="-".join(str(v) for v in kw.values())) for cases in LIST_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    from test_gpu_guard_bands import run_case

    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case_or_a_reason():
    """include/amdkge_lists.h's twin of tests/test_guard_bands_host.py::test_every_header_entry_has_a_case_or_a_reason"""
    declared = declared_names("amdkge_lists.h")
    assert declared and declared == set(LIST_CASES) | set(LIST_EXEMPT), declared ^ (set(LIST_CASES) | set(LIST_EXEMPT))
    assert not set(LIST_CASES) & set(LIST_EXEMPT) and all(LIST_CASES.values()) and all(LIST_EXEMPT.values())


# ------------------------------------------------------------------------------------------------------------------ 7. the model
@pytest.fixture(scope="module")
def fitted():
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(5, n=900)
    m = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type="ComplEx", seed=1)
    m.compile(optimizer="adam", loss="nll")
    m.fit(X[:800], batch_size=300, epochs=2, verbose=False)
    known = set(X[:800, 0]) | set(X[:800, 2])
    test = np.array([t for t in X[800:] if t[0] in known and t[2] in known and t[1] in set(X[:800, 1])])[:20]
    return m, X[:800], test, np.array(sorted(known))


@pytest.mark.parametrize("use_filter", ["none", "self", "dict"])
def test_evaluate_candidates_equals_evaluate_row_by_row(gpu_lib, fitted, use_filter):
    """2-D and ragged label lists (duplicate-free) == evaluate(x[i:i+1], entities_subset=list_i), row by row.  use_filter=True
    filters with the WHOLE evaluated array, so its row-by-row twin is evaluate(x[i:i+1], use_filter={"x": x})."""
    from ampligraph_amd.evaluation import mrr_score

    m, train, test, ents = fitted
    rng = np.random.default_rng(3)
    n = test.shape[0]
    C_ = 25
    block_s = np.stack([rng.permutation(ents)[:C_] for _ in range(n)])
    block_o = np.stack([rng.permutation(ents)[:C_] for _ in range(n)])
    ragged_s = [block_s[i, :1 + (7 * i) % C_] for i in range(n)]
    ragged_o = [list(block_o[i, :1 + (3 * i) % C_]) for i in range(n)]
    uf, uf_row = {"none": (False, False), "self": (True, {"x": test}), "dict": ({"train": train, "test": test},) * 2}[use_filter]
    for cs, co in ((block_s, block_o), (ragged_s, ragged_o)):
        for strategy in ("worst", "middle"):
            got = m.evaluate_candidates(test, candidates_s=cs, candidates_o=co, use_filter=uf, ranking_strategy=strategy)
            assert got.shape == (n, 2) and got.dtype == np.int32 and got.min() >= 1
            ref = np.stack([np.concatenate([m.evaluate(test[i:i + 1], use_filter=uf_row, corrupt_side=sd, entities_subset=list(c[i]),
                                                       ranking_strategy=strategy, verbose=False)[0] for sd, c in (("s", cs), ("o", co))])
                            for i in range(n)])
            assert np.array_equal(got, ref), (use_filter, strategy, np.argwhere(got != ref)[:5])
            only_o = m.evaluate_candidates(test, candidates_o=co, use_filter=uf, ranking_strategy=strategy)
            assert only_o.shape == (n, 1) and np.array_equal(only_o[:, 0], got[:, 1])
    assert 0.0 < mrr_score(got) <= 1.0


def test_evaluate_candidates_refuses_what_would_misalign(gpu_lib, fitted):
    m, train, test, ents = fitted
    n = test.shape[0]
    good = [list(ents[:3])] * n
    with pytest.raises(ValueError, match="candidates_s"):
        m.evaluate_candidates(test, candidates_s=[list(ents[:2]) + ["nobody"]] + good[1:])          # an unknown candidate label
    bad_x = test.copy()
    bad_x[2, 0] = "nobody"
    with pytest.raises(ValueError, match=f"1 of the {n} rows"):
        m.evaluate_candidates(bad_x, candidates_s=good)                                              # a row of x with an unseen entity
    with pytest.raises(ValueError, match=f"{n - 1} candidate lists for {n} triples"):
        m.evaluate_candidates(test, candidates_o=good[1:])
    with pytest.raises(ValueError, match="candidates_s"):
        m.evaluate_candidates(test)
    with pytest.raises(ValueError, match="ranking_strategy"):
        m.evaluate_candidates(test, candidates_s=good, ranking_strategy="median")
    with pytest.raises(ValueError, match="use_filter"):
        m.evaluate_candidates(test, candidates_s=good, use_filter="yes")
    empty = m.evaluate_candidates(test, candidates_s=[[] for _ in range(n)])                         # no candidate: rank 1
    assert np.array_equal(empty, np.ones((n, 1), np.int32))
    assert m.evaluate_candidates(test[:0], candidates_s=[], candidates_o=[]).shape == (0, 2)
