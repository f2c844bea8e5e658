"""Type-constrained negatives and evaluation on the GPU (include/amdkge_types.h): the relation-set build and its range lookup
against tests/types_ref.py exactly, amdkge_sample_negatives_typed against the numpy restatement of the draw bit for bit (outputs and
the three counters), its two identities with amdkge_sample_negatives, set membership, compile(negatives=TypedNegatives) end to end
against a stub sampler that uploads the restatement's rows, and evaluate_typed() against evaluate_candidates() on the materialised
sets and against evaluate() where nothing is constrained."""
import ctypes as C

import numpy as np
import pytest
import torch

import negatives_ref as NR
import types_ref as TR
from test_gpu_negatives import Graph, P, dev, gpu_sample

pytestmark = pytest.mark.gpu

SEED, STEP = 12345678901234, (1 << 33) + 5
MODES = [NR.UNIFORM, NR.BERNOULLI, NR.S_ONLY, NR.O_ONLY]


# ------------------------------------------------------------------------------------------------------------------ the planted graph
class Planted:
    """N = 37, R = 5, by hand:
      relation 0: the complete bipartite D0 x R0, 4 x 5 -- every member of R0 is a KNOWN object of every (s, 0): with the filter on,
                  every typed object draw of such a positive is rejected, so those corruptions exhaust by construction
      relation 1: one triple -- sets of one id: below min_size = 2, drawn by the untyped rule
      relation 2: sparse random rows, some of them twice
      relation 3: no training triple; its sets are given explicitly (D3, R3)
      relation 4: training triples, but NO sets: unconstrained"""

    N, R = 37, 5
    D0, R0 = [0, 1, 2, 3], [10, 11, 12, 13, 14]
    D3, R3 = [30, 31, 36], [0, 5, 20, 21]

    def __init__(self):
        rng = np.random.default_rng(11)
        r0 = [(s, 0, o) for s in self.D0 for o in self.R0]
        r1 = [(5, 1, 20)]
        r2 = [(int(s), 2, int(o)) for s, o in zip(rng.integers(0, self.N, 24), rng.integers(0, self.N, 24))]
        r2 += r2[:6]                                                       # duplicate rows
        r4 = [(int(s), 4, int(o)) for s, o in zip(rng.integers(0, self.N, 12), rng.integers(0, self.N, 12))]
        self.train = np.array(r0 + r1 + r2 + r4, np.int32)
        self.graph = Graph(self.train, self.N, self.R)                     # the known statements: FilterIndex, Bernoulli thresholds
        r3 = [(s, 3, o) for s in self.D3 for o in self.R3]
        self.typed_rows = np.array(r0 + r1 + r2 + r3, np.int32)            # what the sets are built from
        self.csr = {sd: TR.build_sets(self.typed_rows, sd) for sd in "so"}
        assert self.csr["s"][0].tolist() == [0, 1, 2, 3] and self.csr["o"][2][:5].tolist() == self.R0
        pick = np.array(r0 + r1 * 3 + r2 + r3 + r4, np.int32)
        order = rng.permutation(len(pick))
        self.pick = pick[np.concatenate([order, order[::-1], order, order[::-1]])]   # > 257 rows, every kind in the first 63
        self.pick[0] = r0[7]

    def batch(self, B):
        return np.ascontiguousarray(self.pick[:B])

    def cand(self, X, min_size=2):
        """((lo, hi, ids) subject side, (lo, hi, ids) object side) of the rows X, the untyped fallback (0, 0)"""
        return tuple((*TR.ranges(self.csr[sd][0], self.csr[sd][1], X, min_size, (0, 0)), self.csr[sd][2]) for sd in "so")


@pytest.fixture(scope="module")
def planted():
    return Planted()


def gpu_typed(X, eta, seed=SEED, step=STEP, sample_base=0, sample_range=None, row_offset=0, b_global=0, side_mode=NR.UNIFORM, side_thr=None,
              pool=None, s_filter=None, o_filter=None, max_tries=8, s_cand=None, o_cand=None):
    """amdkge_sample_negatives_typed with types_ref.sample_negatives_typed's arguments -> (rows, redraws, exhausted, untyped)"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    B = len(X)
    tri = dev(np.asarray(X, dtype=np.int32))
    out = torch.full((B * eta, 3), -7, dtype=torch.int32, device="cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    thr = None if side_thr is None else dev(np.asarray(side_thr, dtype=np.uint32).view(np.int32))
    pl = None if pool is None else dev(np.asarray(pool, dtype=np.int32))

    def six(a, b):
        if a is None:
            return [None] * 6
        return [dev(np.asarray(v, dtype=dt)) for grp in (a, b) for v, dt in zip(grp, (np.int64, np.int64, np.int32))]

    f, c = six(s_filter, o_filter), six(s_cand, o_cand)
    _ffi.check(lib.amdkge_sample_negatives_typed(P(tri), B, eta, sample_base, 0 if sample_range is None else sample_range, seed, step, row_offset,
                                                 b_global, side_mode, P(thr), P(pl), 0 if pool is None else len(pool), *(P(t) for t in f), max_tries,
                                                 P(stats), P(out), *(P(t) for t in c), None))
    torch.cuda.synchronize()
    return (out.cpu().numpy(), *(int(v) for v in stats.tolist()))


def check_against_ref(X, eta, **kw):
    got = gpu_typed(X, eta, **kw)
    want = TR.sample_negatives_typed(X, eta, SEED, STEP, **kw)
    assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]), np.flatnonzero((got[0] != want[0]).any(1))[:10]
    assert got[1:] == want[1:], (got[1:], want[1:])
    return got


# ------------------------------------------------------------------------------------------------------------------ 1. sets and lookup
def _engine(N, R):
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("TransE", 4, N, R)


def _assert_build(eng, X, N, R):
    Xd = dev(np.asarray(X, np.int32).reshape(-1, 3))
    for sd in "so":
        got = eng.relation_sets_build(Xd, sd, N, R)
        want = TR.build_sets(X, sd)
        for g, w in zip(got, want):                                        # keys, start, ids -- their lengths are the two counts
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g, w), sd


def test_relation_sets_build_equals_the_restatement(gpu_lib, planted):
    eng = _engine(planted.N, planted.R)
    _assert_build(eng, planted.typed_rows, planted.N, planted.R)
    _assert_build(eng, planted.train, planted.N, planted.R)
    _assert_build(eng, planted.train[:1], planted.N, planted.R)
    _assert_build(eng, np.zeros((0, 3), np.int32), planted.N, planted.R)   # m = 0: no key, start = [0], no id
    # the raw call with m = 0 touches start[0] and the counts only
    from ampligraph_amd import _ffi

    start, counts = torch.full((3,), 9, dtype=torch.int64, device="cuda"), torch.full((2,), 9, dtype=torch.int64, device="cuda")
    for side in (1, 2):
        _ffi.check(gpu_lib.amdkge_relation_sets_build(None, 0, side, planted.N, planted.R, None, P(start), None, P(counts), None, None))
        assert start.tolist() == [0, 9, 9] and counts.tolist() == [0, 0]


def test_relation_sets_at_a_wide_key(gpu_lib):
    """N = 70 000: n_rels * n_ents^2 needs 36 bits of sort key, ids beyond 2^16"""
    rng = np.random.default_rng(2)
    N, R, m = 70_000, 5, 5_000
    X = np.stack([rng.integers(0, N, m), rng.choice([0, 1, 2, 4], m), rng.integers(N - 3000, N, m)], 1).astype(np.int32)
    X[0], X[1] = (N - 1, 4, N - 1), (N - 1, 4, N - 1)
    eng = _engine(N, R)
    _assert_build(eng, X, N, R)
    keys, start, ids = TR.build_sets(X, "o")
    Q = np.stack([rng.integers(0, N, 300), rng.integers(0, R, 300), rng.integers(0, N, 300)], 1).astype(np.int32)
    for min_size, fb in ((0, (0, 0)), (700, (len(ids), len(ids) + N)), (10 ** 6, (3, 4))):
        lo, hi = eng.relation_sets_ranges(dev(keys), dev(start), dev(Q), min_size, fb)
        want = TR.ranges(keys, start, Q, min_size, fb)
        assert np.array_equal(lo.cpu().numpy(), want[0]) and np.array_equal(hi.cpu().numpy(), want[1])


def test_lookup_falls_back_for_absent_relations_and_small_sets(gpu_lib, planted):
    eng = _engine(planted.N, planted.R)
    Q = np.array([(0, r, 0) for r in range(planted.R)] * 3, np.int32)
    for sd in "so":
        keys, start, ids = planted.csr[sd]
        for min_size, fb in ((0, (0, 0)), (1, (0, 0)), (2, (0, 0)), (2, (len(ids), len(ids) + planted.N)), (5, (7, 9)), (100, (1, 1))):
            lo, hi = (t.cpu().numpy() for t in eng.relation_sets_ranges(dev(keys), dev(start), dev(Q), min_size, fb))
            want = TR.ranges(keys, start, Q, min_size, fb)
            assert lo.dtype == np.int64 and np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]), (sd, min_size)
            assert (lo[4], hi[4]) == fb                                    # relation 4: absent
            if min_size >= 2:
                assert (lo[1], hi[1]) == fb                                # relation 1: one id
            if min_size <= 3:
                assert (lo[3], hi[3]) != fb or fb == (0, 0) and hi[3] > lo[3]
    # an empty CSR: every triple falls back (NULL key pointers are fine with n_keys = 0)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    lo, hi = eng.relation_sets_ranges(none, torch.zeros(1, dtype=torch.int64, device="cuda"), dev(Q), 1, (2, 39))
    assert set(lo.tolist()) == {2} and set(hi.tolist()) == {39}


# ------------------------------------------------------------------------------------------------------------------ 2. the sampler
@pytest.mark.parametrize("mode", MODES, ids=[NR.SIDE_NAMES[m] for m in MODES])
@pytest.mark.parametrize("eta", [1, 3, 20])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_typed_kernel_equals_the_restatement(gpu_lib, planted, B, eta, mode):
    X = planted.batch(B)
    sc, oc = planted.cand(X)
    sf, of = planted.graph.filters(X)
    pl = np.array([36, 0, 12, 12, 5, 20, 33], np.int32)
    seen = np.zeros(3, np.int64)
    for flt in (False, True):
        for pool in (False, True):
            for mt in (1, 8):
                got = check_against_ref(X, eta, sample_range=planted.N, row_offset=5, b_global=B + 11, side_mode=mode, side_thr=planted.graph.thr,
                                        pool=pl if pool else None, s_filter=sf if flt else None, o_filter=of if flt else None, max_tries=mt,
                                        s_cand=sc, o_cand=oc)
                if not flt:
                    assert got[1:3] == (0, 0)
                if mt == 1:
                    assert got[1] == 0
                seen += got[1:]
    if B >= 63:
        assert seen[2] > 0                                                 # relations 1 and 4: the untyped rule
        if mode != NR.S_ONLY:
            assert seen[0] > 0 and seen[1] > 0                             # relation 0's object draws: rejected to the last try


def test_planted_counts_membership_and_min_size(gpu_lib, planted):
    """filter on, object side: EVERY corruption of a relation-0 positive exhausts (its range set is its known objects), none of the
    others' can be told in advance; every typed replacement is a member of its set; min_size moves relation 1 between the rules"""
    B, eta = 257, 3
    X = planted.batch(B)
    sf, of = planted.graph.filters(X)
    i = np.tile(np.arange(B), eta)
    for min_size in (1, 2):
        sc, oc = planted.cand(X, min_size)
        for mode, cand, col in ((NR.O_ONLY, oc, 2), (NR.S_ONLY, sc, 0)):
            out, rd, ex, ut = check_against_ref(X, eta, sample_range=planted.N, side_mode=mode, s_filter=sf, o_filter=of, max_tries=8, s_cand=sc, o_cand=oc)
            lo, hi, ids = cand
            typed = hi[i] > lo[i]
            assert ut == int((~typed).sum()) > 0 and typed.sum() > 0
            assert all(out[r, col] in ids[lo[q]:hi[q]] for r, q in enumerate(i) if typed[r])
            assert np.array_equal(out[:, 2 - col], X[i, 2 - col]) and np.array_equal(out[:, 1], X[i, 1])
            n0 = int((X[i, 1] == 0).sum())
            if mode == NR.O_ONLY:
                assert ex >= n0 > 0 and rd >= 7 * n0
                assert all(out[r, 2] in planted.R0 for r in np.flatnonzero(X[i, 1] == 0))
        n1 = int((X[i, 1] == 1).sum())
        assert n1 > 0 and (oc[1][X[:, 1] == 1] > oc[0][X[:, 1] == 1]).all() == (min_size == 1)
    # relation 3 has sets but no known statement: typed, never rejected
    X3 = X[X[:, 1] == 3]
    sc, oc = planted.cand(X3)
    out, rd, ex, ut = check_against_ref(X3, 5, sample_range=planted.N, s_filter=planted.graph.filters(X3)[0], o_filter=planted.graph.filters(X3)[1],
                                        s_cand=sc, o_cand=oc)
    assert (rd, ex, ut) == (0, 0, 0) and set(out[:, 0].tolist()) <= set(planted.D3) | set(X3[:, 0].tolist())
    assert set(out[:, 0].tolist()) <= set(planted.D3) and set(out[:, 2].tolist()) <= set(planted.R3)


def test_launch_split_and_two_cuts_of_one_batch(gpu_lib, planted):
    X = planted.batch(3)
    sc, oc = planted.cand(X)
    sf, of = planted.graph.filters(X)
    check_against_ref(X, 1500, sample_range=planted.N, side_mode=NR.BERNOULLI, side_thr=planted.graph.thr, s_filter=sf, o_filter=of, max_tries=5,
                      s_cand=sc, o_cand=oc)                                # a thread walks several j: the grid's second dimension is capped
    B, eta = 257, 5
    X = planted.batch(B)
    sc, oc = planted.cand(X)
    sf, of = planted.graph.filters(X)
    kw = dict(sample_range=planted.N, side_mode=NR.UNIFORM, max_tries=8)
    whole = gpu_typed(X, eta, s_filter=sf, o_filter=of, s_cand=sc, o_cand=oc, **kw)
    for cut in (131, 64):
        parts, sums = [], np.zeros(3, np.int64)
        for a, b in ((0, cut), (cut, B)):
            part = lambda f: (f[0][a:b], f[1][a:b], f[2])   # noqa: E731
            got = gpu_typed(X[a:b], eta, row_offset=a, b_global=B, s_filter=part(sf), o_filter=part(of), s_cand=part(sc), o_cand=part(oc), **kw)
            parts.append(got[0].reshape(eta, b - a, 3))
            sums += got[1:]
        assert np.array_equal(np.concatenate(parts, 1).reshape(-1, 3), whole[0]) and tuple(sums) == whole[1:]
    assert whole[1] > 0 and whole[2] > 0 and whole[3] > 0


@pytest.mark.parametrize("mode", MODES, ids=[NR.SIDE_NAMES[m] for m in MODES])
def test_the_two_identities_with_sample_negatives(gpu_lib, planted, mode):
    B, eta = 257, 3
    X = planted.batch(B)
    sf, of = planted.graph.filters(X)
    pl = np.array([36, 0, 12, 12, 5], np.int32)
    base = dict(row_offset=9, b_global=B + 3, side_mode=mode, side_thr=planted.graph.thr, s_filter=sf, o_filter=of, max_tries=8)
    # a. six NULL candidate arrays: amdkge_sample_negatives, pool and window included
    for kw in (dict(sample_range=planted.N), dict(sample_base=3, sample_range=20), dict(pool=pl, sample_range=planted.N)):
        want, rd, ex = gpu_sample(X, eta, **base, **kw)
        got = gpu_typed(X, eta, **base, **kw)
        assert np.array_equal(got[0], want) and got[1:] == (rd, ex, B * eta)
    # b. every range the ascending ids 0 .. N-1 (behind a prefix, so lo != 0): the untyped draw with sample_base 0, sample_range N
    want, rd, ex = gpu_sample(X, eta, sample_base=0, sample_range=planted.N, **base)
    everyone = np.arange(planted.N, dtype=np.int32)
    full = (np.zeros(B, np.int64), np.full(B, planted.N, np.int64), everyone)
    shifted = (np.full(B, 4, np.int64), np.full(B, 4 + planted.N, np.int64), np.concatenate([[7, 7, 7, 7], everyone]).astype(np.int32))
    for kw in (dict(sample_range=planted.N), dict(sample_base=3, sample_range=2), dict(pool=pl, sample_range=1)):
        got = gpu_typed(X, eta, s_cand=full, o_cand=shifted, **base, **kw)
        assert np.array_equal(got[0], want) and got[1:] == (rd, ex, 0)
    assert rd > 0


# ------------------------------------------------------------------------------------------------------------------ 3. fit()
def _labels(ids):
    ids = np.asarray(ids)
    return np.stack([np.char.add("e", ids[:, 0].astype(str)), np.char.add("r", ids[:, 1].astype(str)), np.char.add("e", ids[:, 2].astype(str))], 1)


class _RestatedTyped:
    """What compile(negatives={"types": "observed", "filter": True, "side": "bernoulli"}) binds, with the numpy restatements in place
    of the kernels: bind() -> a StepLoop.negatives that uploads types_ref's rows."""

    def __init__(self, min_size=2, max_tries=8):
        self.min_size, self.max_tries, self.counts, self.calls = min_size, max_tries, np.zeros(3, np.int64), 0

    def bind(self, model, engine, train):
        self.X = train.cpu().numpy()
        self.g = Graph(self.X, model._n_ents, model._n_rels)
        self.filters = self.g.filters(self.X)
        self.csr = {sd: TR.build_sets(self.X, sd) for sd in "so"}
        self.cand = [(*TR.ranges(self.csr[sd][0], self.csr[sd][1], self.X, self.min_size, (0, 0)), self.csr[sd][2]) for sd in "so"]
        return self

    def __call__(self, global_batch, lo, hi, eta, seed, step):
        r0 = global_batch.storage_offset() // 3 + lo
        r1 = r0 + hi - lo
        sf, of, sc, oc = ((f[0][r0:r1], f[1][r0:r1], f[2]) for f in (*self.filters, *self.cand))
        rows, *counts = TR.sample_negatives_typed(self.X[r0:r1], eta, seed, step, sample_range=self.g.N, row_offset=lo, b_global=int(global_batch.shape[0]),
                                                  side_mode=NR.BERNOULLI, side_thr=self.g.thr, s_filter=sf, o_filter=of, max_tries=self.max_tries,
                                                  s_cand=sc, o_cand=oc)
        self.counts, self.calls = self.counts + counts, self.calls + 1
        self.last = dev(rows)
        return self.last


@pytest.fixture(scope="module")
def fitted(gpu_lib, planted):
    """model name -> (a model fitted with TypedNegatives, the same fit on the restated rows, the training labels)"""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = _labels(planted.train)
    kw = dict(optimizer="adam", loss="nll", deterministic=True)
    out = {}
    for name in ("ComplEx", "TransE"):
        m1 = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=name, seed=2)
        m1.compile(negatives={"types": "observed", "filter": True, "side": "bernoulli"}, **kw)
        m1.fit(X, batch_size=24, epochs=3, verbose=False)                  # 63 rows: 3 batches per epoch, the last one short
        m2 = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=name, seed=2)
        m2.compile(**kw)
        m2._negatives = stub = _RestatedTyped()
        m2.fit(X, batch_size=24, epochs=3, verbose=False)
        out[name] = (m1, m2, stub, X)
    return out


@pytest.mark.parametrize("model", ["ComplEx", "TransE"])
def test_fit_with_typed_negatives_equals_fit_on_the_restated_rows(fitted, planted, model):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    m1, m2, stub, X = fitted[model]
    assert len(X) == 63 and stub.calls == 9 and m2._loop.negatives is stub
    (e1, r1), (e2, r2) = m1._engine.get_tables(), m2._engine.get_tables()
    assert np.array_equal(e1.view(np.int32), e2.view(np.int32)) and np.array_equal(r1.view(np.int32), r2.view(np.int32))
    st = m1.negative_sampling_stats_
    assert st == dict(zip(("redraws", "exhausted", "untyped"), (int(v) for v in stub.counts))) and all(type(v) is int for v in st.values())
    assert st["redraws"] > 0 and st["exhausted"] > 0 and st["untyped"] > 0
    # the bound sets are the training set's, in the model's id map
    host = m1.relation_types_.host_sets()
    for sd in "so":
        keys, start, ids = stub.csr[sd]
        assert sorted(host[sd]) == keys.tolist() and all(np.array_equal(host[sd][int(r)], ids[start[g]:start[g + 1]]) for g, r in enumerate(keys))
    assert m1.relation_types_.largest_set == {sd: int(np.diff(stub.csr[sd][1]).max()) for sd in "so"}
    assert not hasattr(m2, "relation_types_")
    # the sampler did something: untyped filtered negatives give other tables
    m3 = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=model, seed=2)
    m3.compile(optimizer="adam", loss="nll", deterministic=True, negatives={"filter": True, "side": "bernoulli"})
    m3.fit(X, batch_size=24, epochs=3, verbose=False)
    assert not np.array_equal(e1, m3._engine.get_tables()[0]) and set(m3.negative_sampling_stats_) == {"redraws", "exhausted"}


def test_explicit_types_through_fit_and_unknown_labels(gpu_lib, planted):
    from ampligraph_amd.datasets.types import RelationTypes
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = _labels(planted.train)
    rt = RelationTypes({"r0": (["e%d" % v for v in planted.D0], ["e%d" % v for v in planted.R0 + planted.R0[:2]]), "r2": (None, ["e1", "e2", "e3"]),
                        "r4": (None, None)})
    m = ScoringBasedEmbeddingModel(eta=4, k=8, scoring_type="DistMult", seed=1)
    m.compile(optimizer="adam", loss="nll", negatives={"types": rt, "side": "o", "min_size": 1})
    m.fit(X, batch_size=63, epochs=1, verbose=False)
    ix = m.data_indexer
    host = m.relation_types_.host_sets()
    rid = lambda r: int(ix.get_indexes(np.array([r]), "r")[0])   # noqa: E731
    eid = lambda es: sorted(int(v) for v in ix.get_indexes(np.array(["e%d" % e for e in es]), "e"))   # noqa: E731
    assert sorted(host["s"]) == [rid("r0")] and sorted(host["o"]) == sorted([rid("r0"), rid("r2")])
    assert host["o"][rid("r0")].tolist() == eid(planted.R0) and host["o"][rid("r2")].tolist() == eid([1, 2, 3]) and host["s"][rid("r0")].tolist() == eid(planted.D0)
    bound = m._loop.negatives
    rows = bound(bound.train, 0, 63, 4, m.seed, 0).cpu().numpy()
    Xi = bound.train.cpu().numpy()
    i = np.tile(np.arange(63), 4)
    assert np.array_equal(rows[:, :2], Xi[i, :2])
    for r, ok in ((rid("r0"), eid(planted.R0)), (rid("r2"), eid([1, 2, 3]))):
        assert set(rows[Xi[i, 1] == r, 2].tolist()) <= set(ok)
    n_free = int(np.isin(Xi[:, 1], [rid("r1"), rid("r4")]).sum())
    assert m.negative_sampling_stats_ == {"redraws": 0, "exhausted": 0, "untyped": 4 * n_free}
    for bad, what in (({"r9": (None, None)}, "relation"), ({"r0": (["e0", "nobody"], None)}, "domain"), ({"r0": (None, ["nobody"])}, "range")):
        m.compile(optimizer="adam", loss="nll", negatives={"types": RelationTypes(bad)})
        with pytest.raises(ValueError, match=what):
            m.fit(X, batch_size=63, epochs=1, verbose=False)


# ------------------------------------------------------------------------------------------------------------------ 4. evaluate_typed
def _materialised(model, bound, x, min_size):
    """the label lists evaluate_candidates takes: the set of each row's relation per side, every entity where evaluate_typed falls back"""
    ix = model.data_indexer
    Xi = ix.get_indexes(x)
    host = bound.host_sets()
    everyone = ix.get_indexes(np.arange(model._n_ents), "e", "ind2raw")
    lists = {"s": [], "o": []}
    for row in Xi:
        for sd in "so":
            ids = host[sd].get(int(row[1]))
            lists[sd].append(everyone if ids is None or len(ids) < min_size else ix.get_indexes(ids, "e", "ind2raw"))
    return lists["s"], lists["o"]


@pytest.fixture(scope="module")
def eval_cases(fitted, planted):
    """test triples: training rows of every relation and unseen combinations of known labels; two kinds of types"""
    from ampligraph_amd.datasets.types import RelationTypes

    rng = np.random.default_rng(5)
    extra = np.stack([rng.integers(0, planted.N, 25), rng.choice([0, 1, 2, 4], 25), rng.integers(0, planted.N, 25)], 1)
    known = set(np.unique(planted.train[:, [0, 2]]).tolist())
    extra = np.array([t for t in extra.tolist() if t[0] in known and t[2] in known], np.int32)
    x = _labels(np.concatenate([planted.train[::2], extra]))
    explicit = RelationTypes({"r0": (["e%d" % v for v in planted.D0 + [20]], ["e%d" % v for v in planted.R0]), "r1": (["e5"], None),
                              "r2": (None, ["e%d" % v for v in sorted(known)[:9]])})
    observed = RelationTypes.observed({"train": _labels(planted.train), "more": _labels(extra)})
    return x, _labels(extra), {"explicit": explicit, "observed": observed}


@pytest.mark.parametrize("kind", ["explicit", "observed"])
@pytest.mark.parametrize("model", ["ComplEx", "TransE"])
def test_evaluate_typed_equals_evaluate_candidates_on_the_materialised_sets(fitted, eval_cases, model, kind):
    m = fitted[model][0]
    x, extra, types = eval_cases
    bound = types[kind].bind(m, m._engine)
    filters = (False, True, {"train": fitted[model][3], "more": extra})
    for min_size in (1, 2):
        cs, co = _materialised(m, bound, x, min_size)
        assert min(len(c) for c in cs + co) >= min_size and any(len(c) < m._n_ents for c in cs)
        assert kind == "observed" or any(len(c) == m._n_ents for c in cs)   # (explicit: relation 2 has no domain, relation 4 nothing)
        for use_filter in filters:
            for strategy in ("worst", "best", "middle"):
                want = m.evaluate_candidates(x, candidates_s=cs, candidates_o=co, use_filter=use_filter, ranking_strategy=strategy)
                got = m.evaluate_typed(x, types=bound, use_filter=use_filter, ranking_strategy=strategy, min_size=min_size)
                assert got.dtype == np.int32 and got.shape == (len(x), 2) and np.array_equal(got, want), (min_size, use_filter is not False, strategy)
                for side, col in (("s", 0), ("o", 1)):
                    one = m.evaluate_typed(x, types=types[kind], use_filter=use_filter, corrupt_side=side, ranking_strategy=strategy, min_size=min_size)
                    assert one.shape == (len(x), 1) and np.array_equal(one[:, 0], want[:, col])
        both = m.evaluate_typed(x, types=bound, use_filter=True, corrupt_side="s+o", min_size=min_size)
        assert both.shape == (len(x), 1) and np.array_equal(both[:, 0], want_sum(m, x, cs, co))
    assert (got >= 1).all() and got.max() > 1


def want_sum(m, x, cs, co):
    r = m.evaluate_candidates(x, candidates_s=cs, candidates_o=co, use_filter=True, ranking_strategy="worst")
    return r.sum(1) - 1


@pytest.mark.parametrize("model", ["ComplEx", "TransE"])
def test_evaluate_typed_defaults_and_the_unconstrained_case(fitted, eval_cases, model):
    from ampligraph_amd.datasets.types import RelationTypes
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.placement import Rows

    m, m2 = fitted[model][:2]
    x, extra, types = eval_cases
    # types=None: the sets fit() bound (the training set's)
    cs, co = _materialised(m, m.relation_types_, x, 1)
    assert np.array_equal(m.evaluate_typed(x, use_filter=True), m.evaluate_candidates(x, candidates_s=cs, candidates_o=co, use_filter=True))
    # every relation unconstrained -- no set at all, or every set below min_size: evaluate()
    for side in ("s", "o", "s,o", "s+o"):
        for use_filter in (False, True):
            want = m.evaluate(x, use_filter=use_filter, corrupt_side=side, ranking_strategy="middle", verbose=False)
            for t, ms in ((RelationTypes({}), 1), (RelationTypes({"r0": (None, None)}), 1), (None, 10 ** 6)):
                got = m.evaluate_typed(x, types=t, use_filter=use_filter, corrupt_side=side, ranking_strategy="middle", min_size=ms)
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (side, use_filter, ms)
    assert m.evaluate_typed(x[:0], types=RelationTypes({})).shape == (0, 2)
    # refusals
    with pytest.raises(ValueError, match="relation_types_"):
        m2.evaluate_typed(x)                                               # fitted without TypedNegatives, no types given
    with pytest.raises(ValueError, match="observed"):
        m.evaluate_typed(x, types=RelationTypes.observed())
    with pytest.raises(ValueError, match="another model"):
        other = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="TransE", seed=0)
        other.compile(optimizer="adam", loss="nll", negatives={"types": "observed"})
        other.fit(x[:10], batch_size=10, epochs=1, verbose=False)
        m.evaluate_typed(x, types=other.relation_types_)
    keep = m._placement
    try:
        m._placement = Rows.__new__(Rows)
        with pytest.raises(NotImplementedError, match="sharded"):
            m.evaluate_typed(x)
    finally:
        m._placement = keep
