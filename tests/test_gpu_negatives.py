"""The training negative samplers on the GPU (kge_negatives.hip, include/amdkge_negatives.h): amdkge_sample_negatives against the
numpy restatement of the draw (tests/negatives_ref.py) bit for bit, the trivial configuration against amdkge_sample_corruptions,
the accounting identity on a dense planted graph, the Bernoulli thresholds, compile(negatives=...) end to end, guard bands."""
import ctypes as C

import numpy as np
import pytest
import torch

import negatives_ref as NR
from abi_decl import declared_names

pytestmark = pytest.mark.gpu

SEED, STEP = 12345678901234, (1 << 33) + 5


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def gpu_sample(X, eta, seed=SEED, step=STEP, sample_base=0, sample_range=None, row_offset=0, b_global=0, side_mode=NR.UNIFORM, side_thr=None,
               pool=None, s_filter=None, o_filter=None, max_tries=8):
    """amdkge_sample_negatives with negatives_ref.sample_negatives' arguments -> (rows, redraws, exhausted)"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    B = len(X)
    tri = dev(np.asarray(X, dtype=np.int32))
    out = torch.full((B * eta, 3), -7, dtype=torch.int32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    thr = None if side_thr is None else dev(np.asarray(side_thr, dtype=np.uint32).view(np.int32))
    pl = None if pool is None else dev(np.asarray(pool, dtype=np.int32))
    f = [None] * 6
    if s_filter is not None:
        f = [dev(np.asarray(a, dtype=dt)) for flt in (s_filter, o_filter) for a, dt in zip(flt, (np.int64, np.int64, np.int32))]
    _ffi.check(lib.amdkge_sample_negatives(P(tri), B, eta, sample_base, 0 if sample_range is None else sample_range, seed, step, row_offset, b_global,
                                           side_mode, P(thr), P(pl), 0 if pool is None else len(pool), *(P(t) for t in f), max_tries, P(stats),
                                           P(out), None))
    torch.cuda.synchronize()
    rd, ex = stats.tolist()
    return out.cpu().numpy(), int(rd), int(ex)


def check_against_ref(X, eta, **kw):
    got, rd, ex = gpu_sample(X, eta, **kw)
    want, rd_ref, ex_ref = NR.sample_negatives(X, eta, SEED, STEP, **kw)
    assert got.dtype == want.dtype and np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:10]
    assert (rd, ex) == (rd_ref, ex_ref)
    return got, rd, ex


# ------------------------------------------------------------------------------------------------------------------ the graphs
class Graph:
    """an id graph, its host-built FilterIndex, the thresholds by the integer formula"""

    def __init__(self, G, N, R):
        from ampligraph_amd.datasets.filters import FilterIndex

        self.G, self.N, self.R = np.asarray(G, dtype=np.int32), N, R
        self.fi = FilterIndex([self.G], N, R)
        self.thr = NR.side_thresholds(self.fi.po_keys, self.fi.sp_keys, N, R)
        self.known = {tuple(int(v) for v in t) for t in self.G}

    def filters(self, X):
        return (*self.fi.subject_ranges(X), self.fi.s_ids), (*self.fi.object_ranges(X), self.fi.o_ids)


@pytest.fixture(scope="module")
def hub():
    """N = 4000, R = 4: object 0 is a HUB of relation 0 (3500 subjects: a range of 3500 ids for every positive (s, 0, 0)), 600
    random triples (ranges of length 1 - 2), and relation 3 absent.  batch(B): hub rows, indexed rows and rows whose keys the index
    does not hold (empty ranges on both sides), in an order that changes from lane to lane."""
    rng = np.random.default_rng(3)
    N, R = 4000, 4
    hubs = np.stack([np.arange(3500), np.zeros(3500, int), np.zeros(3500, int)], 1)
    rand = np.stack([rng.integers(0, N, 600), rng.integers(0, 3, 600), rng.integers(1, N, 600)], 1)
    g = Graph(np.concatenate([hubs, rand]), N, R)
    absent = np.stack([rng.integers(0, N, 400), np.full(400, 3), rng.integers(0, N, 400)], 1)
    pick = np.concatenate([hubs[rng.permutation(3500)[:400]], rand[:400], absent]).astype(np.int32)
    order = rng.permutation(len(pick))
    order = np.concatenate([[0], order[order != 0]])           # (B = 1 is a hub row)
    g.batch = lambda B: np.ascontiguousarray(pick[order][:B])
    lens = np.diff(g.fi.po_start)
    assert lens.max() >= 3000 and (lens == 1).any() and g.thr[3] == 0x80000000
    return g


@pytest.fixture(scope="module")
def tiny():
    """N = 4: (0, 0, o) is known for o = 0, 1, 2 -- an object corruption of those positives has ONE acceptable entity, so tries run
    past the three words of block 0 (and exhaust with probability (3/4)^8 = 10 %)"""
    G = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 0, 3), (2, 1, 3), (3, 1, 0), (1, 1, 1)]
    return Graph(G, 4, 2)


SHAPES = [(1, 1), (37, 3), (300, 5)]
MODES = [NR.UNIFORM, NR.BERNOULLI, NR.S_ONLY, NR.O_ONLY]


# ------------------------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", [False, True], ids=["unfiltered", "filtered"])
@pytest.mark.parametrize("pool", [False, True], ids=["all", "pool"])
@pytest.mark.parametrize("mode", MODES, ids=[NR.SIDE_NAMES[m] for m in MODES])
def test_kernel_equals_the_restatement(gpu_lib, hub, mode, pool, flt, shape):
    B, eta = shape
    X = hub.batch(B)
    sf, of = hub.filters(X) if flt else (None, None)
    # the pool: 40 entities, most of them hub subjects, one listed twice
    pl = np.concatenate([np.arange(0, 3500, 100), [3999, 3700, 0, 17, 17]]).astype(np.int32) if pool else None
    _, rd, ex = check_against_ref(X, eta, sample_range=hub.N, row_offset=5, b_global=B + 11, side_mode=mode, side_thr=hub.thr, pool=pl,
                                  s_filter=sf, o_filter=of, max_tries=8)
    if not flt:
        assert (rd, ex) == (0, 0)
    elif B >= 37 and mode in (NR.UNIFORM, NR.S_ONLY):
        assert rd > 0 and ex > 0   # (7/8 of the entities are known subjects of the hub: 0.875^8 = 34 % of its corruptions exhaust)


@pytest.mark.parametrize("mode", MODES, ids=[NR.SIDE_NAMES[m] for m in MODES])
def test_tries_cross_the_block_boundary_on_four_entities(gpu_lib, tiny, mode):
    rng = np.random.default_rng(0)
    X = tiny.G[rng.integers(0, len(tiny.G), 300)]
    sf, of = tiny.filters(X)
    for mt in (1, 3, 4, 8, 32):
        _, rd, ex = check_against_ref(X, 5, sample_range=4, side_mode=mode, side_thr=tiny.thr, s_filter=sf, o_filter=of, max_tries=mt)
        assert rd <= (mt - 1) * 1500 and (rd > 0) == (mt > 1)


def test_corners_pool_of_one_and_range_of_one(gpu_lib, tiny, hub):
    X = np.ascontiguousarray(np.repeat(tiny.G, 6, axis=0))
    sf, of = tiny.filters(X)
    # every replacement is entity 3 / entity 0: where that is a known one, all tries are rejected and the last one is kept
    for kw in (dict(pool=np.array([3], np.int32), sample_range=4), dict(sample_base=0, sample_range=1), dict(sample_base=3, sample_range=1)):
        for mt in (1, 8):
            got, rd, ex = check_against_ref(X, 3, side_mode=NR.UNIFORM, s_filter=sf, o_filter=of, max_tries=mt, **kw)
            e = 3 if "pool" in kw else kw["sample_base"]
            i = np.tile(np.arange(len(X)), 3)
            assert np.all((got[:, 0] == e) | (got[:, 2] == e))
            assert ex == int(NR.known_rows(got, tiny.known).sum()) > 0 and rd == ex * (mt - 1)
            assert np.array_equal(got[:, 1], X[i, 1])
    # a sampling window of the hub's subjects alone
    Xh = hub.batch(37)
    sf, of = hub.filters(Xh)
    check_against_ref(Xh, 3, sample_base=100, sample_range=50, side_mode=NR.S_ONLY, s_filter=sf, o_filter=of, max_tries=2)


def test_launch_split_and_two_halves(gpu_lib, hub):
    """Few positives with many corruptions: a thread then walks several j (the grid's second dimension is capped); and two half-batch
    launches give the rows of the whole one, with the counters adding up."""
    X = hub.batch(3)
    sf, of = hub.filters(X)
    check_against_ref(X, 1500, sample_range=hub.N, side_mode=NR.BERNOULLI, side_thr=hub.thr, s_filter=sf, o_filter=of, max_tries=5)
    B, eta, cut = 300, 5, 131
    X = hub.batch(B)
    sf, of = hub.filters(X)
    kw = dict(sample_range=hub.N, side_mode=NR.UNIFORM, max_tries=8)
    whole, rd, ex = gpu_sample(X, eta, s_filter=sf, o_filter=of, **kw)
    parts, rds, exs = [], 0, 0
    for a, b in ((0, cut), (cut, B)):
        out, r, e = gpu_sample(X[a:b], eta, row_offset=a, b_global=B, s_filter=tuple(f[a:b] if q < 2 else f for q, f in enumerate(sf)),
                               o_filter=tuple(f[a:b] if q < 2 else f for q, f in enumerate(of)), **kw)
        parts.append(out.reshape(eta, b - a, 3))
        rds, exs = rds + r, exs + e
    assert np.array_equal(np.concatenate(parts, 1).reshape(-1, 3), whole) and (rds, exs) == (rd, ex) and rd > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_trivial_configuration_is_sample_corruptions(gpu_lib, hub, shape):
    from ampligraph_amd import _ffi

    B, eta = shape
    X = hub.batch(B)
    tri = dev(X)
    want = torch.full((B * eta, 3), -7, dtype=torch.int32, device="cuda")
    _ffi.check(gpu_lib.amdkge_sample_corruptions(P(tri), B, eta, 7, hub.N - 9, SEED, STEP, 17, B + 40, P(want), None))
    for mt in (1, 8):
        got, rd, ex = gpu_sample(X, eta, sample_base=7, sample_range=hub.N - 9, row_offset=17, b_global=B + 40, max_tries=mt)
        assert np.array_equal(got, want.cpu().numpy()) and (rd, ex) == (0, 0)


# ------------------------------------------------------------------------------------------------------------------ 2. accounting
def _planted(seed):
    rng = np.random.default_rng(seed)
    s, o = np.nonzero(rng.random((32, 32)) < 0.6)
    return Graph(np.stack([s, np.zeros_like(s), o], 1), 32, 1)


def test_accounting_identity_on_a_dense_planted_graph(gpu_lib):
    """1 relation, 32 entities, ~60 % of the pairs true; every true pair is a positive, eta = 16: ~10^4 corruptions."""
    eta = 16
    g = _planted(0)
    X = g.G
    assert 9000 <= len(X) * eta <= 11000
    sf, of = g.filters(X)
    kw = dict(sample_range=32, s_filter=sf, o_filter=of)
    # max_tries = 8: the known rows of the output are exactly the exhausted corruptions, and the redraws are the restatement's
    got, rd, ex = check_against_ref(X, eta, max_tries=8, **kw)
    assert int(NR.known_rows(got, g.known).sum()) == ex > 0 and rd > len(got) // 2
    # max_tries = 32, on the first seed for which THE RESTATEMENT ALONE (CPU) exhausts no corruption: a condition on the input, not a
    # tolerance -- then the kernel's output holds no known statement at all
    for seed in range(10):
        g = _planted(seed)
        sf, of = g.filters(g.G)
        kw = dict(sample_range=32, s_filter=sf, o_filter=of, max_tries=32)
        if NR.sample_negatives(g.G, eta, SEED, STEP, **kw)[2] == 0:
            break
    else:
        pytest.fail("no planted graph without an exhausted corruption in ten seeds")
    got, rd, ex = gpu_sample(g.G, eta, **kw)
    assert ex == 0 and int(NR.known_rows(got, g.known).sum()) == 0 and rd > 0
    # unfiltered, the same graph is corrupted into known statements: what the feature is for
    got, rd, ex = gpu_sample(g.G, eta, sample_range=32, max_tries=32)
    assert (rd, ex) == (0, 0) and int(NR.known_rows(got, g.known).sum()) > len(got) // 3


# ------------------------------------------------------------------------------------------------------------------ 3. thresholds
def test_side_thresholds_equal_the_integer_formula(gpu_lib):
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.engine import KgeEngine

    rng = np.random.default_rng(5)
    N, R, n = 300, 5, 2000
    rel = rng.choice([0, 1, 2, 4], n, p=[0.4, 0.3, 0.2, 0.1])                 # relation 3 is absent
    s = np.where(rel == 0, rng.integers(0, 5, n), rng.integers(0, N, n))      # relation 0: few heads, many tails
    o = np.where(rel == 1, rng.integers(0, 3, n), rng.integers(0, N, n))      # relation 1: few tails
    X = np.stack([s, rel, o], 1).astype(np.int32)
    eng = KgeEngine("TransE", 4, N, R)
    fi_dev, fi_host = FilterIndex([X], N, R, engine=eng), FilterIndex([X], N, R)
    got = eng.negatives_side_thresholds(*fi_dev.device_keys(eng), N, R).cpu().numpy().view(np.uint32)
    want = NR.side_thresholds(fi_host.po_keys, fi_host.sp_keys, N, R)
    assert np.array_equal(got, want), (got, want)
    assert want[3] == 0x80000000 and want[0] > 0xC0000000 and want[1] < 0x40000000
    # an empty index: every relation gets the fair coin
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert eng.negatives_side_thresholds(empty, empty, N, R).cpu().numpy().view(np.uint32).tolist() == [0x80000000] * R


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
class _RestatedSampling:
    """What compile(negatives={"filter": True, "side": "bernoulli"}) binds, with the numpy restatement in place of the kernel:
    bind() -> a StepLoop.negatives that uploads negatives_ref's rows."""

    def __init__(self, max_tries=8):
        self.max_tries, self.redraws, self.exhausted, self.calls = max_tries, 0, 0, 0

    def bind(self, model, engine, train):
        self.X = train.cpu().numpy()
        self.g = Graph(self.X, model._n_ents, model._n_rels)
        self.filters = self.g.filters(self.X)
        return self

    def __call__(self, global_batch, lo, hi, eta, seed, step):
        r0 = global_batch.storage_offset() // 3 + lo
        r1 = r0 + hi - lo
        assert np.array_equal(global_batch[lo:hi].cpu().numpy(), self.X[r0:r1])
        sf, of = ((f[0][r0:r1], f[1][r0:r1], f[2]) for f in self.filters)
        rows, rd, ex = NR.sample_negatives(self.X[r0:r1], eta, seed, step, sample_range=self.g.N, row_offset=lo, b_global=int(global_batch.shape[0]),
                                           side_mode=NR.BERNOULLI, side_thr=self.g.thr, s_filter=sf, o_filter=of, max_tries=self.max_tries)
        self.redraws, self.exhausted, self.calls = self.redraws + rd, self.exhausted + ex, self.calls + 1
        self.last = dev(rows)
        return self.last


@pytest.mark.parametrize("model", ["ComplEx", "TransE"])
def test_fit_with_the_sampler_equals_fit_on_the_restated_rows(gpu_lib, model, tmp_path):
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import NegativeSampling
    from ampligraph_amd.utils.model_utils import restore_model, save_model

    X = toy_graph(seed=4, n=200, N=25, R=3)   # dense enough for redraws: 200 triples on 25 entities
    kw = dict(optimizer="adam", loss="nll", deterministic=True)

    def fit(m):
        m.fit(X, batch_size=64, epochs=3, verbose=False)   # 4 batches per epoch, the last one short
        return m._engine.get_tables()

    m1 = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=model, seed=2)
    m1.compile(negatives={"filter": True, "side": "bernoulli"}, **kw)
    e1, r1 = fit(m1)
    m2 = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=model, seed=2)
    m2.compile(**kw)
    m2._negatives = stub = _RestatedSampling()
    e2, r2 = fit(m2)
    assert stub.calls == 12 and m2._loop.negatives is stub
    assert np.array_equal(e1.view(np.int32), e2.view(np.int32)) and np.array_equal(r1.view(np.int32), r2.view(np.int32))
    # the sampler did something: the default draw gives other tables
    m3 = ScoringBasedEmbeddingModel(eta=3, k=8, scoring_type=model, seed=2)
    m3.compile(**kw)
    e3, _ = fit(m3)
    assert not np.array_equal(e1, e3) and not hasattr(m3, "negative_sampling_stats_")
    # stats: read back once at the end of fit()
    assert m1.negative_sampling_stats_ == {"redraws": stub.redraws, "exhausted": stub.exhausted}
    assert all(type(v) is int for v in m1.negative_sampling_stats_.values()) and stub.redraws > 0
    # save / restore carries compile()'s engine keywords as far as it carries `deterministic`
    save_model(m1, str(tmp_path / "m"))
    back = restore_model(str(tmp_path / "m"))
    if back._deterministic:
        assert isinstance(back._negatives, NegativeSampling) and (back._negatives.filter, back._negatives.side) == (True, "bernoulli")
    else:
        assert back._negatives is None   # (neither keyword is part of the saved format: compile() again to train on)
    assert np.array_equal(back.predict(X[:20]), m1.predict(X[:20]))


def test_fit_with_a_pool_and_extra_filter_datasets(gpu_lib):
    """The rest of NegativeSampling through fit(): replacements come from the pool alone, the filter datasets count as known, and
    labels outside the training set are refused."""
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    X = toy_graph(seed=6, n=300, N=25, R=3)
    train, extra = X[:200], X[200:]
    ents = np.unique(np.concatenate([train[:, 0], train[:, 2]]))
    pool = ents[:6]
    m = ScoringBasedEmbeddingModel(eta=4, k=8, scoring_type="DistMult", seed=1)
    m.compile(optimizer="adam", loss="nll", negatives={"filter": {"more": extra}, "side": "o", "entities": pool, "max_tries": 4})
    m.fit(train, batch_size=100, epochs=1, verbose=False)
    st = m.negative_sampling_stats_
    assert st["redraws"] > 0 and st["exhausted"] >= 0
    bound = m._loop.negatives
    rows = bound(bound.train[:100], 0, 100, 4, m.seed, 0).cpu().numpy()
    Xi = bound.train[:100].cpu().numpy()
    i = np.tile(np.arange(100), 4)
    pool_ids = set(m.data_indexer.get_indexes(pool, "e").tolist())
    assert np.array_equal(rows[:, :2], Xi[i, :2]) and set(rows[:, 2].tolist()) <= pool_ids
    known = {tuple(t) for t in m.data_indexer.get_indexes(X).tolist()}
    n_known = int(NR.known_rows(rows, known).sum())
    m.compile(optimizer="adam", loss="nll", negatives={"side": "o", "entities": pool})
    m.fit(train, batch_size=100, epochs=1, verbose=False)
    assert m.negative_sampling_stats_ == {"redraws": 0, "exhausted": 0}
    plain = m._loop.negatives(m._loop.negatives.train[:100], 0, 100, 4, m.seed, 0).cpu().numpy()
    assert n_known < int(NR.known_rows(plain, known).sum())
    m.compile(optimizer="adam", loss="nll", negatives={"entities": ["no such entity"]})
    with pytest.raises(ValueError, match="not in the training set"):
        m.fit(train, batch_size=100, epochs=1, verbose=False)


# ------------------------------------------------------------------------------------------------------------------ 5. guard bands
def case_sample_negatives(ar, B, eta, mode, pool, flt):
    """every device argument between bands; the ranges end with the last id of their arrays, the pool holds the last entity"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    rng = np.random.default_rng(7)
    N, R = 130, 5
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
    X[0], X[-1, 2] = (N - 1, R - 1, 0), N - 1
    tri = ar.put("triples", X)
    thr = ar.put("thr", rng.integers(-2 ** 31, 2 ** 31, R).astype(np.int32)) if mode == NR.BERNOULLI else None
    pl = ar.put("pool", np.array([N - 1, 0, 5, 5, 77], np.int32)) if pool else None
    f = [None] * 6
    if flt:
        f = []
        for side in "so":
            cnt = rng.integers(0, 90, B)
            cnt[-1] = 120
            start = np.zeros(B + 1, np.int64)
            start[1:] = np.cumsum(cnt)
            ids = np.concatenate([np.sort(rng.permutation(N)[:c]) for c in cnt]).astype(np.int32)
            f += [ar.put(side + "_lo", start[:-1].copy()), ar.put(side + "_hi", start[1:].copy()), ar.put(side + "_ids", ids)]
    stats = ar.out("stats", (2,), np.int64, 3)
    out = ar.out("negs", (B * eta, 3), np.int32, 1)
    _ffi.check(lib.amdkge_sample_negatives(P(tri), B, eta, 0, N, SEED, STEP, 17, B + 40, mode, P(thr), P(pl), 5 if pool else 0, *(P(t) for t in f),
                                           4, P(stats), P(out), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal((o["negs"] >= 0) & (o["negs"] < N), True))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["stats"] >= 3, True))


def case_side_thresholds(ar, n, N, R):
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex

    lib = _ffi.lib()
    rng = np.random.default_rng(8)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    X[0] = (N - 1, R - 1, N - 1)
    fi = FilterIndex([X], N, R)
    po, sp = ar.put("po_keys", fi.po_keys.astype(np.int64)), ar.put("sp_keys", fi.sp_keys.astype(np.int64))
    thr = ar.out("thr", (R,), np.int32, 7)
    _ffi.check(lib.amdkge_negatives_side_thresholds(P(po), len(fi.po_keys), P(sp), len(fi.sp_keys), N, R, P(thr), None))
    want = NR.side_thresholds(fi.po_keys, fi.sp_keys, N, R)
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["thr"].view(np.uint32), want))


# entry point of include/amdkge_negatives.h -> [(case function, its arguments), ...]
NEG_CASES = {
    "amdkge_sample_negatives": [(case_sample_negatives, dict(B=37, eta=3, mode=NR.BERNOULLI, pool=True, flt=True)),
                                (case_sample_negatives, dict(B=130, eta=3, mode=NR.UNIFORM, pool=False, flt=True)),
                                (case_sample_negatives, dict(B=1, eta=1, mode=NR.S_ONLY, pool=False, flt=False))],
    "amdkge_negatives_side_thresholds": [(case_side_thresholds, dict(n=130, N=37, R=5)), (case_side_thresholds, dict(n=9, N=130, R=257))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in NEG_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    from test_gpu_guard_bands import run_case

    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_negatives.h")
    assert declared and declared == set(NEG_CASES) and all(NEG_CASES.values())
