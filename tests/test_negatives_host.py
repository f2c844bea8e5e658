"""The training negative samplers without a GPU: what is the extension header's own (include/amdkge_negatives.h; names
and types: tests/test_abi_host.py), the argument validation of both entry points, the numpy restatement of the
draw (tests/negatives_ref.py) against oracle/philox.py, the threshold formula on hand-counted relations, and NegativeSampling's /
compile()'s validation."""
import ctypes as C

import numpy as np
import pytest

import abi_decl
import negatives_ref as NR
from ampligraph_amd._ffi import EINVAL


# ------------------------------------------------------------------------------------------------------------ header and binding table
def test_extension_header_and_its_signature_table():
    from ampligraph_amd import _ffi

    hdr = abi_decl.text("amdkge.h")
    assert hdr.count('#include "amdkge_negatives.h"') == 1
    assert hdr.rstrip().endswith('#include "amdkge_negatives.h"\n#endif /* AMDKGE_H */')
    # the names the engine passes and the numpy restatement's
    for name, val in (("UNIFORM", "uniform"), ("BERNOULLI", "bernoulli"), ("S_ONLY", "s"), ("O_ONLY", "o")):
        assert _ffi.NEG_SIDE_MODES[val] == getattr(NR, name)


# ------------------------------------------------------------------------------------------------------------ argument validation
def test_sample_negatives_argument_validation_without_gpu():
    """Every error below is returned before any device work: the pointers that are set are never dereferenced."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)

    def call(tri=X, B=5, eta=2, base=0, rng=50, seed=1, step=2, row_offset=0, b_global=0, mode=NR.UNIFORM, thr=None, pool=None, pool_n=0,
             slo=None, shi=None, sids=None, olo=None, ohi=None, oids=None, max_tries=8, stats=None, out=X):
        return lib.amdkge_sample_negatives(tri, B, eta, base, rng, seed, step, row_offset, b_global, mode, thr, pool, pool_n, slo, shi, sids, olo, ohi,
                                           oids, max_tries, stats, out, None)

    assert call(out=None) == EINVAL and b"NULL" in lib.amdkge_last_error()
    assert call(tri=None) == EINVAL and b"NULL" in lib.amdkge_last_error()
    assert call(B=-1) == EINVAL and b"negative" in lib.amdkge_last_error()
    assert call(eta=-1) == EINVAL and call(row_offset=-1) == EINVAL
    six = ("slo", "shi", "sids", "olo", "ohi", "oids")
    for k in range(1, 6):                                                   # a range array without its siblings
        assert call(**{nm: X for nm in six[:k]}) == EINVAL and b"together" in lib.amdkge_last_error(), k
        assert call(**{nm: X for nm in six[k:]}) == EINVAL, k
    for bad in (0, -1, 33, 1 << 20):
        assert call(max_tries=bad) == EINVAL and b"max_tries" in lib.amdkge_last_error(), bad
    assert call(mode=NR.BERNOULLI) == EINVAL and b"d_side_thr" in lib.amdkge_last_error()
    assert call(mode=4) == EINVAL and call(mode=-1) == EINVAL and b"side_mode" in lib.amdkge_last_error()
    for bad in (0, -3, 1 << 32):
        assert call(pool=X, pool_n=bad) == EINVAL and b"pool_n" in lib.amdkge_last_error(), bad
        assert call(rng=bad) == EINVAL and b"sample_range" in lib.amdkge_last_error(), bad
    assert call(eta=1 << 20, b_global=1 << 36) == EINVAL and b"2^56" in lib.amdkge_last_error()
    assert call(eta=1 << 8, B=1 << 48, b_global=0) == EINVAL            # (b_global defaults to B)
    # nothing to do: OK before any launch, whatever the other pointers
    assert call(B=0) == 0 and call(eta=0) == 0 and call(B=0, tri=None) == 0
    assert call(B=0, mode=NR.BERNOULLI, thr=X, pool=X, pool_n=3, max_tries=32, stats=X, **{nm: X for nm in six}) == 0
    assert call(eta=0, out=None) == EINVAL                                # the checks come first


def test_side_thresholds_argument_validation_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)

    def call(po=X, n_po=4, sp=X, n_sp=4, n_ents=10, n_rels=3, thr=X):
        return lib.amdkge_negatives_side_thresholds(po, n_po, sp, n_sp, n_ents, n_rels, thr, None)

    for bad in (dict(n_po=-1), dict(n_sp=-1), dict(n_sp=1 << 31), dict(n_ents=0), dict(n_rels=0), dict(n_rels=-2), dict(n_ents=1 << 31), dict(n_rels=1 << 31)):
        assert call(**bad) == EINVAL and b"bad sizes" in lib.amdkge_last_error(), bad
    for missing in ("po", "sp", "thr"):
        assert call(**{missing: None}) == EINVAL and b"NULL" in lib.amdkge_last_error(), missing
    assert call(po=None, n_po=0, sp=None, n_sp=0, thr=None) == EINVAL     # an empty index still needs the output


# ------------------------------------------------------------------------------------------------------------ the restatement
def _graph(seed, n, N, R):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)


def _filters(X, N, R, rows=None):
    from ampligraph_amd.datasets.filters import FilterIndex

    fi = FilterIndex([X], N, R)
    T = X if rows is None else rows
    return fi, (*fi.subject_ranges(T), fi.s_ids), (*fi.object_ranges(T), fi.o_ids)


def test_try_zero_uniform_is_todays_draw():
    from oracle.philox import sample_corruption_draws

    B, eta, N, seed, step, off, bg = 37, 3, 130, 12345678901234, (1 << 33) + 5, 17, 77
    X = _graph(0, B, N, 5)
    got, redraws, exhausted = NR.sample_negatives(X, eta, seed, step, sample_range=N, row_offset=off, b_global=bg, max_tries=1)
    i, j = np.tile(np.arange(B), eta), np.repeat(np.arange(eta), B)
    keep, repl = sample_corruption_draws(j * bg + off + i, step, seed, N)
    want = np.stack([np.where(keep == 1, X[i, 0], repl), X[i, 1], np.where(keep == 1, repl, X[i, 2])], 1)
    assert np.array_equal(got, want) and redraws == 0 and exhausted == 0
    for mt in (8, 32):                                                     # without a filter no try is ever rejected
        assert np.array_equal(NR.sample_negatives(X, eta, seed, step, sample_range=N, row_offset=off, b_global=bg, max_tries=mt)[0], want)


def test_side_is_invariant_under_max_tries_and_blocks_differ():
    N, R, B, eta = 8, 2, 60, 4
    X = _graph(1, B, N, R)
    fi, sf, of = _filters(X, N, R)
    thr = NR.side_thresholds(fi.po_keys, fi.sp_keys, N, R)
    i = np.tile(np.arange(B), eta)
    for mode in (NR.UNIFORM, NR.BERNOULLI):
        outs = {}
        for mt in (1, 2, 3, 4, 8, 32):
            out, redraws, exhausted = NR.sample_negatives(X, eta, 3, 9, sample_range=N, side_mode=mode, side_thr=thr, s_filter=sf, o_filter=of, max_tries=mt)
            assert np.all((out[:, 0] == X[i, 0]) | (out[:, 2] == X[i, 2])) and np.array_equal(out[:, 1], X[i, 1])
            assert redraws <= (mt - 1) * B * eta and (mt > 1 or redraws == 0)
            outs[mt] = out
        # a row whose subject changed at some max_tries never has its OBJECT changed at another: the side is decided once
        any_s = np.any([out[:, 0] != X[i, 0] for out in outs.values()], 0)
        assert 0 < any_s.sum() < B * eta
        for mt, out in outs.items():
            assert np.array_equal(out[any_s, 2], X[i, 2][any_s]), (mode, mt)
    # the blocks of one row are different streams, and block 0 is the unmodified counter
    rows = np.arange(5, dtype=np.uint64) + np.uint64(1 << 40)
    b0, b1 = NR.block(rows, 7, 11, 0), NR.block(rows, 7, 11, 1)
    assert not np.array_equal(b0[1], b1[1])
    from oracle.philox import philox4x32_10

    assert np.array_equal(b0[0], philox4x32_10((rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32), 7, 0, 11, 0)[0])


@pytest.mark.parametrize("mode", [NR.UNIFORM, NR.BERNOULLI, NR.S_ONLY, NR.O_ONLY])
def test_two_halves_give_the_rows_of_the_whole_batch(mode):
    N, R, B, eta = 6, 3, 41, 3
    X = _graph(2, B, N, R)
    fi, sf, of = _filters(X, N, R)
    thr = NR.side_thresholds(fi.po_keys, fi.sp_keys, N, R)
    pool = np.array([5, 0, 3, 3, 1], dtype=np.int32)
    kw = dict(sample_range=N, side_mode=mode, side_thr=thr, pool=pool, max_tries=5)
    whole, rd, ex = NR.sample_negatives(X, eta, 5, 6, s_filter=sf, o_filter=of, **kw)
    cut = 17
    parts, rds, exs = [], 0, 0
    for a, b in ((0, cut), (cut, B)):
        part = lambda f: (f[0][a:b], f[1][a:b], f[2])   # noqa: E731
        out, r, e = NR.sample_negatives(X[a:b], eta, 5, 6, row_offset=a, b_global=B, s_filter=part(sf), o_filter=part(of), **kw)
        parts.append(out.reshape(eta, b - a, 3))
        rds, exs = rds + r, exs + e
    assert np.array_equal(np.concatenate(parts, 1).reshape(-1, 3), whole) and (rds, exs) == (rd, ex)
    assert rd > 0                                                          # (the graph is dense enough for the filter to matter)


# ------------------------------------------------------------------------------------------------------------ thresholds
def test_threshold_formula_on_hand_counted_relations():
    from ampligraph_amd.datasets.filters import FilterIndex

    N, R = 20, 5
    X = np.array([(0, 0, t) for t in range(1, 8)]          # relation 0: 1 head x 7 tails
                 + [(h, 1, 0) for h in range(1, 8)]        # relation 1: 7 heads x 1 tail
                 + [(h, 2, h + 1) for h in range(6)]       # relation 2: 1-to-1
                 + [(0, 4, 1), (0, 4, 2), (0, 4, 3), (5, 4, 1), (5, 4, 1)],   # relation 4: 2 (s, p) groups, 3 (p, o) groups, a duplicate
                 dtype=np.int32)                           # relation 3: never seen
    fi = FilterIndex([X], N, R)
    thr = NR.side_thresholds(fi.po_keys, fi.sp_keys, N, R)
    assert thr.dtype == np.uint32
    assert [int(v) for v in thr] == [0xE0000000, 0x20000000, 0x80000000, 0x80000000, (3 << 32) // 5]
    assert (3 << 32) // 5 == 2576980377                                    # floor, not round (2576980377.6)
    assert [int(v) for v in NR.side_thresholds(np.zeros(0, np.int64), np.zeros(0, np.int64), N, 2)] == [0x80000000] * 2


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_negative_sampling_validation():
    from ampligraph_amd.latent_features.negatives import NegativeSampling

    d = NegativeSampling()
    assert (d.filter, d.side, d.entities, d.max_tries) == (False, "uniform", None, 8)
    ok = NegativeSampling(filter={"test": np.zeros((1, 3))}, side="bernoulli", entities=["a", "b"], max_tries=32)
    assert ok.side == "bernoulli" and ok.max_tries == 32 and list(ok.entities) == ["a", "b"] and isinstance(ok.filter, dict)
    for bad in (dict(filter="train"), dict(filter=1), dict(filter={}), dict(filter=None), dict(side="both"), dict(side=None), dict(side="S"),
                dict(max_tries=0), dict(max_tries=33), dict(max_tries=2.0), dict(max_tries=True), dict(entities=[]), dict(entities="abc"),
                dict(entities=[["a"], ["b"]])):
        with pytest.raises(ValueError, match="negatives"):
            NegativeSampling(**bad)
    assert NegativeSampling.get(None) is None and NegativeSampling.get(ok) is ok
    got = NegativeSampling.get({"filter": True, "side": "o", "max_tries": 3})
    assert (got.filter, got.side, got.max_tries) == (True, "o", 3)
    assert got.get_config() == {"filter": True, "side": "o", "entities": None, "max_tries": 3}
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"filtered": True})
    with pytest.raises(ValueError, match="negatives"):
        NegativeSampling.get("bernoulli")


def test_compile_takes_the_setting_and_refuses_it_on_sharded_tables():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import NegativeSampling

    m = ScoringBasedEmbeddingModel(eta=2, k=4)
    assert m._negatives is None
    m.compile(optimizer="adam", loss="nll")
    assert m._negatives is None
    m.compile(optimizer="adam", loss="nll", negatives={"filter": True, "side": "bernoulli"})
    assert isinstance(m._negatives, NegativeSampling) and m._negatives.filter is True and m._negatives.side == "bernoulli"
    m.compile(optimizer="adam", loss="nll")                                # compiled again without it: off again
    assert m._negatives is None
    for sharding in ("rows", "columns"):
        with pytest.raises(NotImplementedError, match="entity_sharding"):
            m.compile(optimizer="adam", loss="nll", entity_sharding=sharding, negatives={"filter": True})
        m.compile(optimizer="adam", loss="nll", entity_sharding=sharding)   # (without a sampler the modes compile as before)
    with pytest.raises(ValueError, match="side"):
        m.compile(optimizer="adam", loss="nll", negatives={"side": "random"})


def test_step_loop_hands_the_sampler_its_slice_and_passes_the_rows_on():
    import torch

    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    calls = []

    class Eng:
        scoring_type, k = "TransE", 8   # (narrow TransE: the atomic path)

        def prepare_training(self, name):
            pass

        def train_fwdbwd(self, triples, eta, loss, seed, step, **kw):
            calls.append(("fwdbwd", tuple(triples.shape), kw))

        def opt_step(self, *a, **kw):
            pass

    loop = StepLoop(Eng(), 3, loss_functions.get("nll"), optimizers.get("sgd"), None, seed=7, dist=None)
    assert loop.negatives is None
    batch = torch.zeros(10, 3, dtype=torch.int32)
    loop.step(batch, 5)
    assert calls[-1][2] == {"row_offset": 0, "b_global": 10}              # without a sampler: today's call, no new keyword
    rows = torch.ones(30, 3, dtype=torch.int32)
    seen = []
    loop.negatives = lambda gb, lo, hi, eta, seed, step: (seen.append((gb is batch, lo, hi, eta, seed, step)), rows)[1]
    loop.step(batch, 6)
    assert seen == [(True, 0, 10, 3, 7, 6)]
    assert calls[-1][2]["neg_override"] is rows and calls[-1][2]["row_offset"] == 0 and calls[-1][2]["b_global"] == 10


def test_bound_sampler_finds_the_rows_of_a_batch():
    import torch

    from ampligraph_amd.latent_features.negatives import BoundNegatives

    b = object.__new__(BoundNegatives)
    b.train = torch.arange(60, dtype=torch.int32).view(20, 3)
    assert b._first_row(b.train) == 0 and b._first_row(b.train[7:12]) == 7 and b._first_row(b.train[19:]) == 19
    for bad in (b.train.clone()[2:4], b.train[:, :2], b.train.view(-1)[1:7].view(2, 3), b.train[::2]):
        with pytest.raises(ValueError, match="row slice"):
            b._first_row(bad)
