"""Type-constrained negatives and evaluation without a GPU: what is the extension header's own (include/amdkge_types.h; names and
types: tests/test_abi_host.py), the argument validation of the three entry points, the typed sampler kernel's
resources in the built code object, the numpy restatement's own identities (tests/types_ref.py), and the validation of
RelationTypes / TypedNegatives / compile() / evaluate_typed()."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_decl
import negatives_ref as NR
import types_ref as TR
from ampligraph_amd._ffi import EINVAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ header and binding table
def test_extension_header_and_its_signature_table():
    from ampligraph_amd import _ffi

    types = _ffi.ABI["amdkge_types.h"]
    hdr = abi_decl.text("amdkge.h")
    assert hdr.count('#include "amdkge_types.h"') == 1 and hdr.index('#include "amdkge_types.h"') > hdr.index("amdkge_session_group_rank(")
    # the typed sampler takes amdkge_sample_negatives' arguments in their order, then six pointers, then the stream
    plain, typed = _ffi.ABI["amdkge_negatives.h"]["amdkge_sample_negatives"][1], types["amdkge_sample_negatives_typed"][1]
    assert typed[:len(plain) - 1] == plain[:-1] and typed[len(plain) - 1:] == [C.c_void_p] * 7
    assert types["amdkge_relation_sets_build"] == _ffi.ABI["amdkge.h"]["amdkge_filter_build"]


def test_typed_sampler_kernel_uses_no_scratch_and_no_lds():
    from ampligraph_amd.utils.codeobj import kernel_resources

    res = kernel_resources(os.path.join(ROOT, "ampligraph_amd", "lib", "libamdkge.so"))
    typed = [k for n, k in res.items() if "negatives_typed_kernel" in n]
    assert len(typed) == 1
    print("negatives_typed_kernel:", typed[0])
    assert typed[0]["scratch"] == 0 and typed[0]["lds"] == 0
    plain = [k for n, k in res.items() if "negatives_kernel" in n]
    assert len(plain) == 1 and plain[0]["scratch"] == 0 and plain[0]["lds"] == 0


# ------------------------------------------------------------------------------------------------------------ argument validation
def test_relation_sets_argument_validation_without_gpu():
    """Every error below is returned before any device work: the pointers that are set are never dereferenced."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)

    def build(tri=X, m=5, side=1, N=10, R=3, keys=X, start=X, ids=X, counts=X, work=X):
        return lib.amdkge_relation_sets_build(tri, m, side, N, R, keys, start, ids, counts, work, None)

    for bad in (0, 3, 4, 5, -1):
        assert build(side=bad) == EINVAL and b"side" in lib.amdkge_last_error(), bad
    for bad in (dict(m=-1), dict(N=0), dict(R=0), dict(N=-4), dict(m=1 << 32)):
        assert build(**bad) == EINVAL and b"bad sizes" in lib.amdkge_last_error(), bad
    for missing in ("tri", "keys", "start", "ids", "counts", "work"):
        assert build(**{missing: None}) == EINVAL and b"NULL" in lib.amdkge_last_error(), missing
    assert build(m=0, start=None) == EINVAL and build(m=0, counts=None) == EINVAL
    assert build(N=1 << 31, R=1 << 10) == -5 and b"64-bit" in lib.amdkge_last_error()       # AMDKGE_EUNSUPPORTED: the shared plan's limit

    def look(keys=X, start=X, n_keys=4, tri=X, n=5, min_size=2, fb_lo=0, fb_hi=0, lo=X, hi=X):
        return lib.amdkge_relation_sets_ranges(keys, start, n_keys, tri, n, min_size, fb_lo, fb_hi, lo, hi, None)

    for bad in (dict(n=-1), dict(n_keys=-1), dict(min_size=-1), dict(fb_lo=-1), dict(fb_lo=5, fb_hi=4)):
        assert look(**bad) == EINVAL and b"bad sizes" in lib.amdkge_last_error(), bad
    for missing in ("keys", "start", "tri", "lo", "hi"):
        assert look(**{missing: None}) == EINVAL and b"NULL" in lib.amdkge_last_error(), missing
    assert look(n=0) == 0 and look(n=0, keys=None, start=None, tri=None, lo=None, hi=None) == 0   # nothing to do


def test_sample_negatives_typed_argument_validation_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)
    six = ("slo", "shi", "sids", "olo", "ohi", "oids")
    cand = ("cslo", "cshi", "csids", "colo", "cohi", "coids")

    def call(tri=X, B=5, eta=2, base=0, rng=50, seed=1, step=2, row_offset=0, b_global=0, mode=NR.UNIFORM, thr=None, pool=None, pool_n=0,
             max_tries=8, stats=None, out=X, **arrays):
        a = [arrays.pop(nm, None) for nm in six + cand]
        assert not arrays
        return lib.amdkge_sample_negatives_typed(tri, B, eta, base, rng, seed, step, row_offset, b_global, mode, thr, pool, pool_n, *a[:6], max_tries,
                                                 stats, out, *a[6:], None)

    assert call(out=None) == EINVAL and b"NULL" in lib.amdkge_last_error()
    assert call(tri=None) == EINVAL and b"NULL" in lib.amdkge_last_error()
    assert call(B=-1) == EINVAL and b"negative" in lib.amdkge_last_error() and b"sample_negatives_typed" in lib.amdkge_last_error()
    assert call(eta=-1) == EINVAL and call(row_offset=-1) == EINVAL
    for k in range(1, 6):                                                   # an array without its siblings, in either group of six
        assert call(**{nm: X for nm in six[:k]}) == EINVAL and b"range arrays" in lib.amdkge_last_error(), k
        assert call(**{nm: X for nm in six[k:]}) == EINVAL, k
        assert call(**{nm: X for nm in cand[:k]}) == EINVAL and b"candidate arrays" in lib.amdkge_last_error(), k
        assert call(**{nm: X for nm in cand[k:]}) == EINVAL and b"together" in lib.amdkge_last_error(), k
        assert call(**{nm: X for nm in six + cand[:k]}) == EINVAL, k
    for bad in (0, -1, 33, 1 << 20):
        assert call(max_tries=bad) == EINVAL and b"max_tries" in lib.amdkge_last_error(), bad
    assert call(mode=NR.BERNOULLI) == EINVAL and b"d_side_thr" in lib.amdkge_last_error()
    assert call(mode=4) == EINVAL and call(mode=-1) == EINVAL and b"side_mode" in lib.amdkge_last_error()
    for bad in (0, -3, 1 << 32):                                           # the untyped rule must be usable even when every range is typed
        assert call(pool=X, pool_n=bad, **{nm: X for nm in cand}) == EINVAL and b"pool_n" in lib.amdkge_last_error(), bad
        assert call(rng=bad, **{nm: X for nm in cand}) == EINVAL and b"sample_range" in lib.amdkge_last_error(), bad
    assert call(eta=1 << 20, b_global=1 << 36) == EINVAL and b"2^56" in lib.amdkge_last_error()
    # nothing to do: OK before any launch, whatever the other pointers
    assert call(B=0) == 0 and call(eta=0) == 0 and call(B=0, tri=None) == 0
    assert call(B=0, mode=NR.BERNOULLI, thr=X, pool=X, pool_n=3, max_tries=32, stats=X, **{nm: X for nm in six + cand}) == 0
    assert call(eta=0, out=None) == EINVAL                                # the checks come first


# ------------------------------------------------------------------------------------------------------------ the restatement
def _graph(seed, n, N, R):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)


def _filters(X, N, R):
    from ampligraph_amd.datasets.filters import FilterIndex

    fi = FilterIndex([X], N, R)
    return (*fi.subject_ranges(X), fi.s_ids), (*fi.object_ranges(X), fi.o_ids)


def test_ref_sets_and_lookup_on_a_hand_counted_graph():
    from ampligraph_amd.datasets.types import sets_csr

    X = np.array([(4, 0, 1), (2, 0, 1), (4, 0, 9), (4, 0, 1), (7, 2, 7), (0, 3, 5), (1, 3, 5)], np.int32)   # relation 1 absent, a duplicate row
    keys, start, ids = TR.build_sets(X, "s")
    assert keys.tolist() == [0, 2, 3] and start.tolist() == [0, 2, 3, 5] and ids.tolist() == [2, 4, 7, 0, 1]
    keys_o, start_o, ids_o = TR.build_sets(X, "o")
    assert keys_o.tolist() == [0, 2, 3] and start_o.tolist() == [0, 2, 3, 4] and ids_o.tolist() == [1, 9, 7, 5]
    for sd in "so":                                                        # the product's host restatement (a sort) agrees
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(TR.build_sets(X, sd), sets_csr(X, sd)))
    e = TR.build_sets(np.zeros((0, 3), np.int32), "s")
    assert [a.tolist() for a in e] == [[], [0], []] and all(np.array_equal(a, b) for a, b in zip(e, sets_csr(np.zeros((0, 3), np.int32), "s")))
    Q = np.array([(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0)], np.int32)
    lo, hi = TR.ranges(keys, start, Q)
    assert lo.tolist() == [0, 0, 2, 3, 0] and hi.tolist() == [2, 0, 3, 5, 0]
    lo, hi = TR.ranges(keys, start, Q, min_size=2, fallback=(5, 15))       # absent (1, 4) and below min_size (2) fall back
    assert lo.tolist() == [0, 5, 5, 3, 5] and hi.tolist() == [2, 15, 15, 5, 15]
    lo, hi = TR.ranges(keys, start, Q, min_size=3, fallback=(0, 0))
    assert hi.tolist() == [0] * 5


@pytest.mark.parametrize("mode", [NR.UNIFORM, NR.BERNOULLI, NR.S_ONLY, NR.O_ONLY])
def test_ref_identities(mode):
    """a. no candidate arrays: amdkge_sample_negatives' draw (pool, filter and all); b. every range the ids 0 .. N-1: the untyped draw
    with sample_base 0, sample_range N"""
    N, R, B, eta = 9, 3, 41, 4
    X = _graph(2, B, N, R)
    sf, of = _filters(X, N, R)
    thr = np.array([0x20000000, 0x80000000, 0xE0000000], np.uint32)
    pool = np.array([5, 0, 3, 3, 1], dtype=np.int32)
    kw = dict(row_offset=3, b_global=B + 7, side_mode=mode, side_thr=thr, s_filter=sf, o_filter=of, max_tries=5)
    for pl in (None, pool):
        want, rd, ex = NR.sample_negatives(X, eta, 5, 6, sample_range=N, pool=pl, **kw)
        got, rd2, ex2, ut = TR.sample_negatives_typed(X, eta, 5, 6, sample_range=N, pool=pl, **kw)
        assert np.array_equal(got, want) and got.dtype == want.dtype and (rd2, ex2, ut) == (rd, ex, B * eta) and rd > 0
    want, rd, ex = NR.sample_negatives(X, eta, 5, 6, sample_base=0, sample_range=N, **kw)
    everyone = np.arange(N, dtype=np.int32)
    full = (np.zeros(B, np.int64), np.full(B, N, np.int64), everyone)
    shifted = (np.full(B, 4, np.int64), np.full(B, 4 + N, np.int64), np.concatenate([[7, 7, 7, 7], everyone]).astype(np.int32))
    for pl, rng in ((None, N), (pool, 1), (None, 3)):                      # (the untyped rule's tables do not matter when no range is empty)
        got, rd2, ex2, ut = TR.sample_negatives_typed(X, eta, 5, 6, sample_base=2, sample_range=rng, pool=pl, s_cand=full, o_cand=shifted, **kw)
        assert np.array_equal(got, want) and (rd2, ex2, ut) == (rd, ex, 0)


def test_ref_typed_draw_stays_inside_the_sets_and_counts_untyped():
    N, R, B, eta = 30, 4, 50, 6
    X = _graph(4, B, N, R)
    X[X[:, 1] == 3, 1] = 2                                                  # relation 3 has no set
    X[:5, 1] = 3
    csr = {sd: TR.build_sets(X[5:], sd) for sd in "so"}
    cand = {sd: (*TR.ranges(csr[sd][0], csr[sd][1], X, 2, (0, 0)), csr[sd][2]) for sd in "so"}
    i = np.tile(np.arange(B), eta)
    for mode, sd, col in ((NR.S_ONLY, "s", 0), (NR.O_ONLY, "o", 2)):
        out, rd, ex, ut = TR.sample_negatives_typed(X, eta, 1, 2, sample_range=N, side_mode=mode, s_cand=cand["s"], o_cand=cand["o"], max_tries=4)
        lo, hi, ids = cand[sd]
        n_untyped = int((hi == lo).sum())
        assert ut == n_untyped * eta >= 5 * eta and (rd, ex) == (0, 0)
        assert all(out[r, col] in ids[lo[q]:hi[q]] for r, q in enumerate(i) if hi[q] > lo[q])
        assert np.array_equal(out[:, 1], X[i, 1]) and np.array_equal(out[:, 2 - col], X[i, 2 - col])


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_relation_types_validation():
    from ampligraph_amd.datasets.types import RelationTypes

    ok = RelationTypes({"born_in": (["a", "b"], ["x"]), "likes": (None, ["a"]), "knows": (None, None)})
    assert not ok.is_observed and list(ok.sets["born_in"][0]) == ["a", "b"] and ok.sets["likes"][0] is None
    assert RelationTypes({}).sets == {}
    for bad in ("observed", None, [("r", (None, None))]):
        with pytest.raises(ValueError, match="types"):
            RelationTypes(bad)
    for pair in (None, "ab", (None,), (None, None, None), ([], None), (None, "abc"), ([["a"]], None)):
        with pytest.raises(ValueError, match="types"):
            RelationTypes({"r": pair})
    ob = RelationTypes.observed()
    assert ob.is_observed and ob.datasets is None
    d = {"train": np.zeros((2, 3)), "test": np.ones((1, 3))}
    assert len(RelationTypes.observed(d).datasets) == 2 and len(RelationTypes.observed(d["train"]).datasets) == 1
    with pytest.raises(ValueError, match="types"):
        RelationTypes.observed([])
    assert set(ob.get_config()) == {"observed", "datasets", "sets"}


def test_typed_negatives_validation_and_dict_dispatch():
    from ampligraph_amd.datasets.types import RelationTypes
    from ampligraph_amd.latent_features.negatives import NegativeSampling, TypedNegatives

    d = TypedNegatives("observed")
    assert (d.filter, d.side, d.entities, d.max_tries, d.min_size) == (False, "uniform", None, 8, 2) and d.types.is_observed
    rt = RelationTypes({"r": (["a"], None)})
    ok = TypedNegatives(rt, filter=True, side="bernoulli", entities=["a", "b"], max_tries=32, min_size=1)
    assert ok.types is rt and ok.min_size == 1 and ok.side == "bernoulli" and ok.filter is True
    for bad in (dict(types=None), dict(types="lcwa"), dict(types={"r": (None, None)}), dict(types="observed", min_size=0),
                dict(types="observed", min_size=2.0), dict(types="observed", min_size=True), dict(types="observed", side="both"),
                dict(types="observed", max_tries=0), dict(types="observed", filter="train"), dict(types="observed", entities=[])):
        with pytest.raises(ValueError, match="negatives"):
            TypedNegatives(**bad)
    got = NegativeSampling.get({"types": "observed", "filter": True, "side": "o", "min_size": 3})
    assert type(got) is TypedNegatives and (got.filter, got.side, got.min_size) == (True, "o", 3) and got.types.is_observed
    assert type(NegativeSampling.get({"types": rt})) is TypedNegatives and NegativeSampling.get(ok) is ok
    cfg = got.get_config()
    assert cfg == {"filter": True, "side": "o", "entities": None, "max_tries": 8, "types": got.types, "min_size": 3}
    assert type(NegativeSampling.get(cfg)) is TypedNegatives                # the config is the dict form
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"types": "observed", "group_size": 4})
    with pytest.raises(ValueError, match="unknown keys"):                  # without "types" the key is still unknown to NegativeSampling
        NegativeSampling.get({"min_size": 2})
    assert type(NegativeSampling.get({"filter": True})) is NegativeSampling


def test_compile_takes_typed_negatives_and_refuses_them_on_sharded_tables():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import TypedNegatives

    m = ScoringBasedEmbeddingModel(eta=2, k=4)
    m.compile(optimizer="adam", loss="nll", negatives={"types": "observed", "filter": True})
    assert type(m._negatives) is TypedNegatives and m._negatives.filter is True and not hasattr(m, "relation_types_")
    m.compile(optimizer="adam", loss="nll", negatives=TypedNegatives("observed"), deterministic=True)   # deterministic mode takes the override
    assert m._deterministic and type(m._negatives) is TypedNegatives
    for sharding in ("rows", "columns"):
        with pytest.raises(NotImplementedError, match="entity_sharding"):
            m.compile(optimizer="adam", loss="nll", entity_sharding=sharding, negatives={"types": "observed"})
    m.compile(optimizer="adam", loss="nll")
    assert m._negatives is None


def test_sharded_placements_refuse_rank_typed():
    from ampligraph_amd.placement import Columns, Replicated, Rows

    assert Replicated.lists_supported
    for cls in (Rows, Columns):
        pl = cls.__new__(cls)
        assert not pl.lists_supported
        with pytest.raises(NotImplementedError, match="evaluate_typed.*sharded"):
            pl.rank_typed(np.zeros((1, 3), np.int32), ["s"], None, None, "worst", 1)
        assert cls.rank_typed is not Replicated.rank_typed


def test_evaluate_typed_validates_before_any_device_work():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    m = ScoringBasedEmbeddingModel(eta=2, k=4)
    x = np.array([["a", "r", "b"]])
    with pytest.raises(ValueError, match="ranking_strategy"):
        m.evaluate_typed(x, ranking_strategy="random")
    with pytest.raises(ValueError, match="corrupt_side"):
        m.evaluate_typed(x, corrupt_side="both")
    with pytest.raises(ValueError, match="not fitted"):
        m.evaluate_typed(x)
    m.is_fitted = True
    with pytest.raises(ValueError, match="use_filter"):
        m.evaluate_typed(x, use_filter="train")
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="min_size"):
            m.evaluate_typed(x, min_size=bad)
    from ampligraph_amd.placement import Replicated, Rows

    m._placement = Rows.__new__(Rows)
    with pytest.raises(NotImplementedError, match="sharded"):
        m.evaluate_typed(x)
    m._placement = Replicated.__new__(Replicated)
    with pytest.raises(ValueError, match="relation_types_"):
        m.evaluate_typed(x)
    with pytest.raises(ValueError, match="types"):
        m.evaluate_typed(x, types="observed")
