"""Guard bands (tests/guarded.py, the harness of tests/test_gpu_guard_bands.py) around every buffer the entry points of
include/amdkge_types.h are handed: no write outside a buffer, no result that depends on bytes outside one.  d_stats has exactly
the three words the typed sampler adds to; the build's outputs have exactly the capacity m."""
import numpy as np
import pytest

import negatives_ref as NR
import types_ref as TR
from abi_decl import declared_names
from test_gpu_guard_bands import I32, I64, P, run_case

pytestmark = pytest.mark.gpu

SEED, STEP = 12345678901234, (1 << 33) + 5


def _lib():
    from ampligraph_amd import _ffi

    return _ffi, _ffi.lib()


def _triples(seed, m, N, R):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.integers(0, N, m), rng.integers(0, R, m), rng.integers(0, N, m)], 1).astype(I32)
    X[: m // 3] = X[0]                                                # duplicates
    X[-1] = (N - 1, R - 1, N - 1)                                     # the last relation, the last entity
    return X


def case_relation_sets_build(ar, side, m, N=23, R=5):
    """the outputs are valid up to n_groups / n_unique (d_counts); what lies behind is unspecified, so the compared form is the valid part"""
    _ffi, lib = _lib()
    X = _triples(3, m, N, R)
    tri = ar.put("triples", X)
    keys, start, ids = ar.out("keys", (m,), I64, 1), ar.out("start", (m + 1,), I64, 1), ar.out("ids", (m,), I32, 1)
    counts = ar.out("counts", (2,), I64, 0)
    work = ar.work("work", lib.amdkge_filter_build_workspace_bytes(m, N, R))
    _ffi.check(lib.amdkge_relation_sets_build(P(tri), m, 1 if side == "s" else 2, N, R, P(keys), P(start), P(ids), P(counts), P(work), None))
    ar.canon["keys"] = lambda v, o: v[:o["counts"][0]]
    ar.canon["start"] = lambda v, o: v[:o["counts"][0] + 1]
    ar.canon["ids"] = lambda v, o: v[:o["counts"][1]]
    rk, rs, ri = TR.build_sets(X, side)

    def expect(o):
        ng, nu = (int(c) for c in o["counts"])
        assert (ng, nu) == (len(rk), len(ri))
        assert np.array_equal(o["keys"][:ng], rk) and np.array_equal(o["start"][:ng + 1], rs) and np.array_equal(o["ids"][:nu], ri)

    ar.expects.append(expect)


def case_relation_sets_ranges(ar, n, min_size, N=23, R=7):
    """relations 5 and 6 are absent from the index; the queries hold the first and the last key"""
    _ffi, lib = _lib()
    rk, rs, ri = TR.build_sets(_triples(3, 130, N, 5), "o")
    X = _triples(9, n, N, R)
    X[0, 1] = 0
    keys, start, tri = ar.put("keys", rk), ar.put("start", rs), ar.put("triples", X)
    lo, hi = ar.out("lo", (n,), I64, 1), ar.out("hi", (n,), I64, 1)
    fb = (len(ri), len(ri) + N)
    _ffi.check(lib.amdkge_relation_sets_ranges(P(keys), P(start), len(rk), P(tri), n, min_size, fb[0], fb[1], P(lo), P(hi), None))
    want = TR.ranges(rk, rs, X, min_size, fb)
    ar.expects.append(lambda o: (np.testing.assert_array_equal(o["lo"], want[0]), np.testing.assert_array_equal(o["hi"], want[1])))


def case_sample_negatives_typed(ar, B, eta, mode, pool, flt, typed):
    """every device argument between bands; filter and candidate ranges end with the last id of their arrays, a candidate range of the
    last positive is the last set; d_stats is exactly three words"""
    _ffi, lib = _lib()
    rng = np.random.default_rng(7)
    N, R = 130, 5
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(I32)
    X[0], X[-1, 2] = (N - 1, R - 1, 0), N - 1
    tri = ar.put("triples", X)
    thr_np = rng.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    thr = ar.put("thr", thr_np.view(I32)) if mode == NR.BERNOULLI else None
    pool_np = np.array([N - 1, 0, 5, 5, 77], I32) if pool else None
    pl = ar.put("pool", pool_np) if pool else None

    def ragged(names, lens, empty_some):
        out_np, out = [], []
        for side in names:
            cnt = rng.integers(1, lens, B)
            if empty_some:
                cnt[rng.random(B) < 0.3] = 0
            cnt[-1] = lens + 30
            start = np.zeros(B + 1, I64)
            start[1:] = np.cumsum(cnt)
            ids = np.concatenate([np.sort(rng.permutation(N)[:c]) for c in cnt]).astype(I32)
            out_np.append((start[:-1].copy(), start[1:].copy(), ids))
            out += [ar.put(side + "_lo", out_np[-1][0]), ar.put(side + "_hi", out_np[-1][1]), ar.put(side + "_ids", ids)]
        return out_np, out

    f_np, f = ragged(("s", "o"), 90, True) if flt else ((None, None), [None] * 6)
    c_np, c = ragged(("cs", "co"), 60, True) if typed else ((None, None), [None] * 6)
    stats = ar.out("stats", (3,), I64, 3)
    out = ar.out("negs", (B * eta, 3), I32, 1)
    _ffi.check(lib.amdkge_sample_negatives_typed(P(tri), B, eta, 0, N, SEED, STEP, 17, B + 40, mode, P(thr), P(pl), 5 if pool else 0, *(P(t) for t in f),
                                                 4, P(stats), P(out), *(P(t) for t in c), None))
    want = TR.sample_negatives_typed(X, eta, SEED, STEP, sample_range=N, row_offset=17, b_global=B + 40, side_mode=mode, side_thr=thr_np, pool=pool_np,
                                     s_filter=f_np[0], o_filter=f_np[1], max_tries=4, s_cand=c_np[0], o_cand=c_np[1])
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["negs"], want[0]))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["stats"], 3 + np.array(want[1:])))


# entry point of include/amdkge_types.h -> [(case function, its arguments), ...]
TYPES_CASES = {
    "amdkge_relation_sets_build": [(case_relation_sets_build, dict(side="s", m=130)), (case_relation_sets_build, dict(side="o", m=130)),
                                   (case_relation_sets_build, dict(side="o", m=1))],
    "amdkge_relation_sets_ranges": [(case_relation_sets_ranges, dict(n=37, min_size=2)), (case_relation_sets_ranges, dict(n=257, min_size=0)),
                                    (case_relation_sets_ranges, dict(n=1, min_size=1000))],
    "amdkge_sample_negatives_typed": [(case_sample_negatives_typed, dict(B=37, eta=3, mode=NR.BERNOULLI, pool=True, flt=True, typed=True)),
                                      (case_sample_negatives_typed, dict(B=130, eta=3, mode=NR.UNIFORM, pool=False, flt=True, typed=True)),
                                      (case_sample_negatives_typed, dict(B=65, eta=2, mode=NR.O_ONLY, pool=False, flt=False, typed=True)),
                                      (case_sample_negatives_typed, dict(B=1, eta=1, mode=NR.S_ONLY, pool=False, flt=False, typed=False))],
}


@pytest.mark.parametrize("fn,kw", [pytest.param(fn, kw, id=fn.__name__[5:] + "-" + "-".join(str(v) for v in kw.values())) for cases in TYPES_CASES.values() for fn, kw in cases])
def test_guard_bands(gpu_lib, fn, kw):
    """bands on fill A, on fill B and ordinary tensors: bands clean, inputs unchanged, outputs bit-identical between the three"""
    run_case(fn, kw)


def test_every_extension_header_entry_has_a_case():
    declared = declared_names("amdkge_types.h")
    assert declared and declared == set(TYPES_CASES) and all(TYPES_CASES.values())
