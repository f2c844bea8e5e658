"""Every width of evaluate()'s count pass against the declared-order oracle (oracle/rank_ordered.py), bit for bit.

test_gpu_fullsize holds seven shapes to that oracle; test_gpu_rank_screen and test_gpu_rank_early compare the screened pass and
the early exit with the product's own exact kernels.  A rounding point or an accumulation order that an exact kernel and its
front-end share at some width passes all of those, so here each kernel meets the oracle on its own, at small shapes
(N ~ 3 000 candidates, n ~ 300 queries: partial last entity tile, partial last query block, above the n >= 128 / N >= 512 below
which rank_counts_impl does not screen):

  * contraction models, slab counts S = ceil(U / 32) of the screening pass (U = stored units of a row): S = 1, 2, 3 and 14, 19, 22,
    64 (rank_screen_kernel_v1; 64 = the pass's upper limit U = 2 048), each of S = 4 .. 13 from a one-plane (DistMult) and a
    two-halves (ComplEx / HolE, the latter with its 2 / k scale) model -- all ten rank_screen_kernel_r instantiations --, padded
    halves, and dense rows whose unit count is no multiple of 4 (the scalar-load kernels, never screened); under the VALU tile
    kernel, both fp32 MFMA kernels and the default (screened) path, each against the oracle independently; on tables of scores
    of a few units ("gaussian"), of exact ties ("ties") and of scores large enough for every ulp of a chain to move a quantised
    score ("large": what makes a wrong rounding point or accumulation order visible -- see _contraction_tables);
  * rank_screen_kernel_r across its 16-tile hand-over boundary (SCRR_UB), per slab count;
  * TransE / RotatE below, at and above the early exit's U >= 64, padded and odd widths: the plain tile kernel and the early exit;
  * candidate id lists, ranges that do not start on a tile, filters, tie strategies, corrupt_side forms, entities_subset and the
    two-sides-in-flight route of rank_sides at a few of those widths.

Exact equality everywhere: there are no tolerances in this module.  (The "wild" and non-finite families stay with the
self-comparisons: the oracle's semantics on inf / NaN are pinned by nothing.)"""
import contextlib

import numpy as np
import pytest
import torch

from oracle import kge_oracle as O
from oracle import rank_ordered as RO
from test_gpu_kernels import gpu_ranks
from test_gpu_rank_early import _counts as _early_counts   # (counts, (pairs handed over, fell back?, third statistics word))
from test_gpu_rank_early import _tables as distance_tables

pytestmark = pytest.mark.gpu

N_BASE, N_QUERIES, N_RELS = 3001, 300, 9   # 46 entity tiles of 64 + 57 rows; 2 query blocks of 128 + 44 rows
SIDES = (("s", "SIDE_S"), ("o", "SIDE_O"))


def _slabs(units):
    return (units + 31) // 32


def _contraction_tables(model, k, N, R, n, family, rng):
    K = O.internal_k(model, k)
    if family == "large":
        # Scores whose quantised value int32(score * 1000) sits around 2^24, so that a chain off by ONE ulp -- a rounding point more,
        # another accumulation order -- changes counts: at the 0.25 scale below an ulp is ~1e-4 of a quantisation step and such a
        # chain passes (a copy of the oracle with the fmaf unfused, or the units walked backwards, changes no count row of the
        # "gaussian" family at most widths listed below and one at the others; of this family 44 .. 112 resp. 134 .. 180 of 300).  A score is a
        # sum of k (DistMult) or 4 k (ComplEx, HolE) products of three table values, HolE's times 2 / k: with normal * s tables its
        # standard deviation is g s^3, g = sqrt(k), 2 sqrt(k), 4 / sqrt(k); s puts it at 2^24 / 1000.  The largest of the 5e6
        # scores of a case (~6 standard deviations) then quantises to ~1e8, far inside int32.
        g = {"DistMult": np.sqrt(k), "ComplEx": 2.0 * np.sqrt(k), "HolE": 4.0 / np.sqrt(k)}[model]
        s = float((2.0 ** 24 / 1000.0 / g) ** (1.0 / 3.0))
        ent = (rng.normal(size=(N, K)) * s).astype(np.float32)
        rel = (rng.normal(size=(R, K)) * s).astype(np.float32)
    elif family == "gaussian":   # scores of a few units, thousands of distinct quantised values (as test_gpu_fullsize)
        ent = (rng.normal(size=(N, K)) * 0.25).astype(np.float32)
        rel = (rng.normal(size=(R, K)) * 0.25).astype(np.float32)
    else:                        # "ties": many exactly equal scores, small integers / 8 (as test_gpu_rank_screen)
        ent = (rng.integers(-4, 5, size=(N, K)) / 8.0).astype(np.float32)
        rel = (rng.integers(-2, 3, size=(R, K)) / 4.0).astype(np.float32)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    return ent, rel, X


def _assert_kernel_r_kept_the_call(st, slabs, mcand, where):
    """Rows of 4 .. 13 slabs go to rank_screen_kernel_r<S> unless run_screen finds no room for its row records in the pair list
    (b.cap * 8 < mcand * 16: the list holds >= 2^20 pairs = 8 MiB, amdkge_rank_screen_workspace_bytes, against 16 x 33 250 bytes at
    the largest shape here, so it never does) or the device finds the candidate table wild -- which the third statistics word
    rules out.  (AMDKGE_SCREEN_KERNEL=1 in the environment pins rank_screen_kernel_v1; the library reports no kernel name.)"""
    if slabs is not None and 4 <= slabs <= 13:
        assert st[2] * 64 <= mcand, (where, st)


def _engine(model, k, ent, rel, pad=True):
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(model, k, ent.shape[0], rel.shape[0], max_rel_size=rel.shape[0], pad=pad)
    eng.set_tables(ent, rel)
    return eng


def _counts(eng, gpu_lib, Xd, side, which, **kw):
    """(counts, statistics) of one rank_side call under amdkge_set_rank_kernel(which), through test_gpu_rank_early's reader of the
    call's statistics words: (pairs handed to the exact chain, fell back?, third word) or None without a workspace.  The third
    word is "tiles ended early" for the distance models and, for the contraction models, the candidate rows that
    rank_limbs_tile_kernel found far below their tile's scale (screen_wild: more than m / 64 of them send the call from
    rank_screen_kernel_r to the per-row-scale path)."""
    from ampligraph_amd import _ffi

    return _early_counts(eng, gpu_lib, Xd, getattr(_ffi, side), which, **kw)


def _dot_scores_fp64(ctx):
    """All (query, candidate) scores of a contraction side in fp64, from the oracle's own query vectors (RO.prep)."""
    qpos, Q, mode, U, plane, scale, ent = ctx
    assert mode == RO.MODE_DOT
    return float(scale) * (Q.astype(np.float64) @ ent.astype(np.float64).T)


def _assert_every_ulp_shows(ctx, where):
    """The "large" family, from the oracle alone: int32(score * 1000) of the typical score lies beyond 2^21 -- there an ulp of the
    fp32 score is a quarter of a quantisation step or more, a thousand times the 0.25-scaled family's -- and every score well inside int32."""
    q = np.abs(_dot_scores_fp64(ctx)) * 1000.0
    assert np.median(q) > 2 ** 21 and q.max() < 2 ** 30, (where, float(np.median(q)), float(q.max()))


@contextlib.contextmanager
def _early_kernel_always(gpu_lib):
    """The early-exit kernel does the work whatever its probe would say (as test_gpu_rank_early's autouse fixture)."""
    gpu_lib.amdkge_set_rank_early(1, 4, 1, 16, 0)
    try:
        yield
    finally:
        gpu_lib.amdkge_set_rank_early(1, 4, 1, 16, 1)


# (model, k, pad, slabs).  DistMult: U = k rounded up to 4; ComplEx / HolE: U = 2 x (k rounded up to 4); pad=False: dense rows, U = K.
CONTRACTION_WIDTHS = [
    # rank_screen_kernel_v1 below kernel r
    ("DistMult", 32, True, 1), ("ComplEx", 20, True, 2), ("HolE", 40, True, 3), ("DistMult", 96, True, 3),
    # rank_screen_kernel_r<4 .. 13>, one plane
    ("DistMult", 100, True, 4), ("DistMult", 160, True, 5), ("DistMult", 164, True, 6), ("DistMult", 200, True, 7),
    ("DistMult", 256, True, 8), ("DistMult", 260, True, 9), ("DistMult", 300, True, 10), ("DistMult", 350, True, 11),   # 350 -> 352
    ("DistMult", 384, True, 12), ("DistMult", 400, True, 13),
    # rank_screen_kernel_r<4 .. 13>, two halves (ComplEx k = 50 -> 52, 90 -> 92, 150 -> 152, HolE k = 130 -> 132, 175 -> 176: padded)
    ("ComplEx", 50, True, 4), ("HolE", 80, True, 5), ("ComplEx", 90, True, 6), ("HolE", 100, True, 7), ("ComplEx", 128, True, 8),
    ("HolE", 130, True, 9), ("ComplEx", 150, True, 10), ("HolE", 175, True, 11), ("ComplEx", 192, True, 12), ("HolE", 196, True, 13),
    # rank_screen_kernel_v1 above kernel r: ComplEx k = 300 and HolE k = 350 (-> 352) are the reference's published widths
    ("DistMult", 420, True, 14), ("ComplEx", 300, True, 19), ("HolE", 350, True, 22),
    # the screened pass's upper limit, U = 2 048
    ("ComplEx", 1024, True, 64),
    # dense rows, unit count no multiple of 4: scalar loads, no screening
    ("DistMult", 37, False, None), ("DistMult", 50, False, None), ("HolE", 25, False, None), ("ComplEx", 101, False, None),
]


@pytest.mark.parametrize("family", ["gaussian", "ties", "large"])
@pytest.mark.parametrize("model,k,pad,slabs", CONTRACTION_WIDTHS)
def test_contraction_counts_equal_the_ordered_oracle(gpu_lib, model, k, pad, slabs, family):
    """(greater, equal) of both sides under the VALU tile kernel (1), the first MFMA kernel (2), the pipelined MFMA kernel (3;
    rows whose unit count is no multiple of 4: the scalar-load form of kernel 2) and the default path (0: the int8 screened pass +
    exact recheck wherever U % 4 == 0 and U <= 2 048), each against RO.side_counts."""
    N, n, R = N_BASE, N_QUERIES, N_RELS
    rng = np.random.default_rng(1000 * k + len(model))
    ent, rel, X = _contraction_tables(model, k, N, R, n, family, rng)
    eng = _engine(model, k, ent, rel, pad)
    U = eng.Ks
    screened = U % 4 == 0 and U <= 2048
    assert (_slabs(U) == slabs) if pad else not screened, (U, slabs)   # the case is the width it is listed as
    Xd = torch.as_tensor(X).cuda()
    for nm, side in SIDES:
        ref, ctx = RO.side_counts(model, nm, ent, rel, X, R)
        # a real ranking problem, from the oracle's counts alone
        if family in ("gaussian", "large"):
            assert len(np.unique(ref[:, 0])) > n // 2, (nm, len(np.unique(ref[:, 0])))
        else:
            assert int(ref[:, 1].sum()) > 0, nm
        if family == "large":
            _assert_every_ulp_shows(ctx, nm)
        for which in (1, 2, 3, 0):
            got, st = _counts(eng, gpu_lib, Xd, side, which)
            assert np.array_equal(got, ref), (nm, "kernel", which, "rows off", int((got != ref).any(1).sum()), st)
            if which == 0 and screened:   # the default path was the screened pass: workspace used, no fall-back, pairs rechecked
                assert st is not None and not st[1], (nm, st)
                if family in ("gaussian", "large"):
                    assert st[0] > 0, (nm, st)
                _assert_kernel_r_kept_the_call(st, slabs, N, nm)
            elif which == 0:              # ... and was not, where the pass does not apply
                assert st is None or st[0] == 0, (nm, st)


def _screen_r_run(n, m, slots=256, startup=1.0, run_cap=64, max_run=1024):
    """Entity tiles per block that run_screen's schedule (kge_rank_screen.hip) gives rank_screen_kernel_r for n queries against m
    candidates: the run length tp in 1 .. min(etiles, run_cap, max_run) with the smallest
    ceil(8 ceil(qtiles / 8) ceil(etiles / tp) / slots) x (tp + startup), ties to the longer run."""
    qtiles, etiles = -(-n // 128), -(-m // 64)
    qt8 = 8 * (-(-qtiles // 8))
    best, pick = None, 1
    for tp in range(1, min(etiles, run_cap, max_run) + 1):
        cost = -(-(qt8 * (-(-etiles // tp))) // slots) * (tp + startup)
        if best is None or cost <= best:
            best, pick = cost, tp
    return pick


@pytest.mark.parametrize("model,k,slabs", [("DistMult", 100, 4), ("HolE", 80, 5), ("DistMult", 164, 6), ("ComplEx", 100, 7), ("DistMult", 256, 8),
                                            ("HolE", 130, 9), ("DistMult", 300, 10), ("ComplEx", 175, 11), ("DistMult", 384, 12), ("HolE", 196, 13)])
@pytest.mark.parametrize("family", ["gaussian", "large"])
def test_kernel_r_across_its_hand_over_boundary(gpu_lib, model, k, slabs, family):
    """rank_screen_kernel_r counts its masks and hands its undecided marks over SCRR_UB = 16 tiles at a time (kge_rank_screen_r.h);
    at the other shapes of this suite the schedule gives a block 2 - 4 tiles, so the boundary and the tail behind it are never reached.

    n = 160, N = 33 250 -- derivation against run_screen's schedule(sr, 256, 1.0, SCRR_TMCAP, ...): qtiles = 2, so qt8 = 8 and one
    round of 256 co-resident blocks holds 32 entity splits; etiles = ceil(33 250 / 64) = 520, the last tile holds 34 rows; the run
    length tp <= 64 (AMDKGE_SCREEN_RUN's default) costs ceil(8 ceil(520 / tp) / 256) x (tp + 1):
        one round needs ceil(520 / tp) <= 32, i.e. tp >= 17:   tp = 17 -> 31 splits, 248 blocks, cost 18   (tp = 18: 19, ...)
        two rounds  need ceil(520 / tp) <= 64, i.e. tp >= 9:    tp = 9  -> 2 x 10 = 20
        three: tp = 6 -> 3 x 7 = 21;   four: tp = 5 -> 24;   tp = 4, 3, 2, 1 -> 25, 24, 27, 34;   tp = 16 -> 33 splits, two rounds: 34
    so every block but the last runs 17 tiles -- one full batch of 16, then a tail of one -- and the last one 10 tiles, the final one
    partial.  The library exposes no run length: _screen_r_run restates the schedule, and a change to it must prompt a revisit."""
    n, N, R = 160, 33250, 7
    assert _screen_r_run(n, N) == 17 and N % 64 != 0
    rng = np.random.default_rng(77 + k)
    ent, rel, X = _contraction_tables(model, k, N, R, n, family, rng)
    eng = _engine(model, k, ent, rel)
    assert _slabs(eng.Ks) == slabs
    Xd = torch.as_tensor(X).cuda()
    for nm, side in SIDES:
        ref, ctx = RO.side_counts(model, nm, ent, rel, X, R)
        assert len(np.unique(ref[:, 0])) > n // 2, nm
        if family == "large":
            _assert_every_ulp_shows(ctx, nm)
        got, st = _counts(eng, gpu_lib, Xd, side, 0)
        assert np.array_equal(got, ref), (nm, "rows off", int((got != ref).any(1).sum()), st)
        assert st is not None and not st[1] and st[0] > 0, (nm, st)
        _assert_kernel_r_kept_the_call(st, slabs, N, nm)


# (model, k): TransE walks U = k rounded up to 4 units, RotatE's exact mode the k live ones; the early exit needs U >= 64
DISTANCE_WIDTHS = [("TransE", 37), ("TransE", 50), ("TransE", 60), ("TransE", 64), ("TransE", 101), ("TransE", 200),
                   ("RotatE", 50), ("RotatE", 63), ("RotatE", 64), ("RotatE", 101), ("RotatE", 200)]


def _early_applies(model, k):
    return (k if model == "RotatE" else (k + 3) // 4 * 4) >= 64


@pytest.mark.parametrize("kind", ["gaussian", "trained", "ties"])
@pytest.mark.parametrize("model,k", DISTANCE_WIDTHS)
def test_distance_counts_equal_the_ordered_oracle(gpu_lib, model, k, kind):
    """The plain tile kernel (1: rank_count_kernel / rank_rot_kernel) and the default path with the early-exit kernel forced, each
    against RO.side_counts; on tables whose positives score near the top the exit must really have fired."""
    N, n, R = N_BASE - N_QUERIES, N_QUERIES, N_RELS   # (_tables appends one planted row per query: 3 001 candidates)
    rng = np.random.default_rng(1000 * k + len(model))
    ent, rel, X = distance_tables(model, k, N, R, n, kind, rng)
    eng = _engine(model, k, ent, rel)
    Xd = torch.as_tensor(X).cuda()
    with _early_kernel_always(gpu_lib):
        for nm, side in SIDES:
            ref, _ = RO.side_counts(model, nm, ent, rel, X, R)
            if kind == "gaussian":
                assert len(np.unique(ref[:, 0])) > n // 2, (nm, len(np.unique(ref[:, 0])))
            plain, _ = _counts(eng, gpu_lib, Xd, side, 1)
            assert np.array_equal(plain, ref), (nm, "plain kernel, rows off", int((plain != ref).any(1).sum()))
            early, st = _counts(eng, gpu_lib, Xd, side, 0)
            assert np.array_equal(early, ref), (nm, "default path, rows off", int((early != ref).any(1).sum()), st)
            if _early_applies(model, k):
                assert st is not None and not st[1], (nm, st)
                if kind == "trained":
                    assert st[2] > 0, (nm, st)   # tiles ended early: the exit was under test


# three contraction widths (kernel r, kernel v1, scalar loads) and one of each distance model
SUBSET_CASES = [("DistMult", 200, True), ("ComplEx", 300, True), ("DistMult", 50, False), ("TransE", 101, True), ("RotatE", 101, True)]


def _case_tables(model, k, rng):
    if model in ("TransE", "RotatE"):
        return distance_tables(model, k, N_BASE - N_QUERIES, N_RELS, N_QUERIES, "trained", rng)
    return _contraction_tables(model, k, N_BASE, N_RELS, N_QUERIES, "large", rng)   # (the family in which every ulp shows)


@pytest.mark.parametrize("model,k,pad", SUBSET_CASES)
def test_candidate_lists_and_ranges_equal_the_ordered_oracle(gpu_lib, model, k, pad):
    """ent_ids (a permuted id list), ent_lo / ent_hi ranges that start inside a tile, and both: counts of the default path and of the
    VALU tile kernel against RO.side_counts over the same candidate rows."""
    rng = np.random.default_rng(31 + k)
    ent, rel, X = _case_tables(model, k, rng)
    eng = _engine(model, k, ent, rel, pad)
    M, R = ent.shape[0], rel.shape[0]
    Xd = torch.as_tensor(X).cuda()
    ids = rng.permutation(M)[:2000].astype(np.int32)
    ids_d = torch.as_tensor(ids).cuda()
    cases = ((dict(ent_ids=ids_d), ids), (dict(ent_lo=1000, ent_hi=2900), np.arange(1000, 2900, dtype=np.int32)),
             (dict(ent_ids=ids_d, ent_lo=130, ent_hi=1777), ids[130:1777]))
    with _early_kernel_always(gpu_lib):
        for kw, cand in cases:
            for nm, side in SIDES:
                ref, _ = RO.side_counts(model, nm, ent, rel, X, R, ent_ids=cand)
                for which in (1, 0):
                    got, st = _counts(eng, gpu_lib, Xd, side, which, **kw)
                    assert np.array_equal(got, ref), (sorted(kw), nm, "kernel", which, "rows off", int((got != ref).any(1).sum()), st)
                    if which == 0 and pad:
                        assert st is not None and not st[1], (sorted(kw), nm, st)
                        assert model in ("TransE", "RotatE") or st[0] > 0, (sorted(kw), nm, st)


@pytest.mark.parametrize("model,k,pad", SUBSET_CASES)
def test_filtered_ranks_equal_the_ordered_oracle(gpu_lib, model, k, pad):
    """Filtered ranks of the default path -- three tie strategies x four corrupt_side forms, entities_subset, and both sides in
    flight through rank_sides (the route the drop-in evaluate() takes) -- against RO.evaluate_ranks."""
    from ampligraph_amd import _ffi
    from test_gpu_kernels import csr_filters

    rng = np.random.default_rng(53 + k)
    ent, rel, X = _case_tables(model, k, rng)
    eng = _engine(model, k, ent, rel, pad)
    M, R, n = ent.shape[0], rel.shape[0], X.shape[0]
    other = np.stack([rng.integers(0, M, 20000), rng.integers(0, R, 20000), rng.integers(0, M, 20000)], 1).astype(np.int32)
    other[:6000, 1:] = X[rng.integers(0, n, 6000), 1:]    # several true subjects / objects per test (p, o) / (s, p) pair
    other[6000:12000, :2] = X[rng.integers(0, n, 6000), :2]
    fs, fo = O.filter_sets(X, [X, other])
    assert sum(len(f) for f in fs) > 4 * n and sum(len(f) for f in fo) > 4 * n
    with _early_kernel_always(gpu_lib):
        for strat in ("worst", "best", "middle"):
            for cs in ("s", "o", "s,o", "s+o"):
                ref = RO.evaluate_ranks(model, ent, rel, X, fs, fo, cs, strat, max_rel_size=R)
                assert np.array_equal(gpu_ranks(eng, X, cs, strat, fs, fo), ref), (strat, cs)
        subset = rng.permutation(M)[:1500]
        ref = RO.evaluate_ranks(model, ent, rel, X, fs, fo, "s,o", "worst", entities_subset=subset, max_rel_size=R)
        assert np.array_equal(gpu_ranks(eng, X, "s,o", "worst", fs, fo, subset=subset), ref), "entities_subset"
        # both sides at once, each on a stream and with workspaces of its own, writing the columns of one rank matrix
        Xd = torch.as_tensor(X).cuda()
        ranks = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
        eng.rank_sides(Xd, [(_ffi.SIDE_S, csr_filters(fs, n), ranks[:, 0], 2), (_ffi.SIDE_O, csr_filters(fo, n), ranks[:, 1], 2)], "middle")
        torch.cuda.synchronize()
        assert {1, 3} <= set(eng._fstreams), sorted(eng._fstreams)   # the sides ran on lanes of their own, not one after the other
        ref = RO.evaluate_ranks(model, ent, rel, X, fs, fo, "s,o", "middle", max_rel_size=R)
        assert np.array_equal(ranks.cpu().numpy(), ref), "rank_sides"
        st = eng.screen_stats()
        if pad:
            assert st is not None and not st[1], st
