"""The int8 screening pass of evaluate() (kge_rank_screen.hip, kge_rank_screen.h): counts bit-identical to the exact fp32 kernels -- it only decides
WHICH comparisons need the exact chain.  Against the unscreened pipelined MFMA kernel (amdkge_set_rank_kernel(3)), on real-valued
tables, tables with wild dynamic range, ties, inf / NaN rows, candidate subsets and ranges; and the recheck statistics (a fraction
of a per cent of the comparisons).  That anchor, and the screened pass itself, are held bit for bit to the declared-order oracle
in test_gpu_rank_widths_oracle -- every slab count 1 .. 14, 19, 22 and 64 (all ten rank_screen_kernel_r instantiations, from a
one-plane and a two-halves model; rank_screen_kernel_v1 elsewhere), padded halves, unit counts that are no multiple of 4, kernel
r's 16-tile hand-over boundary, on the "gaussian" and "ties" families -- and at full size in test_gpu_fullsize (13- and 22-slab
rows).  The wild and non-finite families stay here: the oracle's semantics on inf / NaN are pinned by nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _counts(eng, gpu_lib, Xd, side, which, **kw):
    from ampligraph_amd import _ffi

    try:
        _ffi.check(gpu_lib.amdkge_set_rank_kernel(which))
        _, counts, _ = eng.rank_side(Xd, side, "worst", **kw)
        stats = eng.screen_stats()
        return counts.cpu().numpy().copy(), stats
    finally:
        gpu_lib.amdkge_set_rank_kernel(0)


@pytest.mark.parametrize("model,k,N,n", [("ComplEx", 200, 14505, 2000), ("DistMult", 400, 9000, 1500), ("HolE", 350, 3000, 700),
                                          ("DistMult", 50, 5000, 300), ("ComplEx", 1000, 2000, 256), ("ComplEx", 16, 700, 130),
                                          # (7- and 10-slab rows: the narrower instantiations of rank_screen_kernel_r, several slice steps per slot)
                                          ("DistMult", 200, 14505, 2000), ("ComplEx", 100, 6000, 1500), ("ComplEx", 150, 9000, 1100), ("DistMult", 300, 4100, 600),
                                          ("DistMult", 100, 8000, 900), ("ComplEx", 50, 5000, 700), ("DistMult", 128, 3000, 500),
                                          ("ComplEx", 128, 7000, 1200), ("DistMult", 256, 5000, 800),
                                          # (5, 6, 9, 11, 12 slabs; DistMult k = 350 is the reference's published width)
                                          ("ComplEx", 80, 4000, 600), ("DistMult", 192, 6000, 700), ("ComplEx", 144, 5000, 500), ("DistMult", 350, 9000, 1000), ("ComplEx", 192, 3000, 600)])
@pytest.mark.parametrize("tables", ["gaussian", "wild", "ties"])
def test_screened_counts_equal_exact_counts(gpu_lib, model, k, N, n, tables):
    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    R = 11
    rng = np.random.default_rng(k + N)
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    K = eng.K
    if tables == "gaussian":
        ent = (rng.normal(size=(N, K)) * 0.25).astype(np.float32)
        rel = (rng.normal(size=(R, K)) * 0.25).astype(np.float32)
    elif tables == "wild":   # rows 12 orders of magnitude apart, units 6 orders apart inside a row, exact zeros, one huge unit
        ent = (rng.normal(size=(N, K)) * np.exp(rng.uniform(-14, 14, size=(N, 1))) * np.exp(rng.uniform(-7, 7, size=(N, K)))).astype(np.float32)
        ent[rng.random((N, K)) < 0.1] = 0.0
        ent[5, 3] = 3e18
        rel = (rng.normal(size=(R, K)) * np.exp(rng.uniform(-3, 3, size=(R, K)))).astype(np.float32)
    else:                    # many exactly equal scores: small integers / 8
        ent = (rng.integers(-4, 5, size=(N, K)) / 8.0).astype(np.float32)
        rel = (rng.integers(-2, 3, size=(R, K)) / 4.0).astype(np.float32)
    eng.set_tables(ent, rel)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    Xd = torch.as_tensor(X).cuda()
    for side in (_ffi.SIDE_S, _ffi.SIDE_O):
        exact, st0 = _counts(eng, gpu_lib, Xd, side, 3)
        scr, st = _counts(eng, gpu_lib, Xd, side, 0)
        assert np.array_equal(scr, exact), (side, int((scr != exact).sum()), st)
        assert st is not None and not st[1]
        if tables == "gaussian" and k >= 50:
            assert st[0] < 0.02 * n * N, st    # the recheck list is a small fraction of the comparisons
    print("rechecked pairs", model, k, tables, st, "of", n * N)


# (k = 64: 4-slab rows; ComplEx k = 200 / DistMult k = 400 / HolE k = 196: 13-slab rows, DistMult k = 200: 7, ComplEx k = 150: 10 -- round 6's rank_screen_kernel_r with
# its tile-wide candidate scales -- partial last tiles, ranges that do not start on a tile, id lists, non-finite / denormal / zero rows)
@pytest.mark.parametrize("model,k", [("ComplEx", 64), ("ComplEx", 200), ("DistMult", 400), ("HolE", 196), ("DistMult", 200), ("ComplEx", 150), ("DistMult", 350), ("ComplEx", 80)])
def test_screened_counts_subsets_ranges_and_bad_rows(gpu_lib, model, k):
    """entities_subset (candidate id list), a candidate range (row-sharded evaluation) and rows holding inf / NaN / denormals."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    N, R, n = 6000, 5, 600
    rng = np.random.default_rng(3)
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    ent = (rng.normal(size=(N, eng.K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, eng.K)) * 0.3).astype(np.float32)
    ent[17, 5] = np.inf
    ent[99, :] = np.nan
    ent[200, :] = 1e-42      # denormal row
    ent[201, :] = 0.0
    eng.set_tables(ent, rel)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    X[:4, 0] = [17, 99, 200, 201]
    Xd = torch.as_tensor(X).cuda()
    ids = torch.as_tensor(rng.permutation(N)[:3000].astype(np.int32)).cuda()
    for kw in (dict(), dict(ent_ids=ids), dict(ent_lo=1000, ent_hi=5200), dict(ent_ids=ids, ent_lo=128, ent_hi=2900), dict(ent_lo=17, ent_hi=18),
               dict(ent_lo=5937, ent_hi=6000)):
        for side in (_ffi.SIDE_S, _ffi.SIDE_O):
            exact, _ = _counts(eng, gpu_lib, Xd, side, 3, **kw)
            scr, st = _counts(eng, gpu_lib, Xd, side, 0, **kw)
            assert np.array_equal(scr, exact), (kw.keys(), side, int((scr != exact).sum()), st)


def test_screened_counts_few_far_rows_stay_on_the_tile_scale_path(gpu_lib):
    """Fewer than 1 / 64 of the rows lie orders of magnitude below their tile's scale: rank_screen_kernel_r keeps the call (no fall-back
    to per-row scales), their outputs go to the exact recheck -- counts equal, list not overflowed."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    N, R, k, n = 9000, 5, 200, 700
    rng = np.random.default_rng(11)
    eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
    ent = (rng.normal(size=(N, eng.K)) * 0.25).astype(np.float32)
    rel = (rng.normal(size=(R, eng.K)) * 0.25).astype(np.float32)
    far = rng.permutation(N)[:100]                       # 100 of 9 000 rows < 1 / 64
    ent[far] *= np.exp(rng.uniform(-20, -6, size=(100, 1))).astype(np.float32)
    ent[far[:5]] *= np.float32(1e6)                      # ... and a few far ABOVE their neighbours (they set their tile's scale)
    eng.set_tables(ent, rel)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    X[:100, 2] = far                                      # positives among them too
    Xd = torch.as_tensor(X).cuda()
    for side in (_ffi.SIDE_S, _ffi.SIDE_O):
        exact, _ = _counts(eng, gpu_lib, Xd, side, 3)
        scr, st = _counts(eng, gpu_lib, Xd, side, 0)
        assert np.array_equal(scr, exact), (side, int((scr != exact).sum()), st)
        assert st is not None and not st[1], st


def test_screened_overflowing_recheck_list_falls_back(gpu_lib):
    """A recheck list too small for the call's undecided pairs (a deliberately tiny workspace through the C ABI): the device-side
    flag sends the whole call to the guarded exact kernel -- same counts, no host round trip."""
    import ctypes as C

    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine, _ptr, _stream

    N, R, k, n = 14505, 7, 200, 2048
    rng = np.random.default_rng(5)
    eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
    eng.set_tables((rng.normal(size=(N, eng.K)) * 0.25).astype(np.float32), (rng.normal(size=(R, eng.K)) * 0.25).astype(np.float32))
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    Xd = torch.as_tensor(X).cuda()
    exact, _ = _counts(eng, gpu_lib, Xd, _ffi.SIDE_O, 3)
    full, st = _counts(eng, gpu_lib, Xd, _ffi.SIDE_O, 0)
    assert np.array_equal(full, exact) and not st[1] and st[0] > 12000
    need = int(gpu_lib.amdkge_rank_screen_workspace_bytes(C.byref(eng.model), n, N))
    small = need - (max(1 << 20, n * N // 32) - 8200) * 8          # room for 8 200 pairs only
    buf = torch.empty(small, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    work = eng._workspace(n)
    _ffi.check(gpu_lib.amdkge_rank_counts_screened(C.byref(eng.model), _ptr(eng.ent), _ptr(eng.rel), _ptr(Xd), n, _ffi.SIDE_O, None, 0, N,
                                                   _ptr(counts), _ptr(work), _ptr(buf), small, _stream()))
    torch.cuda.synchronize()
    flag = buf[:8].view(torch.int32).cpu().numpy()
    assert flag[1] != 0 and flag[0] > 8200
    assert np.array_equal(counts.cpu().numpy(), exact)


@pytest.mark.parametrize("model,k,undecided", [("ComplEx", 200, 52503), ("DistMult", 200, 29446), ("ComplEx", 150, 39257)])
def test_screened_pass_is_repeatable_down_to_its_recheck_list(gpu_lib, model, k, undecided):
    """The screening kernels issue their matrix instructions as inline assembly; round 6 met two rearrangements of rank_screen_kernel_r in
    which a matrix instruction read a register a VALU copy had written fewer than two wait states before (tests/test_build_hazards.py):
    one of them produced the RIGHT ranks on this very input and a recheck list that differed from run to run (~1 % of one entity block's
    marks) -- the equality of the counts with the exact kernel does not see that.  Same call five times: the same number of undecided
    pairs, the same counts; and the count of undecided pairs is the shipped kernel's (a hazard moves it, a legitimate change of the
    bound would too: then update the figures)."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    N, R, n = 14505, 237, 4096
    rng = np.random.default_rng(0)
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    eng.set_tables((rng.normal(size=(N, eng.K)) * 0.25).astype(np.float32), (rng.normal(size=(R, eng.K)) * 0.25).astype(np.float32))
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    Xd = torch.as_tensor(X).cuda()
    exact, _ = _counts(eng, gpu_lib, Xd, _ffi.SIDE_S, 3)
    seen = []
    for _ in range(5):
        scr, st = _counts(eng, gpu_lib, Xd, _ffi.SIDE_S, 0)
        assert np.array_equal(scr, exact) and st is not None and not st[1], st
        seen.append(st[0])
    assert len(set(seen)) == 1, seen
    assert seen[0] == undecided, (seen[0], undecided)   # (profiles/r06y*: the shipped rank_screen_kernel_r<13 / 7 / 10> on this input)
