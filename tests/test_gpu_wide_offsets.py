"""Every table-indexed entry point beyond 2^31 elements, and every score block beyond 2^31 elements of stride.

One GPU's C5 shard is 6.25 M rows x 2 000 floats: every row offset has to be 64-bit.  test_gpu_fullsize::test_table_beyond_2_31_elements
holds four calls to that on one wide table; the guard-band suite rules the class out by its own words (tests/guarded.py: a wrong 64-bit
offset is out of its reach).  Here the calls merged since meet two tables whose every row the host knows (tests/wide_tables.py: row
i = base[i % 4 099]):

  wide    1 151 819 rows x 2 000 floats   DistMult k = 2 000, RotatE k = 1 000
  narrow  5 500 858 rows x   400 floats   DistMult / TransE k = 400, ComplEx / HolE k = 200  (the C2 / C3 widths: rank_screen_kernel_r,
                                          the staged persistent forward kernel, the LDS tile kernels)

and three techniques:

  * WINDOW: a call addressed by row ids gets ids inside a window of <= 4 096 consecutive rows -- T (the last rows), S (straddling element
    offset 2^31), B (read-only calls: straddling byte offset 2^32) -- and the feature's own reference runs on the window's compact copy
    with the ids shifted.  Whatever a call writes into a table-shaped buffer is checked over ALL rows: rows outside the touched set
    keep their bits, one inside moved.
  * MULTIPLICITY: a call that sweeps the table sees every base row c = N / 4 099 times: counts are c times the counts over `base`.
  * STRIDE: a (vals, n, m, ld) score block with ld = 2^26 + 64: rows 32 and up start beyond element 2^31.

No tolerance is new: a case is exact or names the feature test whose bar it uses.  No case keeps both tables alive.

Entry points without a case, and why:
  * train_shared_masked_fwdbwd / train_shared_dist_fwdbwd with the IDENTITY list: it is the promise ids[g][j] == j over M = n_ents negatives
    per group -- M = N is not a test-sized step; the GIVEN form runs the same kernels.
  * join_nearest / join_radius / dbscan: quadratic in n.  Their row staging (join_stage) is the KMeans assignment's, covered by
    test_kmeans_assign_whole_table.
  * topk_rows / topk_rows_excluding with m beyond 2^31 - 1 columns: refused (their column indices are int32),
    tests/test_complete_host.py::test_topk_rows_refuse_columns_beyond_int32.
  * cols_partial_scores on a DistMult slice of 400 units: refused by design (a slice holds up to 256 units per half),
    tests/test_api_surface.py::test_session_group_argument_validation_without_gpu; the ComplEx slice of 2 x 200 units has the case.
  * relation_topk, corruption_select, query_topn*: engine wrappers over calls that have a case each (relation_scores / corruption_scores
    into topk_rows_excluding / discover_select), covered through _corruption_topk_case and section 4.

Which kernel served a call is asserted where the library reports it (the screening pass's and the early exit's statistics words); the
tile-direct pass, the hot-row replicas and the persistent forward kernel report nothing, see _tiled_case.

Peak device memory of the module: 37.3 GB (table + gradient + two Adam slots of either geometry, and the chunked checks' temporaries);
test_table_beyond_2_31_elements, whose whole-buffer `.abs()` adds a fifth buffer of the table's size, peaks at 46.1 GB.
"""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import torch

import shared_mask_ref as MR
import shared_ref as SR
import wide_tables as WT
from oracle import kge_oracle as O
from oracle import rank_ordered as RO
from test_gpu_complete import ID_BASE, _blocks, _csr, _order, _reference, _same
from test_gpu_discover import csr as select_csr
from test_gpu_discover import make_block, pair_keys, select_numpy
from test_gpu_kernels import assert_grads_close, dev, loss_desc
from test_gpu_rank_early import _counts as rank_counts_with_stats
from test_gpu_rank_widths_oracle import _assert_kernel_r_kept_the_call, _early_kernel_always
from test_gpu_relation import bits, numpy_counts
from test_gpu_shared import check_against_oracle
from test_gpu_shared_dist import assert_conditioned, check_against_ref
from test_gpu_shared_mask import check_against_masked_step, filters
from wide_tables import M, NARROW, P, WIDE

pytestmark = pytest.mark.gpu

LD = 2 ** 26 + 64      # the stride of section 4's score blocks
N_BLOCK = 40           # their rows: 32 .. 39 start beyond element 2^31 - 1
assert 32 * LD >= 2 ** 31


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module", autouse=True)
def _module_budget(gpu_lib):
    """Peak device memory and wall time of the module, printed at teardown (run with -s): the module must stay at or below the
    37 GB of test_table_beyond_2_31_elements (table + gradient + two Adam slots)."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    WT.release_all()
    peak = torch.cuda.max_memory_allocated()
    print(f"\n[wide offsets] peak device memory {peak / 1e9:.2f} GB ({peak / 2 ** 30:.2f} GiB), module wall time {time.time() - t0:.1f} s")
    assert peak <= 37.5e9, peak


@pytest.fixture(scope="module")
def wide(gpu_lib):
    yield WIDE
    WIDE.release()


@pytest.fixture(scope="module")
def narrow(gpu_lib):
    """(Allocated only once the wide table is gone: Geometry.engine releases whatever other geometry is alive.)"""
    yield NARROW
    NARROW.release()


def _window_got(geo, eng, lo, L, ps, ns):
    """the (loss, dense entity gradient of the window, relation gradient, scores) tuple the feature tests' checkers take"""
    torch.cuda.synchronize()
    return L, eng.g_ent[lo:lo + M].cpu().numpy(), eng.g_rel.cpu().numpy(), ps.cpu().numpy(), ns.cpu().numpy()


def _assert_gradient_only_in(geo, eng, ids, what):
    geo.assert_only(geo.rows_nonzero(eng.g_ent), ids, what)


WINDOWS = ("T", "S")


def _lo(geo, name):
    return getattr(geo, name)


# ====================================================================================================== 4. wide score blocks
@pytest.fixture
def block(gpu_lib):
    """fp32 [N_BLOCK, LD]: 10.7 GB of which a case writes the first m columns of each row; it lives for one case."""
    WT.release_all()
    blk = torch.empty(N_BLOCK * LD, dtype=torch.float32, device="cuda").view(N_BLOCK, LD)
    yield blk
    del blk
    torch.cuda.empty_cache()


def _put(block, V):
    n, m = V.shape
    block[:n, :m] = dev(V)
    return block


def test_stride_topk_rows(gpu_lib, block):
    """amdkge_topk_rows on the strided block == test_gpu_complete._reference (the documented order: best first, equal values by
    increasing column) on the same values held contiguously; exact.  k = 1 and 1 024, largest and smallest, and a payload of the
    same stride."""
    n, m = N_BLOCK, 5003
    V = _blocks(n, m, 7)["ties"]
    _put(block, V)
    pay_host = (np.random.default_rng(3).permutation(n * m).reshape(n, m) % 1_000_003).astype(np.int32)
    payload = torch.empty(n * LD, dtype=torch.int32, device="cuda").view(n, LD)
    payload[:, :m] = dev(pay_host)
    col = np.arange(m, dtype=np.int32)
    for k in (1, 1024):
        for largest in (1, 0):
            ri, rv = _reference(V if largest else -V, k, col, None, None)
            rv = rv if largest else -rv
            for pl in (None, payload):
                idx = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
                val = torch.full((n, k), -7.0, dtype=torch.float32, device="cuda")
                assert gpu_lib.amdkge_topk_rows(_p(block), n, m, LD, None, None, _p(pl), k, largest, _p(idx), _p(val), None) == 0
                want_i = ri if pl is None else np.take_along_axis(pay_host, ri, 1)
                _same(idx.cpu().numpy(), val.cpu().numpy(), want_i, rv, ("topk_rows", k, largest, pl is not None))
    del payload


def test_stride_topk_rows_excluding(gpu_lib, block):
    """amdkge_topk_rows_excluding on the strided block against test_gpu_complete._reference: ranges, d_own, and a row beyond 2^31 whose
    every column is excluded; exact."""
    n, m, k = N_BLOCK, 5003, 100
    rng = np.random.default_rng(11)
    V = _blocks(n, m, 8)["ties"]
    _put(block, V)
    col_id = ID_BASE + np.arange(m, dtype=np.int32)
    best = [_order(V[i]) for i in range(n)]
    ex = [col_id[best[i][:50]] for i in range(n)]
    ex[35] = col_id.copy()                                                 # every column of a row that starts beyond 2^31
    own = np.array([col_id[best[i][50]] for i in range(n)], dtype=np.int32)   # the best column the range leaves
    for use_own in (False, True):
        idx = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
        val = torch.full((n, k), -7.0, dtype=torch.float32, device="cuda")
        lo, hi, ids = _csr(ex, rng)
        assert gpu_lib.amdkge_topk_rows_excluding(_p(block), n, m, LD, None, ID_BASE, _p(lo), _p(hi), _p(ids), _p(dev(own)) if use_own else None, k,
                                                  _p(idx), _p(val), None) == 0
        ri, rv = _reference(V, k, col_id, ex, own if use_own else None)
        _same(idx.cpu().numpy(), val.cpu().numpy(), ri, rv, ("excluding", use_own))
        assert (ri[35] == -1).all()


@pytest.mark.parametrize("n,m,R", [(N_BLOCK, 5003, 19),          # the LDS bitmap of the filter ids
                                   (36, 1_100_000, 59)])         # beyond the bitmap: binary search in the id list (as test_gpu_discover's last shape)
def test_stride_discover_select(gpu_lib, block, n, m, R):
    """amdkge_discover_select on the strided block against test_gpu_discover.select_numpy, for both thr_given values; the pair list as a
    set, the thresholds exact."""
    from ampligraph_amd import _ffi

    assert (n - 1) * LD >= 2 ** 31
    # make_block's four kinds of row (empty, partial, partial, full filter range; a NaN in row 1), repeated down the block: the reference
    # runs on the four rows once and row r expects what row r % 4 does
    V4, own4, flt4 = make_block(4, m, 1000 * R + m % 997)
    want4, thr4 = select_numpy(V4, own4, flt4, R, 1)
    assert len(want4) > 0 and len(np.unique(thr4)) > 2
    rep = np.arange(n) % 4
    own, flt, want_thr = own4[rep], [flt4[j] for j in rep], thr4[rep]
    for i in range(0, n, 4):
        block[i:i + 4, :m] = dev(V4[:n - i])
    want = np.sort(np.concatenate([want4[want4 // m == r % 4] % m + r * m for r in range(n)]))
    queries = np.zeros((n, 3), dtype=np.int32)
    queries[:, 0] = own                                                   # SIDE_O: the row's own entity is the subject
    queries[:, 2] = (own + 1) % m
    lo, hi, ids = select_csr(flt)
    qd = dev(queries)
    for given in (0, 1):
        thr = dev(want_thr.astype(np.int32)) if given else torch.full((n,), 5, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        pairs = torch.full((len(want) + 64, 2), -7, dtype=torch.int32, device="cuda")
        _ffi.check(gpu_lib.amdkge_discover_select(_p(block), n, m, LD, _p(qd), _ffi.SIDE_O, _p(lo), _p(hi), _p(ids), R, 1, _p(thr), given, 0, _p(pairs),
                                                  int(pairs.shape[0]), _p(count), None))
        torch.cuda.synchronize()
        assert int(count.item()) == len(want), (given, int(count.item()), len(want))
        assert np.array_equal(pair_keys(pairs[:len(want)], m), want), given
        assert np.array_equal(thr.cpu().numpy().astype(np.int64), want_thr), given


def test_stride_relation_rank_counts(gpu_lib, block):
    """amdkge_relation_rank_counts on the strided block against test_gpu_relation.numpy_counts, with a filter, a column id list that
    repeats an id, and subset_pos; exact."""
    from ampligraph_amd.engine import subset_positions

    n, m, n_rels = N_BLOCK, 5003, 6000
    rng = np.random.default_rng(13)
    V = (rng.integers(-40, 41, size=(n, m)) / 8.0).astype(np.float32)       # many equal quantised scores
    _put(block, V)
    pos = V[np.arange(n), rng.integers(0, m, n)].copy()
    col_ids = rng.permutation(n_rels)[:m].astype(np.int32)
    col_ids[17] = col_ids[3]                                                # a repeated id: its last column is the one that counts
    spos = subset_positions(col_ids, n_rels, "cuda")
    col_of = {int(r): j for j, r in enumerate(col_ids.tolist())}
    known = [np.unique(rng.choice(n_rels, 300, replace=False)).astype(np.int32) for _ in range(n)]
    known[33] = np.unique(np.concatenate([known[33], col_ids[[3, 17]]])).astype(np.int32)
    kc = [[col_of[int(r)] for r in ks if int(r) in col_of] for ks in known]
    gt, eq, sub = numpy_counts(V, pos, kc)
    assert sub.max() > 0 and (eq > 1).any()
    lo, hi, ids = (dev(a) for a in MR.csr(known))
    counts = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    dsub = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert gpu_lib.amdkge_relation_rank_counts(_p(block), n, m, LD, _p(dev(pos)), _p(dev(col_ids)), 0, _p(lo), _p(hi), _p(ids), _p(spos), _p(counts),
                                               _p(dsub), None) == 0
    assert np.array_equal(counts.cpu().numpy(), np.stack([gt, eq], 1)) and np.array_equal(dsub.cpu().numpy(), sub)


def test_stride_corruption_scores(gpu_lib, block, narrow):
    """amdkge_corruption_scores writing into the strided block (narrow DistMult, candidates = window T) == the contiguous call, bit for
    bit; sampled unwritten positions of every row keep their fill.  (The block and the narrow table together: 19.5 GB.)"""
    from ampligraph_amd import _ffi

    geo = narrow
    eng = geo.engine("DistMult", 400)
    geo.fill("gaussian")
    n = N_BLOCK
    X = geo.spread_triples(np.random.default_rng(17), n)
    Xd = dev(X)
    sentinel = -12345.5
    block.fill_(sentinel)
    work = eng._workspace(n)
    for side in (_ffi.SIDE_S, _ffi.SIDE_O):
        tight = torch.empty(n, M, dtype=torch.float32, device="cuda")
        for out, ld in ((tight, M), (block, LD)):
            _ffi.check(gpu_lib.amdkge_corruption_scores(C.byref(eng.model), _p(eng.ent), _p(eng.rel), _p(Xd), n, side, None, geo.T, geo.N, _p(out), ld,
                                                        _p(work), None))
        assert torch.equal(block[:n, :M].view(torch.int32), tight.view(torch.int32)), side
        assert len(np.unique(tight.cpu().numpy())) > n * M // 2
    probe = torch.as_tensor([M, M + 1, LD // 2, LD - 1], device="cuda")
    assert bool((block[:, probe] == sentinel).all())


# ====================================================================================================== opt_step_merged: a wide part stride
def test_opt_step_merged_part_stride_beyond_2_30(gpu_lib):
    """amdkge_opt_step_merged with n_parts = 3 and part_stride = 2^30 + 64 floats over 4 096 elements: part 2 starts at element 2^31 + 128.
    The parts buffer is 8.6 GB (up to the end of part 2) of mostly untouched memory.  Reference and bars: test_gpu_shard_kernels::test_opt_step_merged_equals_sum_then_sweep
    (Adam: 3e-6 on the parameters, rtol 3e-5 / atol 3e-7 max on the slots)."""
    from ampligraph_amd import _ffi

    WT.release_all()
    n, W, stride = 4096, 3, 2 ** 30 + 64
    assert (W - 1) * stride > 2 ** 31 - 1
    rng = np.random.default_rng(3)
    x0 = (rng.normal(size=(1, n)) * 0.5).astype(np.float32)
    parts_h = (rng.normal(size=(W, n)) * 0.1).astype(np.float32)
    parts = torch.empty((W - 1) * stride + n, dtype=torch.float32, device="cuda")
    for q in range(W):
        parts[q * stride:q * stride + n] = dev(parts_h[q])
    x = dev(x0.reshape(-1).copy())
    s0, s1 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    reg = torch.zeros(1, dtype=torch.float64, device="cuda")
    st = O.TrainState(x0.copy(), np.zeros((1, 4), np.float32), "adam", 1e-2)
    for t in (1, 2):
        opt = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, 0.0, t)
        opt.row_floats = 4
        _ffi.check(gpu_lib.amdkge_opt_step_merged(C.byref(opt), _p(x), _p(parts), W, stride, _p(s0), _p(s1), n, _p(reg), None))
        O.apply_optimizer(st, parts_h.astype(np.float64).sum(0).reshape(1, n), np.zeros((1, 4)))
        torch.cuda.synchronize()
        assert np.abs(x.cpu().numpy() - st.ent[0]).max() <= 3e-6 * max(1.0, np.abs(st.ent).max()), t
        for got, nme in ((s0, "m_e"), (s1, "v_e")):
            ref = st.slots[nme][0]
            assert np.allclose(got.cpu().numpy(), ref, rtol=3e-5, atol=3e-7 * max(np.abs(ref).max(), 1e-30)), (nme, t)
    del parts
    torch.cuda.empty_cache()


# ====================================================================================================== 2. calls addressed by row id
# ---------------------------------------------------------------------------------------------------- gather / scatter
def _gather_scatter_case(geo):
    """amdkge_gather_rows (exact: a negative id gives a zero row) and amdkge_scatter_add_rows (a repeated id adds twice, a negative id is
    skipped; dyadic addends, so the sums are exact in any order) with ids from T and S; every other row of the scattered-into buffer stays
    all-zero bits."""
    eng = geo.engine("DistMult", geo.Ks)
    geo.fill("gaussian")
    rng = np.random.default_rng(19)
    ids = np.concatenate([geo.T + rng.integers(0, M, 150), geo.S + rng.integers(0, M, 150)]).astype(np.int64)
    ids[:4] = (geo.N - 1, geo.first_high, geo.first_high - 1, geo.T)
    ids[7] = ids[5]                                                          # a repeated id
    idx = ids.astype(np.int32)
    idx[11] = -1
    assert int(idx.max()) * geo.Ks > 2 ** 31 - 1
    got = eng.gather_rows(eng.ent, dev(idx)).cpu().numpy()
    want = geo.rows(np.where(idx < 0, 0, idx))
    want[11] = 0.0
    assert np.array_equal(bits(got), bits(want))
    # scatter-add into the (zeroed) gradient buffer
    geo.training(eng, "sgd")
    src = (rng.integers(-8, 9, size=(len(idx), geo.Ks)) / 8.0).astype(np.float32)
    eng.scatter_add_rows(eng.g_ent, dev(idx), dev(src))
    torch.cuda.synchronize()
    live = idx >= 0
    uniq = np.unique(idx[live])
    ref = np.zeros((len(uniq), geo.Ks), np.float32)
    np.add.at(ref, np.searchsorted(uniq, idx[live]), src[live])
    assert np.array_equal(eng.g_ent[dev(uniq.astype(np.int64))].cpu().numpy(), ref)
    _assert_gradient_only_in(geo, eng, uniq, "scatter_add_rows")
    eng.g_flat.zero_()



# ---------------------------------------------------------------------------------------------------- pack / unpack
def test_pack_unpack_all_rows(gpu_lib, wide):
    """amdkge_pack_rows / amdkge_unpack_rows over all N rows of a PADDED layout (RotatE k = 999: halves of 999 live units stored as 1 000,
    so dense rows of 1 998 floats become stored rows of 2 000): the layout rule -- stored[h * ks + u] = dense[h * k + u], padding units zero
    -- bitwise on rows of T, S, B and row 0; unpack(pack(x)) == x on the same rows."""
    from ampligraph_amd.engine import KgeEngine

    WT.release_all()   # (the dense source, the stored table and the unpacked copy are three buffers of the wide table's size)
    geo, k = wide, 999
    N = geo.N
    small = KgeEngine("RotatE", k, 8, 2, max_rel_size=2)                    # supplies the model descriptor; the rows are ours
    assert small.ks == 1000 and small.Ks == 2000 and small.K == 1998
    rng = np.random.default_rng(23)
    base = rng.normal(size=(P, small.K)).astype(np.float32)
    base_d = dev(base)
    dense = torch.empty(N, small.K, dtype=torch.float32, device="cuda")
    for r0 in range(0, N, WT.CHUNK):
        r1 = min(N, r0 + WT.CHUNK)
        torch.index_select(base_d, 0, torch.arange(r0, r1, device="cuda") % P, out=dense[r0:r1])
    assert N * small.Ks > 2 ** 31 - 1 and dense.numel() > 2 ** 31 - 1
    stored = torch.full((N, small.Ks), 7.0, dtype=torch.float32, device="cuda")
    small.pack(dense, out=stored)
    rows = np.concatenate([[0], geo.T + np.arange(M), geo.S + np.arange(M), geo.B + np.arange(M)])[::7]
    rows = np.unique(np.concatenate([rows, [N - 1, geo.first_high, geo.first_high - 1]]))
    want = np.zeros((len(rows), 2, 1000), np.float32)
    want[:, :, :k] = base[rows % P].reshape(len(rows), 2, k)
    got = stored[dev(rows)].cpu().numpy()
    assert np.array_equal(bits(got), bits(want.reshape(len(rows), 2000)))
    back = small.unpack(stored)
    assert np.array_equal(bits(back[dev(rows)]), bits(base[rows % P]))
    del dense, stored, back
    torch.cuda.empty_cache()


def test_gather_and_scatter_add_rows_narrow(gpu_lib, narrow):
    _gather_scatter_case(narrow)


# ---------------------------------------------------------------------------------------------------- predict, relation prediction
NARROW_MODELS = [("DistMult", 400), ("ComplEx", 200), ("TransE", 400), ("HolE", 200)]


@pytest.mark.parametrize("model,k", NARROW_MODELS)
def test_score_and_relation_prediction(gpu_lib, narrow, model, k):
    """score against O.compute_scores on `base` with the ids mod P (test_gpu_kernels::test_score_parity's bar: 1e-5 of the score, floored
    at 5 % of the rms score); relation_scores == score on the materialised triples, bit for bit, and relation_rank against
    test_gpu_relation.numpy_counts on those bits (test_gpu_relation's yardsticks: exact)."""
    geo = narrow
    eng = geo.engine(model, k)
    geo.fill("gaussian")
    rng = np.random.default_rng(29)
    n = 140
    X = geo.spread_triples(rng, n)
    Xd = dev(X)
    got = eng.score(Xd).cpu().numpy()
    s, p, o = O.lookup(geo.base, geo.rel, geo.mod(X))
    ref = O.compute_scores(model, s, p, o, max_rel_size=geo.R)
    scale = np.maximum(np.abs(ref), 0.05 * np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
    assert np.max(np.abs(got - ref) / scale) < 1e-5
    # relation_scores: the bits of score() on (s_i, r_j, o_i)
    T3 = np.repeat(X, geo.R, 0)
    T3[:, 1] = np.tile(np.arange(geo.R, dtype=np.int32), n)
    block_ref = eng.score(dev(T3)).cpu().numpy().reshape(n, geo.R)
    blk = eng.relation_scores(Xd)
    assert np.array_equal(bits(blk), bits(block_ref))
    ranks, counts, _ = eng.relation_rank(Xd, "worst")
    gt, eq, _ = numpy_counts(block_ref, got, [[]] * n)
    assert np.array_equal(counts.cpu().numpy(), np.stack([gt, eq], 1)) and np.array_equal(ranks.cpu().numpy(), (gt + eq + 1).astype(np.int32))


# ---------------------------------------------------------------------------------------------------- candidate lists
def _rank_lists_case(geo, model, k, family):
    from ampligraph_amd.evaluation.candidates import as_csr

    eng = geo.engine(model, k)
    geo.fill(family)
    rng = np.random.default_rng(31)
    n = 37
    X = geo.spread_triples(rng, n)
    lens = (0, 1, 63, 64, 65, 500, 3000)
    lists = [geo.spread_ids(rng, max(lens[i % len(lens)], 3))[:lens[i % len(lens)]].astype(np.int32) for i in range(n)]
    lists[5][7] = lists[5][2]                                                # one list repeats an id: two candidates
    assert max(int(a.max()) for a in lists if len(a)) * geo.Ks > 2 ** 31 - 1
    off, ids, ml = as_csr(lists, n)
    cand = (dev(off[:-1].copy()), dev(off[1:].copy()), dev(ids), ml)
    Xm = geo.mod(X)
    for nm, side in (("s", 1), ("o", 2)):
        ref = np.zeros((n, 2), np.int32)
        for i, a in enumerate(lists):
            ref[i] = RO.side_counts(model, nm, geo.base, geo.rel, Xm[i:i + 1], geo.R, ent_ids=a % P)[0][0]
        got = eng.rank_lists(dev(X), side, cand)[1].cpu().numpy()
        assert np.array_equal(got, ref), (model, nm, np.argwhere(got != ref)[:5])
        if family == "ties":
            assert ref[:, 1].sum() > 0


@pytest.mark.parametrize("model,k,family", [("DistMult", 400, "ties"), ("TransE", 400, "gaussian")])
def test_rank_lists_narrow(gpu_lib, narrow, model, k, family):
    """rank_lists with candidate lists drawn from T, S and B against the declared-order oracle on `base` (candidate ids mod P), one triple
    at a time as test_gpu_rank_lists.oracle_counts; exact."""
    _rank_lists_case(narrow, model, k, family)


# ====================================================================================================== 3. calls that sweep the table
def _sweep_queries(geo, n=140):
    """n = 140: one full and one partial block of 128 queries, and >= 128 so that the screening pass engages"""
    return geo.spread_triples(np.random.default_rng(37), n)


@contextlib.contextmanager
def _screen_room(eng, gib):
    """rank_side hands the count pass a screening workspace only below SCREEN_MAX_BYTES (4 GiB); the narrow table's is 6.7 GiB -- its
    limb images pass 2^32 bytes, which is the point -- so the limit is raised on this engine instance for the call."""
    eng.SCREEN_MAX_BYTES = gib << 30
    try:
        yield
    finally:
        del eng.SCREEN_MAX_BYTES
        eng._bufs.pop("rank_screen", None)
        eng._last_screen = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("family", ["gaussian", "ties"])
@pytest.mark.parametrize("model,k", [("DistMult", 400), ("ComplEx", 200), ("HolE", 200)])
def test_rank_side_whole_table_contraction(gpu_lib, narrow, model, k, family):
    """rank_side over [0, N), both sides, under the VALU tile kernel (1), both fp32 MFMA kernels (2, 3) and the default path (0: the int8
    screened pass with rank_screen_kernel_r<13> + exact recheck): counts == c x RO.side_counts over `base`, exact.  Kernel 0 must have
    been the screened pass: workspace used, no fall-back, rank_screen_kernel_r kept the call (_assert_kernel_r_kept_the_call)."""
    from ampligraph_amd import _ffi

    geo = narrow
    eng = geo.engine(model, k)
    geo.fill(family)
    X = _sweep_queries(geo)
    Xd, Xm = dev(X), geo.mod(X)
    need = int(gpu_lib.amdkge_rank_screen_workspace_bytes(C.byref(eng.model), len(X), geo.N))
    assert need > 2 ** 32, need                                              # the per-candidate workspaces pass 2^32 bytes
    for nm, side in (("s", _ffi.SIDE_S), ("o", _ffi.SIDE_O)):
        ref = RO.side_counts(model, nm, geo.base, geo.rel, Xm, geo.R)[0].astype(np.int64) * geo.mult
        if family == "ties":
            assert int(ref[:, 1].sum()) > 0
        else:
            assert len(np.unique(ref[:, 0])) > len(X) // 2
        for which in (1, 2, 3, 0):
            with _screen_room(eng, 8) if which == 0 else contextlib.nullcontext():
                got, st = rank_counts_with_stats(eng, gpu_lib, Xd, side, which)
            assert np.array_equal(got, ref), (nm, "kernel", which, "rows off", int((got != ref).any(1).sum()), st)
            if which == 0:
                assert st is not None and not st[1], (nm, st)
                if family == "gaussian":
                    assert st[0] > 0, (nm, st)
                _assert_kernel_r_kept_the_call(st, 13, geo.N, nm)


def _distance_sweep(gpu_lib, geo, model, k):
    from ampligraph_amd import _ffi

    eng = geo.engine(model, k)
    geo.fill("gaussian", scale=0.3)
    X = _sweep_queries(geo)
    Xd, Xm = dev(X), geo.mod(X)
    with _early_kernel_always(gpu_lib):
        for nm, side in (("s", _ffi.SIDE_S), ("o", _ffi.SIDE_O)):
            ref = RO.side_counts(model, nm, geo.base, geo.rel, Xm, geo.R)[0].astype(np.int64) * geo.mult
            assert len(np.unique(ref[:, 0])) > len(X) // 2
            plain, _ = rank_counts_with_stats(eng, gpu_lib, Xd, side, 1)
            assert np.array_equal(plain, ref), (nm, "plain kernel, rows off", int((plain != ref).any(1).sum()))
            early, st = rank_counts_with_stats(eng, gpu_lib, Xd, side, 0)
            assert np.array_equal(early, ref), (nm, "early exit, rows off", int((early != ref).any(1).sum()), st)
            assert st is not None and not st[1], (nm, st)                    # the early-exit kernel had the call and did not fall back


def test_rank_side_whole_table_transe(gpu_lib, narrow):
    """The same for TransE: the plain tile kernel and the early exit forced (amdkge_set_rank_early(1, ..., probe = 0)), exact."""
    _distance_sweep(gpu_lib, narrow, "TransE", 400)


def test_rank_side_range_and_filter(gpu_lib, narrow):
    """rank_side over a range that starts and ends off a tile inside the upper half, with a filter whose ids lie in the range: counts ==
    RO.side_counts over the range's residues, the subtraction == RO.filter_sub with the ids mod P; exact."""
    from ampligraph_amd import _ffi
    from test_gpu_kernels import csr_filters

    geo = narrow
    eng = geo.engine("DistMult", 400)
    geo.fill("ties")
    X = _sweep_queries(geo)
    Xd, Xm = dev(X), geo.mod(X)
    lo = geo.first_high + 37
    hi = lo + 3 * P + 50                                                     # (three copies of every base row and 50 rows more)
    assert lo % 64 and (hi - lo) % 64 and lo * geo.Ks > 2 ** 31 - 1 and hi < geo.N
    rng = np.random.default_rng(41)
    cand = (np.arange(lo, hi) % P).astype(np.int32)
    for nm, side in (("s", _ffi.SIDE_S), ("o", _ffi.SIDE_O)):
        lists = [np.unique(lo + rng.integers(0, hi - lo, int(rng.integers(0, 40)))).astype(np.int32) for _ in range(len(X))]
        own = X[:, 0] if nm == "s" else X[:, 2]
        lists = [np.unique(np.append(a, own[i])).astype(np.int32) if lo <= own[i] < hi else a for i, a in enumerate(lists)]
        ref, ctx = RO.side_counts("DistMult", nm, geo.base, geo.rel, Xm, geo.R, ent_ids=cand)
        sub = RO.filter_sub(ctx, [a % P for a in lists])
        assert sub.max() > 0 and int(ref[:, 1].sum()) > 0
        ranks, counts, dsub = eng.rank_side(Xd, side, "worst", csr_filters(lists, len(X)), ent_lo=lo, ent_hi=hi)
        assert np.array_equal(counts.cpu().numpy(), ref) and np.array_equal(dsub.cpu().numpy(), sub), nm
        assert np.array_equal(ranks.cpu().numpy(), ref.sum(1) - sub + 1), nm


def _corruption_topk_case(geo, model, k):
    """Top-k corruptions over [0, N) in the engine's own chunks, and over the rows from the first one beyond 2^31 - 1 elements on.  Rows
    repeat, and equal values come back by increasing id: the k best of a query are the FIRST k copies (inside the candidate range) of
    the best base row -- for [0, N) those are low rows; the upper range is what sends high rows back.  Every returned value has the
    bits of the declared chain on base[id % P] (RO.chain_scores_numpy)."""
    from ampligraph_amd import _ffi

    eng = geo.engine(model, k)
    geo.fill("gaussian", scale=0.3)
    n, kk = 8, 10
    X = geo.spread_triples(np.random.default_rng(43), n)
    Xm = geo.mod(X)
    s, p, o = O.lookup(geo.base, geo.rel, Xm)
    for nm, side in (("s", _ffi.SIDE_S), ("o", _ffi.SIDE_O)):
        qpos, Q, mode, U, plane, scale = RO.prep(model, nm, s, p, o, geo.R)
        chain = RO.chain_scores_numpy(mode, Q, geo.base, U, plane, scale)    # [n, P]
        srt = np.sort(chain, 1)
        assert (srt[:, -1] > srt[:, -2]).all()                               # one best base row per query
        best = chain.argmax(1)
        for lo in (0, geo.first_high + 5):
            pos, val = eng.corruption_topk(dev(X), side, kk, ent_lo=lo, ent_hi=geo.N)
            ids, val = pos.cpu().numpy().astype(np.int64) + lo, val.cpu().numpy()
            assert np.array_equal(bits(val), bits(np.take_along_axis(chain, ids % P, 1))), (nm, lo)
            first = lo + ((best - lo) % P)                                   # the best row's first copy at or behind lo
            assert np.array_equal(ids, first[:, None] + P * np.arange(kk)[None, :]), (nm, lo)
            if lo:
                assert int(ids.min()) * geo.Ks > 2 ** 31 - 1


def test_corruption_topk_narrow(gpu_lib, narrow):
    _corruption_topk_case(narrow, "ComplEx", 200)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_nearest_rows(gpu_lib, narrow, metric):
    """nearest_rows (row_dots + row_sqnorms + topk_rows + pair_distances) of 20 queries that are no table rows, over [0, N), over the rows
    from the first one beyond 2^31 - 1 elements on, and over an id list drawn from T, S and B: distances against fp64 on `base`
    (test_gpu_discovery::test_nearest_rows_against_numpy's bar: rtol 1e-5, atol 1e-6)."""
    geo = narrow
    eng = geo.engine("DistMult", 400)
    geo.fill("gaussian")
    rng = np.random.default_rng(47)
    nq, kk = 20, 8
    Q = (rng.normal(size=(nq, geo.Ks)) * 0.25).astype(np.float32)
    Qd = dev(Q)
    Q64, E64 = Q.astype(np.float64), geo.base.astype(np.float64)
    if metric == "cosine":
        D = 1.0 - (Q64 @ E64.T) / np.linalg.norm(Q64, axis=1)[:, None] / np.linalg.norm(E64, axis=1)[None, :]
    else:
        D = np.sqrt(np.maximum((Q64 ** 2).sum(1)[:, None] + (E64 ** 2).sum(1)[None, :] - 2.0 * Q64 @ E64.T, 0))
    ids = np.unique(geo.spread_ids(rng, 3000)).astype(np.int32)
    cases = ((dict(), np.arange(P), geo.mult), (dict(ent_lo=geo.first_high + 5, ent_hi=geo.N), None, None), (dict(ent_ids=dev(ids)), ids % P, 1))
    order = np.argsort(D, axis=1, kind="stable")[:, :kk]                     # every base row has a copy in every candidate set below
    for kw, cand, copies in cases:
        if cand is None:     # a range of rows: base row r has cnt[r] copies in it
            lo = kw["ent_lo"]
            res, cnt = np.unique(np.arange(lo, geo.N) % P, return_counts=True)
            assert len(res) == P and cnt.min() >= 1
            to_row = lambda pos: (pos + lo) % P   # noqa: E731
        elif copies == 1:    # an id list (unique ids: some base rows several times, some not at all)
            cnt = np.bincount(cand, minlength=P)
            to_row = lambda pos: cand[pos]   # noqa: E731
        else:                # the whole table
            cnt = np.full(P, copies)
            to_row = lambda pos: pos % P   # noqa: E731
        pos, got = eng.nearest_rows(Qd, kk, metric, **kw)
        pos, got = pos.cpu().numpy().astype(np.int64), got.cpu().numpy().astype(np.float64)
        if copies == 1:
            want = np.sort(np.repeat(D, cnt, axis=1), axis=1)[:, :kk]
        else:                # the kk smallest of the multiset: the nearest base rows, each as often as it occurs
            want = np.stack([np.repeat(D[i, order[i]], cnt[order[i]])[:kk] for i in range(nq)])
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (sorted(kw), np.abs(got - want).max())
        assert np.allclose(D[np.arange(nq)[:, None], to_row(pos)], want, rtol=1e-5, atol=1e-6), sorted(kw)
        assert all(len(set(r.tolist())) == kk for r in pos)
        if "ent_lo" in kw:
            assert int((pos + kw["ent_lo"]).min()) * geo.Ks > 2 ** 31 - 1


def test_kmeans_assign_whole_table(gpu_lib, narrow):
    """kmeans_assign of all N rows (d = 400) to three centres: label[i] == label_base[i % P], the counts per centre c x the base counts.
    The base labels come from fp64 distances after asserting that no base row is within test_gpu_kmeans.BAND (relative 1e-4) of
    two centres."""
    from test_gpu_kmeans import BAND

    geo = narrow
    eng = geo.engine("DistMult", 400)
    geo.fill("gaussian")
    rng = np.random.default_rng(4)   # (the first seed, counting from 1, for which the margin below holds on `base`: found on the CPU)
    Cn = (geo.base[rng.choice(P, 3, replace=False)] + rng.normal(size=(3, geo.Ks)) * 0.05).astype(np.float32)
    d2 = ((geo.base.astype(np.float64)[:, None, :] - Cn.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    srt = np.sort(d2, 1)
    assert ((srt[:, 1] - srt[:, 0]) / srt[:, 1]).min() > BAND
    lab_base = d2.argmin(1).astype(np.int32)
    assert len(np.unique(lab_base)) == 3
    labels, mind2 = eng.kmeans_assign(eng.ent, dev(Cn))
    lab_d = dev(lab_base)
    for r0 in range(0, geo.N, WT.CHUNK):
        r1 = min(geo.N, r0 + WT.CHUNK)
        want = lab_d[torch.arange(r0, r1, device="cuda") % P]
        assert torch.equal(labels[r0:r1], want), (r0, int((labels[r0:r1] != want).sum()))
    assert np.array_equal(torch.bincount(labels.long(), minlength=3).cpu().numpy(), geo.mult * np.bincount(lab_base, minlength=3))
    # equal rows, equal distances: the fp32 value of a row is that of its first copy, bit for bit
    first = mind2[:P]
    for r0 in range(0, geo.N, WT.CHUNK):
        r1 = min(geo.N, r0 + WT.CHUNK)
        assert torch.equal(mind2[r0:r1].view(torch.int32), first[torch.arange(r0, r1, device="cuda") % P].view(torch.int32)), r0


# ====================================================================================================== 2. training in a window
def _shared_lists(geo, rng, lo, B, G, Mn, seed):
    X, Xc = geo.window_triples(rng, lo, B)
    ids_c, side = SR.sample_shared(Xc, G, Mn, seed, 4, sample_range=M)
    ids_c[0, 0] = M - 1                                                      # the window's last and first row in the first list
    ids_c[0, Mn // 2] = 0
    assert 0 < side.sum() < B
    return X, Xc, ids_c, (ids_c + lo).astype(np.int32), side


def _touched_shared(X, ids):
    return np.concatenate([X[:, 0], X[:, 2], ids.reshape(-1)])


@pytest.mark.parametrize("window", WINDOWS)
def test_train_shared_fwdbwd_narrow(gpu_lib, narrow, window):
    """train_shared_fwdbwd (narrow ComplEx; B = 97 in groups of 32: a last group of one; M = 33 crosses the 32-wide MFMA tile) against the
    oracle on the window's compact copy: test_gpu_shared.check_against_oracle with its bars (test_gpu_shared::test_shared_fwdbwd_parity)."""
    _shared_case(narrow, "ComplEx", 200, _lo(narrow, window), 0.25)


def _shared_case(geo, model, k, lo, scale):
    eng = geo.engine(model, k)
    geo.fill("gaussian", scale=scale)
    geo.training(eng, "sgd")
    B, G, Mn = 97, 32, 33
    X, Xc, ids_c, ids, side = _shared_lists(geo, np.random.default_rng(59), lo, B, G, Mn, 9)
    ps = torch.full((B,), 7.0, device="cuda")
    ns = torch.full((B * Mn,), 7.0, device="cuda")
    eng.train_shared_fwdbwd(dev(X), G, Mn, dev(ids), dev(side), loss_desc("self_adversarial", "sum"), pos_scores=ps, neg_scores=ns)
    got = _window_got(geo, eng, lo, float(eng.loss_acc[0].item()), ps, ns)
    check_against_oracle(model, geo.window(lo), geo.rel, Xc, G, ids_c, side, got, "self_adversarial", "sum", geo.R)
    _assert_gradient_only_in(geo, eng, _touched_shared(X, ids), "train_shared_fwdbwd")
    eng.g_flat.zero_()


def test_train_shared_masked_fwdbwd(gpu_lib, narrow):
    """train_shared_masked_fwdbwd with GIVEN lists (narrow DistMult, window T) against shared_mask_ref.masked_step on the compact copy:
    test_gpu_shared_mask.check_against_masked_step with its bars (test_gpu_shared_mask::test_masked_fwdbwd_parity)."""
    geo, model, lo = narrow, "DistMult", narrow.T
    eng = geo.engine(model, 400)
    geo.fill("gaussian")
    geo.training(eng, "sgd")
    B, G, Mn = 97, 32, 33
    X, Xc, ids_c, ids, side = _shared_lists(geo, np.random.default_rng(61), lo, B, G, Mn, 11)
    # known statements: for every positive a third of its own list (so the mask bites), as table ids
    rng = np.random.default_rng(62)
    ks_c = [np.unique(ids_c[i // G][rng.random(Mn) < 0.33]).astype(np.int32) for i in range(B)]
    ko_c = [np.unique(ids_c[i // G][rng.random(Mn) < 0.33]).astype(np.int32) for i in range(B)]
    mask, n_masked, n_unmaskable = MR.mask_matrix(Xc, G, ids_c, side, ks_c, ko_c)
    assert n_masked > B
    sf, of = filters([a + lo for a in ks_c], [a + lo for a in ko_c])
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    ps = torch.full((B,), 7.0, device="cuda")
    ns = torch.full((B * Mn,), 7.0, device="cuda")
    eng.train_shared_masked_fwdbwd(dev(X), G, Mn, dev(ids), dev(side), loss_desc("nll", "sum"), s_filter=sf, o_filter=of, stats=stats,
                                   pos_scores=ps, neg_scores=ns)
    got = _window_got(geo, eng, lo, float(eng.loss_acc[0].item()), ps, ns)
    check_against_masked_step(model, geo.window(lo), geo.rel, Xc, G, ids_c, side, mask, got, "nll", "sum", geo.R)
    assert stats.cpu().tolist() == [n_masked, n_unmaskable]
    _assert_gradient_only_in(geo, eng, _touched_shared(X, ids), "train_shared_masked_fwdbwd")
    eng.g_flat.zero_()


def _shared_dist_case(geo, model, k, lo, scale, seed):
    """B = 13 in groups of 8 (a last group of 5), M = 5 (test_gpu_shared_dist::test_shared_dist_fwdbwd_parity's geometry, fewer positives:
    the precondition |d| > 1e-6 / |z| > 1e-3 on every scored pair-unit has to hold over rows of 400 / 1 000 units); plain and masked.
    The pairwise loss: distances over rows this long are far beyond the +-75 at which nll and self_adversarial clip their argument -- there
    every coefficient is zero and a step has no gradient to compare."""
    eng = geo.engine(model, k)
    geo.fill("gaussian", scale=scale)
    geo.training(eng, "sgd")
    B, G, Mn = 13, 8, 5
    X, Xc, ids_c, ids, side = _shared_lists(geo, np.random.default_rng(seed), lo, B, G, Mn, seed)
    ent_c = geo.window(lo)
    assert_conditioned(model, ent_c, geo.rel, Xc, G, ids_c, side, geo.R)
    ks_c = [ids_c[i // G][:2].astype(np.int32) if side[i] else np.zeros(0, np.int32) for i in range(B)]
    ko_c = [np.zeros(0, np.int32) if side[i] else ids_c[i // G][1:3].astype(np.int32) for i in range(B)]
    ks_c, ko_c = [np.unique(a) for a in ks_c], [np.unique(a) for a in ko_c]
    mask, n_masked, n_unmaskable = MR.mask_matrix(Xc, G, ids_c, side, ks_c, ko_c)
    for masked in (False, True):
        eng.g_flat.zero_()
        eng.loss_acc.zero_()
        ps = torch.full((B,), 7.0, device="cuda")
        ns = torch.full((B * Mn,), 7.0, device="cuda")
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
        sf, of = filters([a + lo for a in ks_c], [a + lo for a in ko_c]) if masked else (None, None)
        eng.train_shared_dist_fwdbwd(dev(X), G, Mn, dev(ids), dev(side), loss_desc("pairwise", "sum"), s_filter=sf, o_filter=of, stats=stats,
                                     pos_scores=ps, neg_scores=ns)
        got = _window_got(geo, eng, lo, float(eng.loss_acc[0].item()), ps, ns)
        if not masked:
            check_against_oracle(model, ent_c, geo.rel, Xc, G, ids_c, side, got, "pairwise", "sum", geo.R)
        check_against_ref(model, ent_c, geo.rel, Xc, G, ids_c, side, got, "pairwise", "sum", geo.R, mask=mask if masked else None)
        assert stats.cpu().tolist() == ([n_masked, n_unmaskable] if masked else [0, 0])
        _assert_gradient_only_in(geo, eng, _touched_shared(X, ids), "train_shared_dist_fwdbwd")
    eng.g_flat.zero_()


@pytest.mark.parametrize("window", WINDOWS)
def test_train_shared_dist_fwdbwd_narrow(gpu_lib, narrow, window):
    """train_shared_dist_fwdbwd, plain and masked (narrow TransE), conditioning asserted first as in test_gpu_shared_dist.py; the bars of
    test_gpu_shared.check_against_oracle and test_gpu_shared_dist.check_against_ref."""
    _shared_dist_case(narrow, "TransE", 400, _lo(narrow, window), 0.3, DIST_SEEDS[("narrow", window)])


def test_train_fwdbwd_neg_override(gpu_lib, narrow):
    """train_fwdbwd with neg_override rows inside window T (narrow ComplEx) against O.dense_gradients on the compact copy: the bars of
    test_gpu_kernels::test_train_fwdbwd_parity."""
    geo, model, lo = narrow, "ComplEx", narrow.T
    eng = geo.engine(model, 200)
    geo.fill("gaussian")
    geo.training(eng, "sgd")
    B, eta = 257, 6
    rng = np.random.default_rng(67)
    X, Xc = geo.window_triples(rng, lo, B)
    negs_c = O.generate_corruptions(Xc, M, eta, 9, 4)
    negs = negs_c.copy()
    negs[:, 0] += lo
    negs[:, 2] += lo
    ps, ns = torch.empty(B, device="cuda"), torch.empty(B * eta, device="cuda")
    eng.train_fwdbwd(dev(X), eta, loss_desc("self_adversarial", "sum"), 1, 1, neg_override=dev(negs.astype(np.int32)), pos_scores=ps, neg_scores=ns)
    L, Ge, Gr, ps, ns = _window_got(geo, eng, lo, float(eng.loss_acc[0].item()), ps, ns)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, geo.window(lo), geo.rel, Xc, negs_c, eta, "self_adversarial", None, "sum", geo.R)
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
    assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L))
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)
    _assert_gradient_only_in(geo, eng, np.concatenate([X[:, 0], X[:, 2], negs[:, 0], negs[:, 2]]), "train_fwdbwd(neg_override)")
    eng.g_flat.zero_()


# the seeds of _shared_dist_case for which the precondition holds, found on the CPU: the first that passes, counting from 1
DIST_SEEDS = {("narrow", "T"): 1, ("narrow", "S"): 1, ("wide", "T"): 1, ("wide", "S"): 1}


# ---------------------------------------------------------------------------------------------------- the owner-computes step, in place
def _tiled_case(gpu_lib, geo, model, k, lo, variant, scale):
    """test_table_beyond_2_31_elements' method: the gradient-only step against O.dense_gradients on the window (its bars: loss 2e-5,
    gradients 2e-4 of the row's magnitude), then the complete in-place step against the rule applied to the kernel's own gradient
    (its bar: 5e-6 on the window's rows, which moved by more than 1e-4); every row outside the window keeps its bits.

    variant: "default" (tile-direct on: the row-direct pass takes rows beyond 2 KB, i.e. the wide table; the narrow tables' rows of
    1 600 bytes stay on the LDS tiles and, being C2 / C3 widths, go through the staged persistent forward kernel), "lds" (tile-direct
    off), "hot" (hot-row replicas of rows inside the window), "pos_atomic", "lazy" (the touched-rows optimizer, Adam: its slots too keep
    their bits outside).  The library reports which tile kernel, forward kernel or replica path a step took nowhere (tiled_status
    speaks of deterministic steps only): a comment, not an assertion."""
    from ampligraph_amd import _ffi

    eng = geo.engine(model, k)
    geo.fill("gaussian", scale=scale, rel_scale=0.5 if model == "RotatE" else None)
    lazy = variant == "lazy"
    if lazy:
        geo.drop_scratch()   # (table + gradient + two Adam slots: the engines' cached workspaces go first)
    geo.training(eng, "adam" if lazy else "sgd")
    B, eta = 192, 8
    rng = np.random.default_rng(71)
    X, Xc = geo.window_triples(rng, lo, B)
    hot_c = np.array([7, 11], dtype=np.int32)
    if variant == "hot":
        X[::3, 0], Xc[::3, 0] = lo + 7, 7
        X[1::5, 2], Xc[1::5, 2] = lo + 11, 11
    ent_c, Xd = geo.window(lo), dev(X)
    ld = loss_desc("self_adversarial", "sum")
    lr = 1e-3 if lazy else 0.5
    opt = _ffi.Opt(_ffi.OPTIMIZERS["adam" if lazy else "sgd"], 2, lr, 0.9, 0.999, 1e-7, 0.0, 1)
    opt.lazy = 1 if lazy else 0
    kw = dict(sample_base=lo, sample_range=M, pos_atomic=variant == "pos_atomic")
    negs_c = O.generate_corruptions(Xc, M, eta, 3, 7)
    tot, Ge, Gr, (sp, sn, per) = O.dense_gradients(model, ent_c, geo.rel, Xc, negs_c, eta, "self_adversarial", None, "sum", geo.R)
    touched = lo + np.unique(np.concatenate([Xc[:, 0], Xc[:, 2], negs_c[:, 0], negs_c[:, 2]]))
    try:
        gpu_lib.amdkge_set_tile_direct(0 if variant == "lds" else 1)
        if variant == "hot":
            eng.set_hot_rows(lo + hot_c)
        eng.train_step_tiled(Xd, eta, ld, opt, 3, 7, grad_only=True, **kw)
        L = float(eng.loss_acc[0].item())
        assert abs(L - float(per.astype(np.float64).sum())) <= 2e-5 * abs(L), variant
        g_tiled = eng.g_ent[lo:lo + M].cpu().numpy()
        scale_e = np.maximum(np.abs(Ge).max(axis=1, keepdims=True), 1e-6 * np.abs(Ge).max())
        assert (np.abs(g_tiled - Ge) / scale_e).max() < 2e-4, variant
        assert (np.abs(eng.g_rel.cpu().numpy() - Gr) / np.maximum(np.abs(Gr).max(axis=1, keepdims=True), 1e-30)).max() < 2e-4, variant
        _assert_gradient_only_in(geo, eng, touched, ("train_step_tiled(grad_only)", variant))
        assert not bool(geo.rows_differing().any())                          # a gradient-only step updates nothing
        # the complete step
        eng.g_flat.zero_()
        eng.train_step_tiled(Xd, eta, ld, opt, 3, 7, **kw)
        torch.cuda.synchronize()
        if lazy:
            m_ = np.float32(1 - 0.9) * g_tiled
            v_ = np.float32(1 - 0.999) * g_tiled * g_tiled
            want = ent_c - np.float32(lr * np.sqrt(1 - 0.999) / (1 - 0.9)) * m_ / (np.sqrt(v_) + np.float32(1e-7))
            rows_t = touched - lo
        else:
            want = ent_c - np.float32(lr) * g_tiled
            rows_t = np.arange(M)
        got = eng.ent[lo:lo + M].cpu().numpy()
        assert np.abs(got[rows_t] - want[rows_t]).max() < 5e-6 and np.abs(got - ent_c).max() > 1e-4, (variant, np.abs(got[rows_t] - want[rows_t]).max())
        geo.assert_only(geo.rows_differing(), touched, ("train_step_tiled", variant))
        assert not bool(geo.rows_nonzero(eng.g_ent).any())                   # the complete step leaves the gradient buffer zero
        if lazy:
            for nme in ("m_e", "v_e"):
                geo.assert_only(geo.rows_nonzero(eng.slots[nme]), touched, ("slot", nme))
        assert eng.tiled_status() == 0
    finally:
        gpu_lib.amdkge_set_tile_direct(1)
        eng.set_hot_rows(None)
        geo.restore(lo=lo, hi=lo + M)
        geo.restore_rel()
        if lazy:
            geo.drop_slots()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("variant", ["default", "hot", "pos_atomic", "lazy"])
@pytest.mark.parametrize("model,k", [("DistMult", 400), ("ComplEx", 200)])
def test_train_step_tiled_narrow(gpu_lib, narrow, model, k, variant, window):
    _tiled_case(gpu_lib, narrow, model, k, _lo(narrow, window), variant, 0.25)


def test_cols_partial_scores_and_loss(gpu_lib, narrow):
    """The column-sliced step's phases A and B on a slice engine of the narrow shape (ComplEx, the slice's k = 200 of k_full = 400 units: a
    slice holds up to 256 units per half, so DistMult's 400-unit rows are refused by design:
    tests/test_api_surface.py::test_session_group_argument_validation_without_gpu),
    positives and corruptions inside window T: the slice's partial sums are ComplEx's scores of the slice on its own, and cols_loss on
    them gives the oracle's loss and dL/dscore -- test_gpu_cols::test_cols_phases_against_oracle's bars (scores rtol 2e-5 / atol 2e-5 max,
    loss 3e-5, coefficients rtol 2e-4 / atol 2e-5 max).  (Phase C is train_step_tiled's tile pass -- test_train_step_tiled_* -- fed
    these coefficients instead of forming them; its given-coefficients flag has no case here.)"""
    geo, lo = narrow, narrow.T
    eng = geo.engine("ComplEx", 200, k_full=400)
    assert eng.k_full == 400 > eng.k
    geo.fill("gaussian")
    B, eta, seed, step = 203, 7, 9, 3
    X, Xc = geo.window_triples(np.random.default_rng(79), lo, B)
    negs_c = O.generate_corruptions(Xc, M, eta, seed, step)
    co = {}
    total, _, _, (sp, sn, per) = O.dense_gradients("ComplEx", geo.window(lo), geo.rel, Xc, negs_c, eta, "nll", None, "sum", geo.R, coeffs=co)
    full = eng.cols_partial_scores(dev(X), eta, seed, step, sample_base=lo, sample_range=M).clone()
    got, ref = full.cpu().numpy(), np.concatenate([sp, sn])
    assert np.allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max()), np.abs(got - ref).max()
    eng.loss_acc.zero_()
    eng.cols_loss(loss_desc("nll", "sum"), full, B, eta)
    torch.cuda.synchronize()
    lv = float(eng.loss_acc[0].item())
    assert abs(lv - float(total)) <= 3e-5 * max(1.0, abs(float(total))), (lv, float(total))
    coef = full.cpu().numpy()
    scale = max(np.abs(co["dN"]).max(), np.abs(co["dP"]).max(), 1e-30)
    assert np.allclose(coef[:B], co["dP"], rtol=2e-4, atol=2e-5 * scale) and np.allclose(coef[B:], co["dN"], rtol=2e-4, atol=2e-5 * scale)
    assert not bool(geo.rows_differing().any())


def test_session_layer_on_the_narrow_shape(gpu_lib):
    """amdkge_session_* with numpy only on the narrow shape (DistMult k = 400; the session owns its tables: 5.5 M zero rows, of which T
    and S are set from the host): get_rows by ids (exact), score, rank against the windows' rows as entities_subset (exact:
    RO.evaluate_ranks, as test_gpu_session does for every model but RotatE), and one train_step whose corruptions fall anywhere in
    the table -- the oracle runs on the compact table of every row the step touches; test_gpu_session's bars (loss 2e-5; rows within
    1e-5 + 1e-3 |x| for 99.5 %, 2.5e-2 at most)."""
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import Session

    WT.release_all()
    geo, model, k, eta, seed = NARROW, "DistMult", 400, 5, 11
    geo.host_tables("gaussian", seed=5)
    N, R = geo.N, geo.R
    s = Session(model, k, N, R, eta, loss_functions.get("nll"), optimizers.get("sgd", {"learning_rate": 1e-2}), None, seed=seed)
    try:
        for lo in (geo.T, geo.S):
            s.set_rows("ent", geo.window(lo), row0=lo)
        s.set_rows("rel", geo.rel)
        rng = np.random.default_rng(83)
        ids = np.concatenate([geo.T + rng.integers(0, M, 50), geo.S + rng.integers(0, M, 50), [N - 1, geo.first_high, geo.first_high - 1, 0, geo.S - 1]])
        want = geo.rows(ids)
        want[-2:] = 0.0                                                      # rows the host never set
        assert int(ids.max()) * geo.Ks > 2 ** 31 - 1 and np.array_equal(bits(s.get_rows("ent", ids=ids)), bits(want))
        # queries and candidates inside T and S: the compact table is [T rows | S rows]
        win = np.concatenate([geo.T + np.arange(M), geo.S + np.arange(M)])
        ent_c = geo.rows(win)
        n = 40
        Tc = np.stack([rng.integers(0, 2 * M, n), rng.integers(0, R, n), rng.integers(0, 2 * M, n)], 1).astype(np.int32)
        Tq = Tc.copy()
        Tq[:, 0], Tq[:, 2] = win[Tc[:, 0]], win[Tc[:, 2]]
        ref_sc = O.compute_scores(model, *O.lookup(ent_c, geo.rel, Tc.astype(np.int64)), max_rel_size=R)
        assert np.allclose(s.score(Tq), ref_sc, rtol=1e-5, atol=1e-5 * np.abs(ref_sc).max())
        got = s.rank(Tq, entities_subset=win.astype(np.int32), corrupt_side="s,o")
        assert np.array_equal(got, RO.evaluate_ranks(model, ent_c, geo.rel, Tc, None, None, "s,o", "worst", max_rel_size=R))
        # one step: positives in T and S, corruptions drawn over all N rows (zero rows outside the windows)
        B = 150
        Xc = np.stack([rng.integers(0, 2 * M, B), rng.integers(0, R, B), rng.integers(0, 2 * M, B)], 1).astype(np.int32)
        X = Xc.copy()
        X[:, 0], X[:, 2] = win[Xc[:, 0]], win[Xc[:, 2]]
        negs = O.generate_corruptions(X, N, eta, seed, 0)
        rows, inv = np.unique(np.concatenate([X[:, [0, 2]].reshape(-1), negs[:, [0, 2]].reshape(-1)]), return_inverse=True)
        table = np.where(np.isin(rows, win)[:, None], geo.rows(rows), np.float32(0.0)).astype(np.float32)
        Xr, negs_r = X.copy(), negs.copy()
        Xr[:, [0, 2]] = inv[:2 * B].reshape(B, 2)
        negs_r[:, [0, 2]] = inv[2 * B:].reshape(-1, 2)
        st = O.TrainState(table, geo.rel, "sgd", 1e-2)
        loss = s.train_step(X)
        ref = float(O.train_step(st, model, Xr, eta, "nll", seed, 0, max_rel_size=R, negs=negs_r))
        assert abs(loss - ref) <= 2e-5 * abs(ref), (loss, ref)
        e = s.get_rows("ent", ids=rows)
        assert np.mean(np.abs(e - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.995 and np.abs(e - st.ent).max() < 2.5e-2
        assert np.abs(e - table).max() > 1e-5                                # the step moved rows
        # rows next to the touched ones kept their bits (the rest of the table is the session's: not visible from the host in one piece)
        near = np.setdiff1d(np.concatenate([win[::5], rows + 1, rows - 1]), rows)
        near = near[(near >= 0) & (near < N)]
        keep = np.where(np.isin(near, win)[:, None], geo.rows(near), np.float32(0.0)).astype(np.float32)
        assert np.array_equal(bits(s.get_rows("ent", ids=near)), bits(keep))
    finally:
        s.close()


# ====================================================================================================== the wide table
# (Its cases stand together behind the narrow ones: Geometry.engine releases the narrow table when the first of them asks for an engine.)
def test_gather_and_scatter_add_rows_wide(gpu_lib, wide):
    _gather_scatter_case(wide)


@pytest.mark.parametrize("window", WINDOWS)
def test_train_shared_fwdbwd_wide(gpu_lib, wide, window):
    """train_shared_fwdbwd on the wide DistMult table (k = 2 000), as test_train_shared_fwdbwd_narrow."""
    _shared_case(wide, "DistMult", 2000, _lo(wide, window), 0.2)


@pytest.mark.parametrize("window", WINDOWS)
def test_train_shared_dist_fwdbwd_wide(gpu_lib, wide, window):
    """train_shared_dist_fwdbwd, plain and masked, on the wide RotatE table (k = 1 000), as test_train_shared_dist_fwdbwd_narrow."""
    _shared_dist_case(wide, "RotatE", 1000, _lo(wide, window), 0.5, DIST_SEEDS[("wide", window)])


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("variant", ["default", "lds", "lazy"])
def test_train_step_tiled_wide(gpu_lib, wide, variant, window):
    """The in-place step on the wide RotatE table: the row-direct tile pass (default), the LDS-accumulator kernel it replaces, the
    touched-rows optimizer."""
    _tiled_case(gpu_lib, wide, "RotatE", 1000, _lo(wide, window), variant, 0.025)   # (scores of about -45: inside the loss's clip at -75)


def test_rank_lists_wide(gpu_lib, wide):
    _rank_lists_case(wide, "RotatE", 1000, "gaussian")


def test_rank_side_whole_table_rotate(gpu_lib, wide):
    """rank_side over all rows of the wide RotatE table: the plain tile kernel and the early exit forced; exact."""
    _distance_sweep(gpu_lib, wide, "RotatE", 1000)


def test_corruption_topk_wide(gpu_lib, wide):
    _corruption_topk_case(wide, "RotatE", 1000)


@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("lazy", [False, True])
def test_opt_step_whole_table(gpu_lib, wide, lazy, lam):
    """amdkge_opt_step (Adam, n_elems > 2^31) over the whole wide table, with and without an L2 term, dense and touched-rows: the rows of T
    and S and six probe rows against the oracle's rule.  Dense: test_gpu_kernels::test_opt_step_parity's bars (2e-6 on the parameters,
    rtol 2e-5 / atol 2e-7 max on the slots, 1e-5 on reg_loss, whose host value counts every base row N / P times).  Touched rows: the
    gradient is non-zero on T and S only, every other row keeps its bits in x and both slots, reg_loss is that of the touched rows
    (test_gpu_lazy::test_lazy_dense_sweep_parity's bars: the same, reg_loss 1e-5)."""
    from ampligraph_amd import _ffi

    geo = wide
    eng = geo.engine("DistMult", 2000)
    geo.fill("gaussian", scale=0.2)
    geo.drop_scratch()   # (the engines' cached workspaces: this case alone holds table + gradient + two slots)
    geo.training(eng, "adam")
    rng = np.random.default_rng(73)
    win = np.concatenate([geo.T + np.arange(M), geo.S + np.arange(M)])
    probes = np.array([0, 1, geo.N // 2, geo.B + 5, geo.S - 1, geo.T - 1])
    rows = np.concatenate([win, probes])
    assert eng.ent.numel() > 2 ** 31 and int(win.max()) * geo.Ks > 2 ** 31 - 1
    G = np.zeros((len(rows), geo.Ks), np.float32)
    G[:len(win)] = (rng.normal(size=(len(win), geo.Ks)) * 0.1).astype(np.float32)
    try:
        if not lazy:   # a dense gradient, g[i] = gbase[i % P] outside the windows: the host knows every row of it too
            gbase = (rng.normal(size=(P, geo.Ks)) * 0.1).astype(np.float32)
            geo.restore(table=eng.g_ent, source=dev(gbase))
            G[len(win):] = gbase[probes % P]
        eng.g_ent[dev(win)] = dev(G[:len(win)])
        x0 = geo.rows(rows)
        st = O.TrainState(x0, geo.rel, "adam", 1e-3)
        opt = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1)
        opt.lazy = 1 if lazy else 0
        eng.opt_step(opt, lam, lam)
        torch.cuda.synchronize()
        Gr = np.zeros(geo.rel.shape, np.float64)
        if lazy:
            want_reg = O.apply_optimizer_lazy(st, G.astype(np.float64), Gr, dict(p=2, lam_e=lam, lam_r=lam) if lam else None)
        else:
            want_reg = lam * (geo.mult * float((geo.base.astype(np.float64) ** 2).sum()) + float((geo.rel.astype(np.float64) ** 2).sum()))
            O.apply_optimizer(st, G.astype(np.float64) + lam * 2 * x0.astype(np.float64), Gr + lam * 2 * geo.rel.astype(np.float64))
        got = eng.ent[dev(rows)].cpu().numpy()
        assert np.abs(got - st.ent).max() <= 2e-6 * max(1.0, np.abs(st.ent).max()), np.abs(got - st.ent).max()
        assert np.abs(got[:len(win)] - x0[:len(win)]).max() > 1e-4                # the rows moved
        for n_ in ("m_e", "v_e"):
            ref = st.slots[n_]
            assert np.allclose(eng.slots[n_][dev(rows)].cpu().numpy(), ref, rtol=2e-5 if lam else 2e-6, atol=2e-7 * max(1e-30, np.abs(ref).max())), n_
        assert not bool(geo.rows_nonzero(eng.g_ent).any())                       # the gradient reset, every row
        if lazy:
            geo.assert_only(geo.rows_differing(), win, "opt_step(lazy): table")
            for n_ in ("m_e", "v_e"):
                geo.assert_only(geo.rows_nonzero(eng.slots[n_]), win, ("opt_step(lazy)", n_))
        else:   # x and g repeat with period P outside the windows, so the swept table and slots do: every row against its first copy
            for t_ in (eng.ent, eng.slots["m_e"], eng.slots["v_e"]):
                geo.assert_only(geo.rows_differing(t_, source=t_[:P].clone()), win, "opt_step(dense): periodicity")
        if lam:
            assert abs(float(eng.loss_acc[1]) - want_reg) <= 1e-5 * want_reg, (float(eng.loss_acc[1]), want_reg)
    finally:
        geo.restore()
        geo.restore_rel()
        geo.drop_slots()
