"""Parity at BASELINE.json's full sizes (the oracle is too slow there) through size-independent properties:
independent kernels must agree with each other, invariants of the domain must hold.
C1 TransE k=50 eta=5, C2 ComplEx k=200 eta=20, C3 DistMult k=400 eta=30 + 1-vs-all filtered eval (WN18RR shape),
C4 ComplEx k=200 on 123 182 entities, C5 row width (RotatE k=1000, eta=64) on a cut-down entity count."""
import numpy as np
import pytest
import torch
from margins import rel_gap, within

pytestmark = pytest.mark.gpu


def _engine(model, k, N, R, seed=0):
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    g = torch.Generator(device="cuda").manual_seed(seed)
    lim = float(np.sqrt(6.0 / (N + eng.K)))
    eng.pack((torch.rand(N, eng.K, device="cuda", generator=g) * 2 - 1) * lim, out=eng.ent)
    eng.pack((torch.rand(R, eng.K, device="cuda", generator=g) * 2 - 1) * float(np.sqrt(6.0 / (R + eng.K))), out=eng.rel)
    return eng


def _triples(n, N, R, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.stack([torch.randint(0, N, (n,), device="cuda", generator=g), torch.randint(0, R, (n,), device="cuda", generator=g),
                        torch.randint(0, N, (n,), device="cuda", generator=g)], 1).to(torch.int32).contiguous()


def _loss(name, **kw):
    from ampligraph_amd import _ffi

    d = {"pairwise": (0, 1.0, 0.0), "nll": (1, 0.0, 0.0), "self_adversarial": (3, 3.0, 0.5), "multiclass_nll": (4, 0.0, 0.0)}[name]
    return _ffi.Loss(d[0], 0, d[1], d[2])


def _rows_close(a, b, tol):
    scale = b.abs().amax(dim=1, keepdim=True).clamp_min(1e-6 * float(b.abs().max()) + 1e-30)
    return float(((a - b).abs() / scale).max()) < tol


def _rotate_rows_close(a, b, tol):
    """RotatE entity gradients of two fp32 evaluations.  The tile pass differentiates |e o r - o| w.r.t. a replaced SUBJECT
    row as (e - B) / |e - B| with the staged B = o o conj(r) (kge_train_kernel.h), the atomic path as
    conj(r) o (e o r - o) / |e o r - o|: the same unit vector, and both ill-conditioned where a unit's modulus m is ~0 --
    each carries the operands' rounding noise divided by m, so over the 1e7 ... 1e8 corruption units of a full-size batch
    the two part by up to ~1e-3 of a row's scale in a handful of elements (either is as far from the exact value as from
    the other).  Bulk at `tol`, tail bounded."""
    scale = b.abs().amax(dim=1, keepdim=True).clamp_min(1e-6 * float(b.abs().max()) + 1e-30)
    err = (a - b).abs() / scale
    return float((err > tol).float().mean()) < 1e-6 and float(err.max()) < 2e-2


@pytest.mark.parametrize("model,k,eta,N,R,B,loss", [("ComplEx", 200, 20, 14505, 237, 10000, "self_adversarial"),    # C2
                                                     ("DistMult", 400, 30, 40943, 11, 10000, "multiclass_nll"),      # C3
                                                     ("TransE", 52, 5, 14505, 237, 10000, "pairwise"),
                                                     ("TransE", 50, 5, 14505, 237, 10000, "pairwise"),               # C1 (stored as 52 units)
                                                     ("ComplEx", 350, 20, 14505, 237, 10000, "self_adversarial"),    # the reference's published k (experiments/config.json:43-52), stored as 352
                                                     ("RotatE", 350, 20, 14505, 237, 4096, "self_adversarial"),
                                                     ("ComplEx", 200, 20, 123182, 37, 8192, "nll")])                 # C4
def test_fullsize_train_paths_agree(gpu_lib, model, k, eta, N, R, B, loss):
    """The owner-computes pair (gradient-only form) and the atomic-scatter kernel are independent implementations of the
    same step: loss, scores and both dense gradients must agree at full size; then the in-place pair == gradient-only
    pair + dense sweep."""
    from ampligraph_amd import _ffi

    eng = _engine(model, k, N, R)
    X = _triples(B, N, R)
    ld = _loss(loss)
    opt = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1)
    eng.prepare_training("adam")
    ps1, ns1 = torch.empty(B, device="cuda"), torch.empty(B * eta, device="cuda")
    eng.loss_acc.zero_()
    eng.train_fwdbwd(X, eta, ld, 5, 9, pos_scores=ps1, neg_scores=ns1)
    l1 = float(eng.loss_acc[0])
    ge1, gr1 = eng.g_ent.clone(), eng.g_rel.clone()
    eng.g_flat.zero_()
    eng.loss_acc.zero_()
    ps2, ns2 = torch.empty(B, device="cuda"), torch.empty(B * eta, device="cuda")
    eng.train_step_tiled(X, eta, ld, opt, 5, 9, grad_only=True, pos_scores=ps2, neg_scores=ns2)
    l2 = float(eng.loss_acc[0])
    assert abs(l1 - l2) <= 2e-5 * abs(l1), (l1, l2)
    assert torch.allclose(ps1, ps2, rtol=2e-5, atol=2e-5 * float(ps1.abs().max()))
    assert torch.allclose(ns1, ns2, rtol=2e-5, atol=2e-5 * float(ns1.abs().max()))
    assert (_rotate_rows_close if model == "RotatE" else _rows_close)(eng.g_ent, ge1, 2e-4) and _rows_close(eng.g_rel, gr1, 2e-4)
    if model == "TransE":   # translation invariance: d/ds + d/do = 0 for every triple => column sums of the entity gradient vanish
        assert float(eng.g_ent.sum(0).abs().max()) < 1e-3 * float(eng.g_ent.abs().sum(0).max())
    # in-place pair vs gradient-only pair + dense sweep (same gradient buffers as input)
    ent0, rel0 = eng.ent.clone(), eng.rel.clone()
    eng.opt_step(opt)
    ent_a, rel_a = eng.ent.clone(), eng.rel.clone()
    eng.ent.copy_(ent0); eng.rel.copy_(rel0)
    for t in eng.slots.values():
        t.zero_()
    eng.train_step_tiled(X, eta, ld, opt, 5, 9)
    assert float((eng.ent - ent_a).abs().max()) < 2.1e-3   # one Adam step moves at most lr (sign flips of ~0 gradients)
    assert float(((eng.ent - ent_a).abs() < 2e-6).float().mean()) > 0.995
    assert float(((eng.rel - rel_a).abs() < 2e-6).float().mean()) > 0.99
    assert float(eng.g_rel.abs().max()) == 0.0


def test_fullsize_c3_eval_invariants(gpu_lib):
    """C3: DistMult k=400, 40 943 entities, 2 924 test triples, both sides (MFMA path)."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.datasets.filters import FilterIndex

    d = make_synthetic_kg("synth-wn18rr")
    N, R = d["n_ents"], d["n_rels"]
    eng = _engine("DistMult", 400, N, R)
    test = d["test"]
    Xd = torch.as_tensor(test).cuda()
    fi = FilterIndex([d["train"], d["valid"], test], N, R)
    res = {}
    for side, nm, rng_fn, ids in ((_ffi.SIDE_S, "s", fi.subject_ranges, fi.s_ids), (_ffi.SIDE_O, "o", fi.object_ranges, fi.o_ids)):
        lo, hi = rng_fn(test)
        flt = (torch.as_tensor(lo).cuda(), torch.as_tensor(hi).cuda(), torch.as_tensor(ids).cuda())
        r_w, c_mfma, sub = eng.rank_side(Xd, side, "worst", flt)
        try:
            _ffi.check(gpu_lib.amdkge_set_rank_kernel(1))
            c_valu = eng.rank_side(Xd, side, "worst")[1]
        finally:
            gpu_lib.amdkge_set_rank_kernel(0)
        assert torch.equal(c_mfma, c_valu)                       # exact-fp32 MFMA == VALU chain, bit for bit
        r_b = eng.rank_side(Xd, side, "best", flt)[0]
        r_m = eng.rank_side(Xd, side, "middle", flt)[0]
        r_u = eng.rank_side(Xd, side, "worst")[0]
        assert bool((r_b <= r_m).all()) and bool((r_m <= r_w).all()) and bool((r_w <= r_u).all())
        assert int(r_b.min()) >= 1 - int(sub.max()) and int(r_u.max()) <= N + 1
        assert bool((c_mfma.sum(1) <= N).all())
        # the test triple itself is in its own filter: its own corruption (score == positive) is always subtracted
        assert bool((sub >= 1).all())
        res[nm] = r_w


def test_fullsize_c5_row_width_scores_agree(gpu_lib):
    """C5 row width (RotatE k=1000 -> 8 000-byte rows, eta=64) on 200 000 entities: the fused kernel's scores ==
    the stand-alone score kernel on the corruptions the stand-alone sampler materialises (three independent kernels)."""
    from ampligraph_amd import _ffi

    N, R, k, eta, B = 200_000, 100, 1000, 64, 2048
    eng = _engine("RotatE", k, N, R)
    X = _triples(B, N, R, seed=3)
    eng.prepare_training("sgd")
    ps, ns = torch.empty(B, device="cuda"), torch.empty(B * eta, device="cuda")
    eng.train_fwdbwd(X, eta, _loss("self_adversarial"), 21, 4, pos_scores=ps, neg_scores=ns)
    negs = eng.sample_corruptions(X, eta, 21, 4)
    assert bool(((negs[:, 0] == X[:, 0].repeat(eta)) ^ (negs[:, 2] == X[:, 2].repeat(eta)) | (negs[:, 0] == X[:, 0].repeat(eta))).all())
    ref_p, ref_n = eng.score(X), eng.score(negs)
    assert torch.allclose(ps, ref_p, rtol=2e-5, atol=1e-5 * float(ref_p.abs().max()))
    assert torch.allclose(ns, ref_n, rtol=2e-5, atol=1e-5 * float(ref_n.abs().max()))
    assert bool(torch.isfinite(eng.g_ent).all()) and float(eng.g_ent.abs().max()) > 0
    # only touched rows carry gradient: rows that are neither s/o of a positive nor a replacement stay exactly zero
    touched = torch.zeros(N, dtype=torch.bool, device="cuda")
    touched[X[:, 0].long()] = True; touched[X[:, 2].long()] = True
    touched[negs[:, 0].long()] = True; touched[negs[:, 2].long()] = True
    assert float(eng.g_ent[~touched].abs().max()) == 0.0
    # the owner-computes pair at this row width (one positive per workgroup) agrees with the atomic path
    assert eng.tiled_supported(B, eta)
    ge, gr, l1 = eng.g_ent.clone(), eng.g_rel.clone(), float(eng.loss_acc[0])
    eng.g_flat.zero_(); eng.loss_acc.zero_()
    ns2 = torch.empty(B * eta, device="cuda")
    eng.train_step_tiled(X, eta, _loss("self_adversarial"), _ffi.Opt(0, 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1), 21, 4,
                         grad_only=True, neg_scores=ns2)
    assert abs(float(eng.loss_acc[0]) - l1) <= 2e-5 * abs(l1)
    assert torch.allclose(ns2, ns, rtol=2e-5, atol=1e-5 * float(ns.abs().max()))
    assert _rows_close(eng.g_rel, gr, 3e-4)
    assert _rotate_rows_close(eng.g_ent, ge, 3e-4)


def test_fullsize_c2_step_against_oracle(gpu_lib):
    """The one full-size run the oracle affords (~30 s of numpy): a C2 batch (ComplEx k=200, eta=20, 10 000 positives,
    14 505 entities) through the owner-computes pair, loss and both dense gradients against the oracle directly."""
    from oracle import kge_oracle as O

    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    rng = np.random.default_rng(0)
    N, R, k, B, eta = 14505, 237, 200, 10000, 20
    ent = rng.uniform(-0.02, 0.02, (N, 2 * k)).astype(np.float32)
    rel = rng.uniform(-0.1, 0.1, (R, 2 * k)).astype(np.float32)
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
    eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ld = _loss("self_adversarial")
    eng.train_step_tiled(torch.as_tensor(X).cuda(), eta, ld, _ffi.Opt(2, 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1), 5, 9, grad_only=True)
    torch.cuda.synchronize()
    negs = O.generate_corruptions(X, N, eta, 5, 9)
    tot, Ge, Gr, (sp, sn, per) = O.dense_gradients("ComplEx", ent, rel, X, negs, eta, "self_adversarial", None, "sum", R)
    L = float(eng.loss_acc[0])
    assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * abs(L), (L, float(tot))
    for got, ref in ((eng.g_ent.cpu().numpy(), Ge), (eng.g_rel.cpu().numpy(), Gr)):
        scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-6 * np.abs(ref).max())
        assert (np.abs(got - ref) / scale).max() < 1e-4   # up to ~40 unordered fp32 terms per entity row, 1 700 per relation row


@pytest.mark.parametrize("model,k,N,n", [("ComplEx", 200, 14505, 192), ("DistMult", 400, 40943, 48)])
def test_fullsize_ranks_against_oracle(gpu_lib, model, k, N, n):
    """1-vs-all ranks against ALL entities of the C2 / C3 tables for a few test triples (the oracle's numpy broadcast
    costs ~0.1-0.5 s per triple at these sizes), filtered, against the oracle:
    differences only where the quantised comparison is fragile under fp32 summation order (bound per triple),
    MRR within 0.002 (the north_star's bar)."""
    from oracle import kge_oracle as O

    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.engine import KgeEngine

    rng = np.random.default_rng(3)
    R = 11
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    other = np.stack([rng.integers(0, N, 50000), rng.integers(0, R, 50000), rng.integers(0, N, 50000)], 1).astype(np.int32)
    other[:20000, 1:] = X[rng.integers(0, n, 20000), 1:]   # many true subjects for the test (p, o) pairs
    other[20000:40000, :2] = X[rng.integers(0, n, 20000), :2]
    fs, fo = O.filter_sets(X, [X, other])
    ref = O.evaluate_ranks(model, ent, rel, X, fs, fo, "s,o", "worst", max_rel_size=R)
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    fi = FilterIndex([X, other], N, R)
    Xd = torch.as_tensor(X).cuda()
    got = []
    for side, rng_fn, ids in ((_ffi.SIDE_S, fi.subject_ranges, fi.s_ids), (_ffi.SIDE_O, fi.object_ranges, fi.o_ids)):
        lo, hi = rng_fn(X)
        flt = (torch.as_tensor(lo).cuda(), torch.as_tensor(hi).cuda(), torch.as_tensor(ids).cuda())
        got.append(eng.rank_side(Xd, side, "worst", flt)[0])
    got = torch.stack(got, 1).cpu().numpy()
    for c, side in enumerate(("s", "o")):
        frag = O.fragile_rank_mask(model, ent, rel, X, side, max_rel_size=R)
        diff = np.abs(got[:, c] - ref[:, c])
        assert (diff <= 2 * frag).all(), (side, diff.max())
    assert (got != ref).mean() < 0.05
    assert abs(O.mrr_score(got) - O.mrr_score(ref)) < 2e-3


@pytest.mark.parametrize("model,k", [("RotatE", 1000), ("DistMult", 2000)])
def test_table_beyond_2_31_elements(gpu_lib, model, k):
    """(DistMult: the same through the single-pass F and the MFMA rank kernel.)  One GPU's C5 shard is 6.25 M rows x 2 000 floats = 12.5 G elements: every row offset must be 64-bit.  A RotatE
    k=1000 table of 1.15 M rows (2.3 G floats, beyond 2^31) is trained / scored / ranked on its LAST 4 096 rows only
    (sample_base / sample_range, ent_lo / ent_hi) and compared with the oracle on exactly those rows; rows outside stay
    bit-identical; the same on the FIRST 4 096 rows."""
    from oracle import kge_oracle as O

    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    N, R, eta, B, M = 1_150_000, 16, 8, 192, 4096
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    assert eng.ent.numel() > 2**31
    g = torch.Generator(device="cuda").manual_seed(1)
    for r0 in range(0, N, 1 << 18):
        eng.ent[r0:r0 + (1 << 18)].uniform_(-0.05, 0.05, generator=g)
    eng.rel.uniform_(-0.5, 0.5, generator=g)
    eng.prepare_training("adam")
    rng = np.random.default_rng(5)
    ld = _loss("self_adversarial")
    opt = lambda t: _ffi.Opt(2, 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, t)   # noqa: E731
    for base in (N - M, 0):
        ent_c = eng.ent[base:base + M].cpu().numpy()
        rel = eng.rel.cpu().numpy()
        Xc = np.stack([rng.integers(0, M, B), rng.integers(0, R, B), rng.integers(0, M, B)], 1).astype(np.int32)
        X = Xc.copy(); X[:, 0] += base; X[:, 2] += base
        Xd = torch.as_tensor(X).cuda()
        # scores
        ref_s = O.compute_scores(model, *O.lookup(ent_c, rel, Xc.astype(np.int64)), max_rel_size=R)
        assert np.allclose(eng.score(Xd).cpu().numpy(), ref_s, rtol=2e-5, atol=1e-5 * np.abs(ref_s).max())
        # gradients of both fused paths against the oracle on the compact table
        negs_c = O.generate_corruptions(Xc, M, eta, 3, 7)
        tot, Ge, Gr, (sp, sn, per) = O.dense_gradients(model, ent_c, rel, Xc, negs_c, eta, "self_adversarial", None, "sum", R)
        for path in ("tiled", "atomic"):
            eng.g_flat.zero_(); eng.loss_acc.zero_()
            if path == "tiled":
                eng.train_step_tiled(Xd, eta, ld, opt(1), 3, 7, sample_base=base, sample_range=M, grad_only=True)
            else:
                eng.train_fwdbwd(Xd, eta, ld, 3, 7, sample_base=base, sample_range=M)
            L = float(eng.loss_acc[0])
            assert abs(L - float(per.astype(np.float64).sum())) <= 2e-5 * abs(L), path
            got = eng.g_ent[base:base + M].cpu().numpy()
            scale = np.maximum(np.abs(Ge).max(axis=1, keepdims=True), 1e-6 * np.abs(Ge).max())
            assert (np.abs(got - Ge) / scale).max() < 2e-4, path
            assert (np.abs(eng.g_rel.cpu().numpy() - Gr) / np.maximum(np.abs(Gr).max(axis=1, keepdims=True), 1e-30)).max() < 2e-4
            outside = eng.g_ent[:base] if base else eng.g_ent[M:]
            assert float(outside.abs().max()) == 0.0, path
            if path == "tiled":
                g_tiled = got.copy()
        # the complete in-place step: rows of the window follow Adam on the gradient just checked (the kernel's own bits: the
        # update is ill-conditioned where |g| ~ eps, so the oracle's gradient would not do), all other rows keep their bits
        eng.g_flat.zero_()
        probe = [0, 1, N // 2, N - 1, base - 1 if base else M, (base + M) % N]
        probe = [r for r in probe if not (base <= r < base + M)]
        before = eng.ent[probe].clone()
        eng.train_step_tiled(Xd, eta, ld, opt(1), 3, 7, sample_base=base, sample_range=M)
        m = np.float32(1 - 0.9) * g_tiled; v = np.float32(1 - 0.999) * g_tiled * g_tiled
        want = ent_c - np.float32(1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)) * m / (np.sqrt(v) + np.float32(1e-7))
        got = eng.ent[base:base + M].cpu().numpy()
        assert np.abs(got - want).max() < 5e-6 and np.abs(got - ent_c).max() > 1e-4
        assert torch.equal(eng.ent[probe], before)
        for s in eng.slots.values():   # fresh slots for the second window
            s.zero_()
        eng.ent[base:base + M].copy_(torch.as_tensor(ent_c))
        # ranks against the window's rows (what a row-sharded rank counts against its shard)
        T = Xc[:12].astype(np.int64)
        rel = eng.rel.cpu().numpy()   # the in-place step above also swept the relation table
        s_, p_, o_ = O.lookup(ent_c, rel, T)
        tq = O.quantise(O.compute_scores(model, s_, p_, o_, max_rel_size=R))
        for side, nm in ((_ffi.SIDE_S, "s"), (_ffi.SIDE_O, "o")):
            cq = O.quantise(O.corruption_scores(model, nm, s_, p_, o_, ent_c, R))
            ref = np.stack([(tq[:, None] < cq).sum(1), (tq[:, None] == cq).sum(1)], 1)
            _, counts, _ = eng.rank_side(Xd[:12], side, "worst", None, ent_lo=base, ent_hi=base + M)
            assert np.abs(counts.cpu().numpy() - ref).max() <= 2, nm


@pytest.mark.parametrize("model,k,dataset,n_test", [("ComplEx", 200, "synth-fb15k237", None),     # C2: all 20 438 test triples
                                                      ("DistMult", 400, "synth-wn18rr", None),      # C3: all 2 924 test triples
                                                      ("HolE", 350, "synth-fb15k237", 3000),        # padded halves (350 -> 352)
                                                      ("TransE", 50, "synth-fb15k237", 3000),       # C1 shape, L1 chain
                                                      ("RotatE", 200, "synth-fb15k237", None),      # all 20 438 triples, exact-mode modulus (round 3)
                                                      ("RotatE", 50, "synth-fb15k237", 3000)])      # padded halves (50 -> 52): live units only
def test_fullsize_filtered_ranks_bit_identical(gpu_lib, model, k, dataset, n_test):
    """"Identical filtered ranks" (BASELINE.json north_star) at full size on REAL-VALUED tables: the HIP path against the
    oracle's declared-order fp32 mode (oracle/rank_ordered.py: same rounding points, same accumulation order as
    the ranking kernels declare, kge_rank_common.h) -- every test triple, filter = train + valid + test, three tie strategies, four corrupt_side
    forms, bit for bit.  (The fp64 oracle mode stays as the order-free cross-check in test_fullsize_ranks_against_oracle.)"""
    from oracle import kge_oracle as O
    from oracle import rank_ordered as RO

    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.engine import KgeEngine

    d = make_synthetic_kg(dataset)
    N, R = d["n_ents"], d["n_rels"]
    rng = np.random.default_rng(17)
    K = O.internal_k(model, k)
    # trained-table-like magnitudes: scores of a few units, thousands of distinct quantised values, some ties
    ent = (rng.normal(size=(N, K)) * 0.25).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.25).astype(np.float32)
    test = d["test"] if n_test is None else d["test"][:n_test]
    n = test.shape[0]
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    fi = FilterIndex([d["train"], d["valid"], d["test"]], N, R)
    Xd = torch.as_tensor(test).cuda()
    gpu, ora = {}, {}
    for side, nm, rng_fn, ids in ((_ffi.SIDE_S, "s", fi.subject_ranges, fi.s_ids), (_ffi.SIDE_O, "o", fi.object_ranges, fi.o_ids)):
        lo, hi = rng_fn(test)
        flt = (torch.as_tensor(lo).cuda(), torch.as_tensor(hi).cuda(), torch.as_tensor(ids).cuda())
        _, counts, sub = eng.rank_side(Xd, side, "worst", flt)
        gpu[nm] = (counts.cpu().numpy().astype(np.int64), sub.cpu().numpy().astype(np.int64))
        lists = [ids[a:b] for a, b in zip(lo, hi)]
        if nm == "s":   # the filter lists handed to the oracle are the reference's sets (graph_data_loader.py:287-350): spot-check
            pick = rng.choice(n, 64, replace=False)
            fs_ref, _ = O.filter_sets(test[pick], [d["train"], d["valid"], d["test"]])
            assert all(np.array_equal(np.sort(lists[i]), np.sort(np.asarray(f))) for i, f in zip(pick, fs_ref))
        oc, ctx = RO.side_counts(model, nm, ent, rel, test, R)
        ora[nm] = (oc.astype(np.int64), RO.filter_sub(ctx, lists).astype(np.int64))
        assert np.array_equal(gpu[nm][0], ora[nm][0]), (nm, "counts", int((gpu[nm][0] != ora[nm][0]).sum()))
        assert np.array_equal(gpu[nm][1], ora[nm][1]), (nm, "filter subtraction")
        assert len(np.unique(ora[nm][0][:, 0])) > min(n, N) // 50 and int(ora[nm][0][:, 1].sum()) >= 0   # a real ranking problem

    def ranks(src, strat, cs):
        cols = []
        for nm in ("s", "o"):
            if nm not in cs:
                continue
            (gt, eq), sub = (src[nm][0][:, 0], src[nm][0][:, 1]), src[nm][1]
            r = gt if strat == "best" else (gt + (eq + 1) // 2 if strat == "middle" else gt + eq)
            cols.append(r - sub)
        r = np.stack(cols, 1)
        return (r.sum(1, keepdims=True) if cs == "s+o" else r) + 1

    for strat in ("worst", "best", "middle"):
        for cs in ("s", "o", "s,o", "s+o"):
            assert np.array_equal(ranks(gpu, strat, cs), ranks(ora, strat, cs)), (strat, cs)
    # and through the product's own compose kernel (tie strategy + filter subtraction + 1)
    for strat in ("worst", "best", "middle"):
        got = torch.stack([eng.rank_side(Xd, sd, strat, (torch.as_tensor(f(test)[0]).cuda(), torch.as_tensor(f(test)[1]).cuda(), torch.as_tensor(i_).cuda()))[0]
                           for sd, f, i_ in ((_ffi.SIDE_S, fi.subject_ranges, fi.s_ids), (_ffi.SIDE_O, fi.object_ranges, fi.o_ids))], 1).cpu().numpy()
        assert np.array_equal(got, ranks(ora, strat, "s,o")), strat
    mrr_g, mrr_o = float(np.mean(1.0 / ranks(gpu, "worst", "s,o"))), float(np.mean(1.0 / ranks(ora, "worst", "s,o")))
    assert mrr_g == mrr_o


def test_fullsize_rotate_c5_width_ranks_bit_identical(gpu_lib):
    """RotatE at configs[4]'s row width (k = 1000: 8 000-byte rows, 1 000 relations) against 200 000 entities, 1 024 test triples,
    both sides, filtered: counts, filter subtractions and ranks of the HIP path's exact mode == the declared-order oracle, bit
    for bit; then the fast (1-ulp v_sqrt_f32) mode on the same inputs: equal or off by a handful of fragile comparisons."""
    from oracle import rank_ordered as RO

    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.engine import KgeEngine

    N, R, k, n = 200_000, 1000, 1000, 1024
    rng = np.random.default_rng(23)
    ent = (rng.standard_normal((N, 2 * k), dtype=np.float32) * np.float32(0.05))
    rel = (rng.standard_normal((R, 2 * k), dtype=np.float32) * np.float32(0.002))
    train = np.stack([rng.integers(0, N, 300_000), rng.integers(0, R, 300_000), rng.integers(0, N, 300_000)], 1).astype(np.int32)
    test = train[:n].copy()
    test[n // 2:, 0] = rng.integers(0, N, n - n // 2)   # half of the test triples are in the filter set with their own (p, o) group
    eng = KgeEngine("RotatE", k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    fi = FilterIndex([train, test], N, R)
    Xd = torch.as_tensor(test).cuda()
    exact = {}
    for side, nm, rng_fn, ids in ((_ffi.SIDE_S, "s", fi.subject_ranges, fi.s_ids), (_ffi.SIDE_O, "o", fi.object_ranges, fi.o_ids)):
        lo, hi = rng_fn(test)
        flt = (torch.as_tensor(lo).cuda(), torch.as_tensor(hi).cuda(), torch.as_tensor(ids).cuda())
        ranks, counts, sub = eng.rank_side(Xd, side, "worst", flt)
        oc, ctx = RO.side_counts("RotatE", nm, ent, rel, test, R)
        osub = RO.filter_sub(ctx, [ids[a:b] for a, b in zip(lo, hi)])
        assert np.array_equal(counts.cpu().numpy(), oc), (nm, int((counts.cpu().numpy() != oc).sum()))
        assert np.array_equal(sub.cpu().numpy(), osub), nm
        assert np.array_equal(ranks.cpu().numpy(), oc.sum(1) - osub + 1), nm
        assert len(np.unique(oc[:, 0])) > n // 4   # a real ranking problem
        exact[nm] = (counts.cpu().numpy(), flt)
    try:
        _ffi.check(gpu_lib.amdkge_set_rank_rotate_fast(1))
        for side, nm in ((_ffi.SIDE_S, "s"), (_ffi.SIDE_O, "o")):
            c_fast = eng.rank_side(Xd, side, "worst", exact[nm][1])[1].cpu().numpy()
            d = np.abs(c_fast.astype(np.int64) - exact[nm][0])
            assert d.max() <= 3 and (d.sum(1) > 0).mean() < 0.2, (nm, int(d.max()), float((d.sum(1) > 0).mean()))
    finally:
        gpu_lib.amdkge_set_rank_rotate_fast(0)


@pytest.mark.parametrize("deterministic", [False, True])
def test_fullsize_rotate_alternating_batch_sizes_share_one_workspace(gpu_lib, deterministic):
    """fit() ends every epoch with a short batch.  For RotatE k = 200 on 14 505 entities the plan of the owner-computes pair
    differs between B = 10 000 (own rows cached in LDS: twice the tiles) and the epoch's last 2 115 positives, so the bucket
    lists of one plan lie where the other keeps its counters: every step of an alternating sequence on ONE engine
    (one workspace) must still produce the gradients of the independent atomic-scatter kernel."""
    model, k, eta, N, R = "RotatE", 200, 20, 14505, 237
    eng = _engine(model, k, N, R)
    ld = _loss("self_adversarial")
    from ampligraph_amd import _ffi

    opt = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1)
    eng.prepare_training("adam")
    for step, B in enumerate([10000, 2115, 10000, 2115, 300, 10000]):
        X = _triples(B, N, R, seed=10 + step)
        eng.g_flat.zero_()
        eng.loss_acc.zero_()
        eng.train_fwdbwd(X, eta, ld, 5, step)
        l1, ge1, gr1 = float(eng.loss_acc[0]), eng.g_ent.clone(), eng.g_rel.clone()
        eng.g_flat.zero_()
        eng.loss_acc.zero_()
        eng.train_step_tiled(X, eta, ld, opt, 5, step, grad_only=True, deterministic=deterministic)
        torch.cuda.synchronize()
        assert abs(l1 - float(eng.loss_acc[0])) <= 2e-5 * abs(l1), (step, B)
        assert _rotate_rows_close(eng.g_ent, ge1, 2e-4) and _rows_close(eng.g_rel, gr1, 2e-4), (step, B)
        if deterministic:
            assert eng.tiled_status() == 0


def test_fullsize_c1_steps_bitwise_against_the_ordered_oracle(gpu_lib):
    """BASELINE configs[0] at FULL size -- TransE k = 50 (stored as 52 units), eta = 5, pairwise loss, Adam, the FB15K-237 shape,
    B = 10 000 -- three whole steps of the product's StepLoop (the atomic-scatter kernels and the dense sweep: what C1 takes) against
    oracle/train_ordered.py: BOTH tables and both Adam slots bit-identical, the loss to 1e-12.  (Integer-valued gradients: the order
    of 200 000 atomic row-adds does not matter; the score tree, the hinge and the update arithmetic do.)"""
    import torch

    from oracle import train_ordered as TO

    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    d = make_synthetic_kg("synth-fb15k237", seed=0)
    N, R, k, B, eta = d["n_ents"], d["n_rels"], 50, 10000, 5
    rng = np.random.default_rng(1)
    lim_e, lim_r = np.sqrt(6.0 / (N + k)), np.sqrt(6.0 / (R + k))
    ent = rng.uniform(-lim_e, lim_e, size=(N, k)).astype(np.float32)
    rel = rng.uniform(-lim_r, lim_r, size=(R, k)).astype(np.float32)
    eng = KgeEngine("TransE", k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    loop = StepLoop(eng, eta, loss_functions.get("pairwise"), optimizers.get("adam", {"learning_rate": 1e-2}), None, seed=3, dist=None)
    # the oracle works on the STORED rows (k = 50 padded to 52 units: the padding is inert but takes part in the lane layout)
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 2), np.float32)], 1)   # noqa: E731
    st = TO.OptState(pad(ent), pad(rel), "adam", 1e-2)
    X = d["train"]
    Xd = torch.as_tensor(X).cuda()
    loop.reset_loss()
    ref = 0.0
    for step in range(3):
        loop.step(Xd[step * B:(step + 1) * B], step)
        ref += TO.transe_pairwise_step(st, X[step * B:(step + 1) * B], eta, 3, step, layout="unit")   # (52 stored units <= 128: one unit per lane)
    torch.cuda.synchronize()
    got = loop.mean_batch_loss() * 3
    e, r = eng.get_tables()
    assert np.array_equal(e, st.ent[:, :k]) and np.array_equal(r, st.rel[:, :k]), (int((e != st.ent[:, :k]).sum()), int((r != st.rel[:, :k]).sum()))
    assert np.array_equal(eng.unpack(eng.slots["m_e"]).cpu().numpy(), st.s0[0][:, :k]) and np.array_equal(eng.unpack(eng.slots["v_e"]).cpu().numpy(), st.s1[0][:, :k])
    assert np.all(st.ent[:, k:] == 0) and within("fullsize/c2_det_vs_ordered_oracle/loss", rel_gap(got, ref), 1e-12), (got, ref)


@pytest.mark.gpu
def test_fullsize_c2_deterministic_steps_bitwise_against_the_ordered_oracle(gpu_lib):
    """BASELINE configs[1] -- the headline workload -- at FULL size: ComplEx k = 200, eta = 20, self-adversarial loss, Adam, the
    FB15K-237 shape, B = 10 000, in DETERMINISTIC mode: two whole steps of the product's StepLoop (the owner-computes pair with
    sorted tile sums and the batch-ordered relation gradient) against oracle/train_ordered.trilinear_step_det -- 210 000 scores by
    fmaf chains, the online softmax over 20 corruptions in groups of 6, 230 000 tile entries in sorted order, the dense Adam sweep:
    BOTH tables and both Adam slots bit-identical, the loss to 1e-12."""
    import torch

    from oracle import train_ordered as TO

    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    d = make_synthetic_kg("synth-fb15k237", seed=0)
    N, R, k, B, eta = d["n_ents"], d["n_rels"], 200, 10000, 20
    rng = np.random.default_rng(2)
    lim_e, lim_r = np.sqrt(6.0 / (N + 2 * k)), np.sqrt(6.0 / (R + 2 * k))
    ent = rng.uniform(-lim_e, lim_e, size=(N, 2 * k)).astype(np.float32)
    rel = rng.uniform(-lim_r, lim_r, size=(R, 2 * k)).astype(np.float32)
    eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
    eng.set_tables(ent, rel)
    loop = StepLoop(eng, eta, loss_functions.get("self_adversarial"), optimizers.get("adam", {"learning_rate": 1e-3}), None, seed=4, dist=None)
    loop.deterministic = True
    st = TO.OptState(ent.copy(), rel.copy(), "adam", 1e-3)
    X = d["train"]
    Xd = torch.as_tensor(X).cuda()
    loop.reset_loss()
    ref = 0.0
    for step in range(2):
        loop.step(Xd[step * B:(step + 1) * B], step)
        ref += TO.trilinear_step_det("ComplEx", st, X[step * B:(step + 1) * B], eta, 4, step, "self_adversarial")
    torch.cuda.synchronize()
    got = loop.mean_batch_loss() * 2
    e, r = eng.get_tables()
    assert np.array_equal(e, st.ent) and np.array_equal(r, st.rel), (int((e != st.ent).sum()), int((r != st.rel).sum()))
    assert np.array_equal(eng.unpack(eng.slots["m_e"]).cpu().numpy(), st.s0[0]) and np.array_equal(eng.unpack(eng.slots["v_e"]).cpu().numpy(), st.s1[0])
    assert within("fullsize/c5w_det_vs_ordered_oracle/loss", rel_gap(got, ref), 1e-12), (got, ref)
