"""The device KMeans on the MI355X (kge_kmeans.hip, engine.kmeans / kmeans_assign, discovery.KMeans): the assignment against fp64 brute
force over every tile edge, the three centre-tile widths and the batched runs bit for bit, single Lloyd iterations against exact means
(dyadic tables: tests/test_kmeans_host.py), whole runs against sklearn on tables whose trajectories stay clear of ties, chunking,
determinism, the stop rules, the seeding, the estimator and find_clusters."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_kmeans_host import WHOLE_RUN_SHAPES, clean_case, dyadic_mixture, lloyd_ref, start_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAND = 1e-4   # relative gap below which the fp32 chain may order two centres differently: (d + 2) 2^-24 is below it for d <= 1200


def _engine():
    from ampligraph_amd.engine import KgeEngine

    return KgeEngine("DistMult", 4, 4, 2)


def _centres(k, d, seed):
    return (2.0 * np.random.default_rng(seed).normal(size=(k, d))).astype(np.float32)


def _table(Cn, n, seed):
    """Gaussian rows with every third row integer-valued (the style of test_gpu_clusters._table), drawn around the centres they are
    assigned to: row = a centre + N(0, sigma), sigma one of 0.05 / 0.3 / 1.0 per row.  In the wide shapes the distances of a row to
    centres that have nothing to do with it concentrate -- against 2 N(0, 1) centres alone 0.4 to 1.2 % of such rows have their two
    nearest centres within 1e-4 of each other, in fp64 --; a row near one of the centres has a nearest centre to speak of, and with
    enough rows every centre is some row's nearest, so every position of every centre tile is a label that must come out."""
    rng = np.random.default_rng(seed)
    k, d = Cn.shape
    X = (Cn[rng.integers(0, k, n)] + rng.normal(size=(n, d)) * rng.choice([0.05, 0.3, 1.0], size=(n, 1))).astype(np.float32)
    X[::3] = np.round(X[::3])
    return X


def _d2(X, Cn, device="cuda"):
    """fp64 squared distances [n, k] in the direct form (a few rows at a time), as a torch tensor on `device`."""
    x = torch.as_tensor(np.asarray(X), dtype=torch.float64, device=device)
    c = torch.as_tensor(np.asarray(Cn), dtype=torch.float64, device=device)
    step = max(1, (1 << 24) // max(c.numel(), 1))
    return torch.cat([((x[i:i + step, None, :] - c[None, :, :]) ** 2).sum(-1) for i in range(0, len(x), step)])


def _check_assign(X, Cn, labels, mind2, what, max_band=0.01):
    """The labels equal the fp64 argmin on every row whose two nearest centres differ by more than BAND (relative); a row inside the band
    carries one of the centres within it; at most max_band of the rows are inside; mind2 is within the chain bound of the fp64 distance
    to the centre the row carries.  -> the fp64 distances to the carried centres (numpy)."""
    D = _d2(X, Cn)
    n, k = D.shape
    d = X.shape[1]
    lab = torch.as_tensor(np.asarray(labels), device=D.device).to(torch.int64)
    assert int(lab.min()) >= 0 and int(lab.max()) < k, what
    best, arg = D.min(1)
    if k > 1:
        second = torch.topk(D, 2, dim=1, largest=False).values[:, 1]
        clear = (second - best) > BAND * second
    else:
        clear = torch.ones(n, dtype=torch.bool, device=D.device)
    own = D[torch.arange(n, device=D.device), lab]
    in_band = int((~clear).sum())
    wrong_clear = int((clear & (lab != arg)).sum())
    outside = int(((own - best) > BAND * own).sum())
    m2 = torch.as_tensor(np.asarray(mind2), device=D.device).to(torch.float64)
    err = float(((m2 - own).abs() / torch.where(own > 0, own, torch.ones_like(own))).max())
    print("%s: rows in the tie band %d of %d, clear rows with another label %d, carried centres outside the band %d, mind2 rel err %.3g (bound %.3g)" % (
        what, in_band, n, wrong_clear, outside, err, (d + 2) * U))
    assert in_band <= max_band * n, what
    assert wrong_clear == 0 and outside == 0, what
    assert bool(((m2 - own).abs() <= (d + 2) * U * own).all()), what
    return own.cpu().numpy()


NS, DS, KS = (1, 2, 127, 128, 129, 1000, 4097), (1, 3, 4, 10, 400, 1200), (1, 2, 6, 8, 9, 33, 129, 300)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_assign_matches_fp64_brute_force(gpu_lib, n, d):
    eng = _engine()
    for k in [k for k in KS if k <= n]:
        Cn = _centres(k, d, 1000 * k + n + d)
        X = _table(Cn, n, 11 * n + d)
        Xd = torch.as_tensor(X).cuda()
        labels, mind2 = eng.kmeans_assign(Xd, torch.as_tensor(Cn).cuda())
        assert labels.dtype == torch.int32 and mind2.dtype == torch.float32 and labels.is_cuda and labels.shape == (n,) and mind2.shape == (n,)
        _check_assign(X, Cn, labels.cpu().numpy(), mind2.cpu().numpy(), "n %d d %d k %d" % (n, d, k))
        if d >= 10 and n >= 10 * k:
            assert len(np.unique(labels.cpu().numpy())) == k   # (every centre is some row's nearest: every tile position comes out)


@pytest.mark.parametrize("d", [1, 3, 4, 400])
def test_assign_exact_ties_go_to_the_lowest_centre(gpu_lib, d):
    """Integer-valued rows and centres (every distance an exact small integer, in fp32 as in fp64) with duplicated centres: np.argmin's label
    and the exact distance on every row."""
    eng = _engine()
    rng = np.random.default_rng(d)
    n = 1000
    X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    ties = 0
    for k in (2, 6, 9, 33, 129, 300):
        Cn = rng.integers(-2, 3, size=(k, d)).astype(np.float32)
        Cn[(k + 1) // 2:] = Cn[:k // 2]   # the first k // 2 centres twice (the later copies must never be chosen)
        D = _d2(X, Cn).cpu().numpy()
        labels, mind2 = eng.kmeans_assign(torch.as_tensor(X).cuda(), torch.as_tensor(Cn).cuda())
        assert np.array_equal(labels.cpu().numpy(), D.argmin(1)) and np.array_equal(mind2.cpu().numpy().astype(np.float64), D.min(1)), (d, k)
        ties += int(((D == D.min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties >= 5 * n   # (nearly every row of every case has an exact tie: at least the duplicate of its centre)


@pytest.mark.parametrize("d", [10, 400])
def test_tile_variants_agree(gpu_lib, d):
    """The same rows and centres, padded with far-away centres so that k crosses each tile-width threshold (8 | 32 | 128 centres per tile),
    and the scalar-load path (a matrix that is not 16-byte aligned) beside the vector one: bit-identical labels and mind2."""
    eng = _engine()
    n = 1000
    Cn = _centres(6, d, 5)
    X = _table(Cn, n, 3)
    Xd = torch.as_tensor(X).cuda()
    base_l, base_m = eng.kmeans_assign(Xd, torch.as_tensor(Cn).cuda())
    _check_assign(X, Cn, base_l.cpu().numpy(), base_m.cpu().numpy(), "d %d k 6" % d)
    shifted = torch.empty(n * d + 1, dtype=torch.float32, device="cuda")[1:].view(n, d)
    shifted.copy_(Xd)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for k in (7, 8, 9, 32, 33, 128, 129, 300):
        pad = np.full((k - 6, d), 1000.0, dtype=np.float32) + np.arange(k - 6, dtype=np.float32)[:, None]
        Ck = torch.as_tensor(np.concatenate([Cn, pad])).cuda()
        for rows in (Xd, shifted):
            l, m = eng.kmeans_assign(rows, Ck)
            assert torch.equal(l, base_l) and torch.equal(m, base_m), (d, k, rows is shifted)
    # the real centres behind the padding: labels move by the offset, the distances keep their bits
    front = torch.as_tensor(np.concatenate([np.full((40, d), 1000.0, dtype=np.float32), Cn])).cuda()
    l, m = eng.kmeans_assign(Xd, front)
    assert torch.equal(l, base_l + 40) and torch.equal(m, base_m)


def test_batched_runs_equal_single_runs(gpu_lib):
    eng = _engine()
    lengths = []
    for n, d, k in ((1000, 3, 6), (777, 16, 33), (515, 10, 129)):
        X = dyadic_mixture(n, d, k, 0.3, 1)
        Xd = torch.as_tensor(X).cuda()
        C0 = torch.as_tensor(np.stack([start_rows(X, k, s) for s in range(5)])).cuda()
        L, M = eng.kmeans_assign(Xd, C0)
        assert L.shape == (5, n) and M.shape == (5, n)
        whole = eng.kmeans(Xd, C0, 40, 0.0)
        lengths.append({int(v) for v in whole[3].tolist()})
        for r in range(5):
            l, m = eng.kmeans_assign(Xd, C0[r])
            assert torch.equal(l, L[r]) and torch.equal(m, M[r]), (n, d, k, r)
            single = eng.kmeans(Xd, C0[r:r + 1], 40, 0.0)
            for a, b in zip(single, whole):
                assert torch.equal(a[0], b[r]), (n, d, k, r)
    assert max(len(s) for s in lengths) > 1   # (runs of different lengths shared the launches)
    # groups: a workspace bound below one run's need puts every run in its own group
    eng2 = _engine()
    eng2.KMEANS_WORK_BYTES = 1
    for a, b in zip(eng2.kmeans(Xd, C0, 40, 0.0), whole):
        assert torch.equal(a, b)


class _Lloyd:
    """amdkge_kmeans_lloyd driven directly: one run whose state, labels and workspace persist from call to call."""

    def __init__(self, lib, X, C0):
        self.lib = lib
        self.X = torch.as_tensor(X).cuda().contiguous()
        self.C = torch.as_tensor(C0, dtype=torch.float32).cuda().clone().contiguous()
        self.n, self.d = self.X.shape
        self.k = self.C.shape[0]
        self.labels = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.mind2 = torch.zeros(self.n, dtype=torch.float32, device="cuda")
        self.state = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.inertia = torch.zeros(1, dtype=torch.float64, device="cuda")
        nbytes = lib.amdkge_kmeans_workspace_bytes(self.n, self.d, self.k, 1)
        assert nbytes > 0
        self.work = torch.full((nbytes // 4,), 0x55555555, dtype=torch.int32, device="cuda")   # (not zeroed: the call must not rely on it)

    def step(self, iters, tol_abs=0.0):
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        rc = self.lib.amdkge_kmeans_lloyd(p(self.X), self.n, self.d, p(self.C), self.k, 1, iters, float(tol_abs), p(self.labels), p(self.mind2),
                                          p(self.state), p(self.inertia), p(self.work), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.lib.amdkge_last_error()
        torch.cuda.synchronize()

    def counts(self):
        """the last iteration's counts: the third part of the workspace (include/amdkge.h), every part on an 8-byte boundary"""
        at = ((4 * self.k + 7) // 8 * 8 + 8) // 4
        return self.work[at:at + self.k].cpu().numpy()

    def snapshot(self):
        return [t.clone() for t in (self.C, self.labels, self.mind2, self.state, self.inertia)]


@pytest.mark.parametrize("shape", [(1000, 3, 6), (4097, 4, 9), (2000, 400, 6), (4097, 10, 33), (4097, 16, 129)])
def test_single_lloyd_iterations_are_exact(gpu_lib, shape):
    """iters = 1 from the device's own centres.  Whole trajectories of these tables pass through near-ties (relative gaps of 1e-5 and less,
    below the fp32 bound), so each iteration is held to what must be true of it: labels within the tie band of the centres it started
    from, centres = the exact means of the rows by THOSE labels (bit for bit: the tables' sums are exact), exact counts and control."""
    n, d, k = shape
    X = dyadic_mixture(n, d, k, 0.3, 7)
    run = _Lloyd(gpu_lib, X, start_rows(X, k, 7))
    X64 = X.astype(np.float64)
    prev_labels = np.full(n, -1)
    for it in range(1, 9):
        C_before = run.C.cpu().numpy()
        run.step(1)
        labels, C_after, state = run.labels.cpu().numpy(), run.C.cpu().numpy(), run.state.cpu().numpy()
        # (the table's rows are dyadic; the centres are means: ties in the fp64 distances are as rare as in any real table)
        own = _check_assign(X, C_before, labels, run.mind2.cpu().numpy(), "shape %s iteration %d" % (shape, it))
        counts = np.bincount(labels, minlength=k)
        sums = np.zeros((k, d))
        np.add.at(sums, labels, X64)
        assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)   # exact in fp32, as the generator promises
        want = np.where(counts[:, None] > 0, sums.astype(np.float32) / np.maximum(counts, 1).astype(np.float32)[:, None], C_before).astype(np.float32)
        assert np.array_equal(C_after.view(np.uint32), want.view(np.uint32)), (shape, it, int((C_after != want).sum()))
        assert np.array_equal(run.counts(), counts)
        changed = int((labels != prev_labels).sum())
        moved = not np.array_equal(C_after, C_before)
        assert state[0] == it and state[2] == changed and state[1] == (1 if it > 1 and changed == 0 else 0 if moved else 2), (shape, it, state)
        inertia = float(run.inertia.item())
        print("  inertia %.9g against fp64 %.9g, changed %d" % (inertia, own.sum(), changed))
        assert abs(inertia - own.sum()) <= 1e-6 * own.sum()
        prev_labels = labels
        if state[1]:
            break
    assert it >= 2


@pytest.mark.parametrize("sigma", [0.1, 0.3])
@pytest.mark.parametrize("shape", WHOLE_RUN_SHAPES)
def test_whole_runs_match_sklearn(gpu_lib, shape, sigma):
    from sklearn.cluster import KMeans as SkKMeans

    n, d, k = shape
    found = clean_case(n, d, k, sigma)
    assert found is not None, "no seed in range(20) gives a trajectory of 3 iterations with every gap above 1e-3"
    seed, X, C0, traj = found
    want = SkKMeans(n_clusters=k, init=C0.astype(np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(X.astype(np.float64))
    assert want.n_iter_ == traj["n_iter"] and np.array_equal(want.labels_, traj["labels"])   # (the rule of the host tests, once more)
    centres, labels, inertia, n_iter, done = _engine().kmeans(torch.as_tensor(X).cuda(), torch.as_tensor(C0)[None].cuda(), 300, 0.0)
    print("shape %s sigma %g seed %d: %d iterations (sklearn %d), min gap %.3g, label mismatches %d, centre err %.3g, inertia rel err %.3g" % (
        shape, sigma, seed, int(n_iter[0]), want.n_iter_, traj["min_gap"], int((labels[0].cpu().numpy() != want.labels_).sum()),
        np.abs(centres[0].cpu().numpy() - want.cluster_centers_).max(), abs(float(inertia[0]) - want.inertia_) / want.inertia_))
    assert np.array_equal(labels[0].cpu().numpy(), want.labels_)
    assert int(n_iter[0]) == want.n_iter_ and int(done[0]) == 1
    assert np.abs(centres[0].cpu().numpy().astype(np.float64) - want.cluster_centers_).max() <= 1e-6
    assert abs(float(inertia[0]) - want.inertia_) <= 1e-5 * want.inertia_


def _case(n=1500, d=10, k=6, runs=3):
    X = dyadic_mixture(n, d, k, 0.3, 2)
    return torch.as_tensor(X).cuda(), torch.as_tensor(np.stack([start_rows(X, k, s) for s in range(runs)])).cuda(), X


def test_chunking_and_idempotence(gpu_lib):
    eng = _engine()
    Xd, C0, X = _case()
    base = eng.kmeans(Xd, C0, 60, 0.0, check_every=8)
    assert bool((base[4] == 1).all()) and int(base[3].max()) >= 3 and int(base[3].max()) < 60
    for every in (1, 3):
        for a, b in zip(eng.kmeans(Xd, C0, 60, 0.0, check_every=every), base):
            assert torch.equal(a, b), every
    # a limit in the middle of a chunk: no run goes beyond it
    cut = eng.kmeans(Xd, C0, 2, 0.0, check_every=8)
    assert cut[3].tolist() == [2, 2, 2]
    # more iterations enqueued after the stop change nothing
    run = _Lloyd(gpu_lib, X, C0[0].cpu().numpy())
    run.step(60)
    assert int(run.state[1]) == 1 and int(run.state[0]) == int(base[3][0]) and torch.equal(run.C, base[0][0]) and torch.equal(run.labels, base[1][0])
    assert float(run.inertia) == float(base[2][0])
    before, counts = run.snapshot(), run.counts()
    run.step(5)
    run.step(0)   # (the refresh leaves a run that stopped on equal labels alone)
    for a, b in zip(run.snapshot(), before):
        assert torch.equal(a, b)
    assert np.array_equal(run.counts(), counts)


def test_two_calls_are_bit_identical(gpu_lib):
    eng = _engine()
    for n, d, k in ((1500, 10, 6), (4097, 16, 129), (2000, 400, 6)):
        X = dyadic_mixture(n, d, k, 0.3, 3) + np.float32(1.0 / 3.0)   # (off the dyadic grid: the sums round, and must round alike)
        Xd = torch.as_tensor(X).cuda()
        C0 = torch.as_tensor(np.stack([start_rows(X, k, s) for s in range(3)])).cuda()
        a, b = eng.kmeans(Xd, C0, 30, 1e-7), _engine().kmeans(Xd, C0, 30, 1e-7)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (n, d, k)
        assert not bool(torch.isnan(a[0]).any()) and bool((a[3] >= 1).all())


def test_stop_rules_and_the_empty_cluster(gpu_lib):
    eng = _engine()
    Xd, C0, X = _case()
    # a huge tolerance: one iteration, done == 2, labels and inertia of the final centres
    centres, labels, inertia, n_iter, done = eng.kmeans(Xd, C0, 300, 1e30)
    assert n_iter.tolist() == [1, 1, 1] and done.tolist() == [2, 2, 2]
    l, m = eng.kmeans_assign(Xd, centres)
    assert torch.equal(l, labels)
    assert torch.allclose(inertia, m.double().sum(1), rtol=1e-9, atol=0.0)
    for r in range(3):
        ref = lloyd_ref(X, C0[r].cpu().numpy(), tol_abs=1e30)
        assert ref["done"] == 2 and np.abs(centres[r].cpu().numpy() - ref["centres"]).max() <= 1e-5
    # max_iter
    centres, labels, inertia, n_iter, done = eng.kmeans(Xd, C0, 2, 0.0)
    want_done = [lloyd_ref(X, C0[r].cpu().numpy(), max_iter=2)["done"] for r in range(3)]   # (a run may stop on equal labels at 2)
    assert n_iter.tolist() == [2, 2, 2] and done.tolist() == want_done and 0 in want_done
    l, m = eng.kmeans_assign(Xd, centres)
    assert torch.equal(l, labels) and torch.allclose(inertia, m.double().sum(1), rtol=1e-9, atol=0.0)
    # a centre far from every row: no rows, its bits stay, nothing turns NaN
    far = torch.cat([C0[:1], torch.full((1, 1, C0.shape[2]), 12345.678, device="cuda")], 1)
    centres, labels, inertia, n_iter, done = eng.kmeans(Xd, far, 300, 0.0)
    assert torch.equal(centres[0, -1], far[0, -1]) and int((labels == far.shape[1] - 1).sum()) == 0
    assert not bool(torch.isnan(centres).any()) and bool(torch.isfinite(inertia).all()) and int(done[0]) == 1
    alone = eng.kmeans(Xd, C0[:1], 300, 0.0)
    assert torch.equal(alone[0][0], centres[0, :-1]) and torch.equal(alone[1], labels) and torch.equal(alone[3], n_iter)


def test_kmeans_plusplus_seeding(gpu_lib):
    from ampligraph_amd.discovery import KMeans, _kmeans_plusplus

    eng = _engine()
    k, per, d = 7, 40, 5
    rng = np.random.default_rng(0)
    groups = rng.normal(size=(k, d)).astype(np.float32)
    X = np.repeat(groups, per, axis=0)[rng.permutation(k * per)]
    Xd = torch.as_tensor(X).cuda()
    for seed in range(8):
        c = _kmeans_plusplus(eng, Xd, k, 4, seed)
        assert c.shape == (4, k, d) and c.is_cuda
        for run in c.cpu().numpy():
            # k distinct groups of exact duplicates: D^2 sampling gives a chosen group probability 0; every centre is a row, bit for bit
            assert len({r.tobytes() for r in run}) == k and all(any(np.array_equal(r, g) for g in groups) for r in run), seed
        assert torch.equal(c, _kmeans_plusplus(eng, Xd, k, 4, seed))
        assert torch.equal(c[:2], _kmeans_plusplus(eng, Xd, k, 2, seed))
    Y = torch.as_tensor(dyadic_mixture(3000, 16, 6, 0.3, 1)).cuda()
    c4, c2 = _kmeans_plusplus(eng, Y, 6, 4, 5), _kmeans_plusplus(eng, Y, 6, 2, 5)
    assert torch.equal(c4[:2], c2) and not torch.equal(c4[0], c4[1])
    rows = {r.tobytes() for r in Y.cpu().numpy()}
    assert all(r.tobytes() in rows for r in c4.reshape(-1, 16).cpu().numpy())
    a = KMeans(6, n_init=4, random_state=5).fit(Y, engine=eng)
    b = KMeans(6, n_init=4, random_state=5).fit(Y.cpu().numpy(), engine=eng)
    assert np.array_equal(a.cluster_centers_, b.cluster_centers_) and a.inertia_ == b.inertia_


def _blobs(n=3000, d=16, k=6, seed=0):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.normal(size=(k, d))
    planted = rng.integers(0, k, n)
    return (centres[planted] + 0.5 * rng.normal(size=(n, d))).astype(np.float32), planted


def test_estimator_matches_sklearn_on_planted_blobs(gpu_lib):
    from sklearn.cluster import KMeans as SkKMeans
    from sklearn.metrics import adjusted_rand_score

    from ampligraph_amd.discovery import KMeans

    X, planted = _blobs()
    km = KMeans(n_clusters=6, random_state=0)
    got = km.fit_predict(X)                      # numpy in, standalone, on the current GPU
    want = SkKMeans(n_clusters=6, n_init=10, random_state=0).fit(X.astype(np.float64))
    print("inertia %.9g, sklearn %.9g; iterations %d" % (km.inertia_, want.inertia_, km.n_iter_))
    assert got is km.labels_ and got.dtype == np.int32 and km.cluster_centers_.dtype == np.float32 and km.cluster_centers_.shape == (6, 16)
    assert adjusted_rand_score(planted, got) == 1.0
    assert abs(km.inertia_ - want.inertia_) <= 1e-5 * want.inertia_
    assert km.n_features_in_ == 16 and km.n_iter_ >= 2
    assert np.array_equal(km.predict(X), km.labels_) and np.array_equal(km.predict(torch.as_tensor(X).cuda()), km.labels_)
    again = KMeans(n_clusters=6, random_state=0).fit(torch.as_tensor(X).cuda())
    assert np.array_equal(again.labels_, km.labels_) and np.array_equal(again.cluster_centers_, km.cluster_centers_)
    assert again.inertia_ == km.inertia_ and again.n_iter_ == km.n_iter_
    with pytest.raises(ValueError):
        KMeans(n_clusters=6).fit(np.where(np.arange(X.size).reshape(X.shape) == 5, np.nan, X))
    with pytest.raises(ValueError):
        KMeans(n_clusters=4000).fit(X)


def test_estimator_with_an_explicit_init_reproduces_sklearn(gpu_lib):
    from sklearn.cluster import KMeans as SkKMeans

    from ampligraph_amd.discovery import KMeans

    n, d, k = WHOLE_RUN_SHAPES[1]
    seed, X, C0, traj = clean_case(n, d, k, 0.3)
    km = KMeans(n_clusters=k, init=C0, n_init=1, tol=0.0).fit(X)
    want = SkKMeans(n_clusters=k, init=C0.astype(np.float64), n_init=1, algorithm="lloyd", tol=0).fit(X.astype(np.float64))
    assert np.array_equal(km.labels_, want.labels_) and km.n_iter_ == want.n_iter_
    assert np.abs(km.cluster_centers_ - want.cluster_centers_).max() <= 1e-6 and abs(km.inertia_ - want.inertia_) <= 1e-5 * want.inertia_


# ------------------------------------------------------------------------------------------------------------- find_clusters
def _spies(m):
    calls = {"kmeans": [], "dbscan": []}
    real_k, real_d = m._engine.kmeans, m._engine.dbscan

    def kmeans(X, centres0, max_iter, tol_abs, check_every=8):
        calls["kmeans"].append((tuple(X.shape), tuple(centres0.shape), X.is_cuda))
        return real_k(X, centres0, max_iter, tol_abs, check_every)

    def dbscan(X, thr, min_samples):
        calls["dbscan"].append(1)
        return real_d(X, thr, min_samples)

    m._engine.kmeans, m._engine.dbscan = kmeans, dbscan
    return calls


@pytest.mark.parametrize("mode", ["e", "r", "t"])
def test_find_clusters_with_the_device_kmeans(gpu_lib, mode):
    from sklearn.cluster import KMeans as SkKMeans
    from test_gpu_clusters import _planted_model
    from test_gpu_duplicates import _inputs

    from ampligraph_amd.discovery import KMeans, find_clusters

    m, X = _planted_model(0)
    Xin, emb, _ = _inputs(m, X, mode)
    k = 2 if mode == "r" else 3
    calls = _spies(m)
    given = KMeans(n_clusters=k, n_init=4, random_state=3)
    got = find_clusters(Xin, m, given, mode=mode)
    assert calls["kmeans"] == [(emb.shape, (4, k, emb.shape[1]), True)] and calls["dbscan"] == []
    direct = KMeans(n_clusters=k, n_init=4, random_state=3).fit(emb)
    assert got.dtype == np.int64 and got.shape == (len(emb),) and np.array_equal(got, direct.labels_) and np.array_equal(got, given.labels_)
    assert np.array_equal(given.cluster_centers_, direct.cluster_centers_) and given.inertia_ == direct.inertia_
    # sklearn's own KMeans in the same session still runs on the host, with sklearn's labels
    host = find_clusters(Xin, m, SkKMeans(n_clusters=k, n_init=2, random_state=0), mode=mode)
    assert len(calls["kmeans"]) == 1 and np.array_equal(host, SkKMeans(n_clusters=k, n_init=2, random_state=0).fit_predict(emb))


def test_find_clusters_with_the_device_kmeans_row_sharded(gpu_lib):
    """Two row-sharded engines (in-process rendezvous) return the labels of the gathered table on both ranks."""
    from test_gpu_discovery import _fit_model
    from threaded_dist import ThreadedWorld

    from ampligraph_amd.discovery import KMeans, find_clusters

    def body(dist):
        m, X = _fit_model(dist, sharding=True)
        ents = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
        emb = m.get_embeddings(ents, "e")
        calls = _spies(m)
        got = find_clusters(ents, m, KMeans(n_clusters=3, n_init=3, random_state=1))
        return got, emb, len(calls["kmeans"])

    res = ThreadedWorld(2).run(body)
    for got, emb, n_calls in res:
        want = KMeans(n_clusters=3, n_init=3, random_state=1).fit(emb).labels_   # (the gathered table, fitted alone)
        assert n_calls == 1 and got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
