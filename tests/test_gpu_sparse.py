"""The sparse optimizer mode on the GPU (kge_opt_rows.hip, include/ext/amdkge_sparse.h):
  1. amdkge_step_rows against numpy's unique, ids and count exactly;
  2. amdkge_opt_step_rows against amdkge_opt_step with lazy = 1 on copies of the same table, gradient and slots: bit for bit;
  3. the invariant the mode rests on: after one backward call of each sampler, step_rows + opt_step_rows leave the tables and slots
     the whole-table lazy row sweep leaves, and a gradient table that is entirely zero;
  4. fit(): rows no step can touch keep their bits, fit() equals the steps written out with the engine, a planted graph learns."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_ref as SR
from test_gpu_kernels import dev, loss_desc, make_engine, rand_triples

pytestmark = pytest.mark.gpu

I32, I64, F32 = np.int32, np.int64, np.float32


# ------------------------------------------------------------------------------------------------------------------ 1. step_rows
def step_rows(N, X, ids, cap=None, expect=0):
    """amdkge_step_rows on exactly-sized buffers -> (rows[:n], n, the whole row buffer); expect: the return code"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    B, n_ids = len(X), len(ids)
    cap = min(2 * B + n_ids, N) if cap is None else cap
    rows = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    need = lib.amdkge_step_rows_workspace_bytes(N, 2 * B + n_ids)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    Xd, idd = (dev(X) if B else None), (dev(ids) if n_ids else None)
    rc = lib.amdkge_step_rows(N, Xd.data_ptr() if B else None, B, idd.data_ptr() if n_ids else None, n_ids, rows.data_ptr(), cap, cnt.data_ptr(),
                              work.data_ptr(), None)
    assert rc == expect, (rc, lib.amdkge_last_error())
    torch.cuda.synchronize()
    n = int(cnt.item())
    return rows.cpu().numpy()[:max(n, 0)], n, rows.cpu().numpy()


def triples(s, o):
    s, o = np.asarray(s, I32), np.asarray(o, I32)
    return np.stack([s, np.zeros_like(s), o], 1)


NO_X, NO_IDS = np.zeros((0, 3), I32), np.zeros(0, I32)


def test_step_rows_edges(gpu_lib):
    from ampligraph_amd import _ffi

    N = 1000
    for X, ids, want in ((triples([5], [3]), NO_IDS, [3, 5]), (triples([4], [4]), NO_IDS, [4]), (NO_X, np.array([9], I32), [9]),
                         (triples([7] * 6, [7] * 6), np.full(11, 7, I32), [7]), (triples([0], [N - 1]), np.array([N - 1, 0], I32), [0, N - 1]),
                         (NO_X, NO_IDS, [])):
        got, n, _ = step_rows(N, X, ids)
        assert n == len(want) and got.tolist() == want and got.dtype == I32
    # ids outside [0, n_ents) are skipped, wherever they sort
    got, n, _ = step_rows(N, triples([N, 2], [-1, N - 1]), np.array([2 ** 31 - 1, -(2 ** 31), 5], I32))
    assert got.tolist() == [2, 5, N - 1]
    # cap: exactly the bound passes (and is the bound whichever of the two is smaller); one short is an argument error
    X, ids = triples([1, 2, 3], [4, 5, 6]), np.array([7, 8], I32)
    assert step_rows(N, X, ids, cap=8)[1] == 8 and step_rows(5, X, ids, cap=5)[0].tolist() == [1, 2, 3, 4]
    for n_ents, cap in ((N, 7), (5, 4)):
        step_rows(n_ents, X, ids, cap=cap, expect=_ffi.EINVAL)
    # a buffer larger than the count: entries at and beyond n are not written
    got, n, whole = step_rows(N, triples([1, 1], [1, 2]), np.array([2, 2], I32), cap=6)
    assert got.tolist() == [1, 2] and (whole[2:] == -7).all()


@pytest.mark.parametrize("keys", [255, 256, 257, 4097, 70001])
def test_step_rows_is_numpys_unique(gpu_lib, keys):
    rng = np.random.default_rng(keys)
    for N in (keys // 3 + 2, 14505, 4_000_000):          # many duplicates (n_ents below the key count); few; hardly any
        B = int(rng.integers(1, keys // 2))
        X = rand_triples(rng, B, N, 5)
        ids = rng.integers(0, N, keys - 2 * B).astype(I32)
        got, n, _ = step_rows(N, X, ids)
        want = SR.candidate_rows(X, ids)
        assert n == want.size and np.array_equal(got, want), (keys, N)


def test_step_rows_needs_no_table(gpu_lib):
    """n_ents = 2^31 - 1 with every key in the top 2^16 ids: the call reads no table and its cost does not depend on n_ents"""
    N = 2 ** 31 - 1
    rng = np.random.default_rng(1)
    top = lambda n: (N - 1 - rng.integers(0, 1 << 16, n)).astype(I32)   # noqa: E731
    X, ids = triples(top(3000), top(3000)), top(4000)
    X[0, 0], ids[0] = N - 1, N - (1 << 16)
    got, n, _ = step_rows(N, X, ids)
    want = SR.candidate_rows(X, ids)
    assert n == want.size and np.array_equal(got, want) and got[-1] == N - 1 and got[0] == N - (1 << 16)


# ------------------------------------------------------------------------------------------------------------------ 2. opt_step_rows
HP = {"sgd": {}, "adagrad": {}, "adam": {}, "momentum": {"momentum": 0.9, "nesterov": True}, "rmsprop": {}, "rmsprop_mom": {"momentum": 0.5},
      "adadelta": {}, "adamax": {}}
REGS = {"": (2, 0.0, 2, 0.0), "p2": (2, 1e-2, 2, 0.0), "p3+p1": (3, 1e-2, 1, 1e-3)}


def descriptor(kind, rf, reg, lazy):
    from ampligraph_amd import _ffi
    from ampligraph_amd.latent_features import optimizers

    name = {"momentum": "sgd", "rmsprop_mom": "rmsprop"}.get(kind, kind)
    d = optimizers.get(name, dict(HP[kind], learning_rate=1e-2)).to_ffi(3)
    assert d.kind == _ffi.OPTIMIZERS[kind]
    d.reg_p, d.reg_lambda, d.reg2_p, d.reg2_lambda = reg
    d.lazy, d.row_floats = lazy, rf
    return d


def sweep_both(kind, rf, T, listed, hot, reg, extra=(), count=None):
    """A table of T rows of rf floats with a gradient on the rows `hot`.  (a) amdkge_opt_step(lazy = 1) over the whole table with the
    gradient of the rows that are NOT validly listed cleared beforehand; (b) amdkge_opt_step_rows on `listed` (+ `extra` entries
    behind the count) with the full gradient.  Asserts: x and both slots bit for bit; (b)'s gradient is zero on the listed rows and
    untouched elsewhere; reg_loss to 1e-5 of the value (tests/test_gpu_guard_bands.py case_opt_step's bar).  -> (x0, x after)"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    rng = np.random.default_rng(T * 31 + rf)
    x0 = (rng.normal(size=(T, rf)) * 0.5).astype(F32)
    g0 = np.zeros((T, rf), F32)
    g0[hot] = rng.normal(size=(len(hot), rf)).astype(F32)
    s00, s10 = (rng.random(size=(T, rf)) * 0.01 + 0.01).astype(F32), (rng.random(size=(T, rf)) * 0.01 + 0.01).astype(F32)
    listed = np.asarray(listed, I64)
    valid = listed[(listed >= 0) & (listed < T)]
    is_listed = np.zeros(T, bool)
    is_listed[valid] = True
    n_slots = len(_ffi.OPT_SLOTS[kind])
    out = {}
    for which in "ab":
        x, g, s0, s1 = dev(x0), dev(g0 if which == "b" else g0 * is_listed[:, None]), dev(s00), dev(s10)
        regl = torch.zeros(1, dtype=torch.float64, device="cuda")
        slots = (s0.data_ptr() if n_slots >= 1 else None, s1.data_ptr() if n_slots == 2 else None)
        if which == "a":
            _ffi.check(lib.amdkge_opt_step(C.byref(descriptor(kind, rf, reg, 1)), x.data_ptr(), g.data_ptr(), *slots, T * rf, regl.data_ptr(), None))
        else:
            lst = dev(np.concatenate([listed, np.asarray(extra, I64)]).astype(I32))
            cnt = dev(np.array([len(listed) if count is None else count], I64))
            _ffi.check(lib.amdkge_opt_step_rows(C.byref(descriptor(kind, rf, reg, 0)), x.data_ptr(), g.data_ptr(), *slots, T, lst.data_ptr(),
                                                cnt.data_ptr(), int(lst.numel()), regl.data_ptr(), None))
        torch.cuda.synchronize()
        out[which] = [t.cpu().numpy() for t in (x, s0, s1, g)] + [float(regl.item())]
    a, b = out["a"], out["b"]
    for name, u, v in zip(("x", "slot0", "slot1"), a[:3], b[:3]):
        assert np.array_equal(u.view(I32), v.view(I32)), (kind, rf, name, int((u.view(I32) != v.view(I32)).any(1).sum()))
    assert not a[3].any() and not b[3][is_listed].any() and np.array_equal(b[3][~is_listed].view(I32), g0[~is_listed].view(I32))
    assert abs(a[4] - b[4]) <= 1e-5 * abs(a[4]), (a[4], b[4])
    assert (a[4] > 0) == (reg[1] > 0 and bool(is_listed[hot].any()))
    moved = (b[0].view(I32) != x0.view(I32)).any(1)
    assert np.array_equal(moved, is_listed & (g0 != 0).any(1))          # a listed row without a gradient and a row that is not listed keep every bit
    for u, u0 in ((b[1], s00), (b[2], s10)):
        assert np.array_equal(u[~moved].view(I32), u0[~moved].view(I32))
    return x0, b[0]


def spread(T, n, seed=0):
    return np.sort(np.random.default_rng(seed).choice(T, n, replace=False))


@pytest.mark.parametrize("reg", list(REGS))
@pytest.mark.parametrize("kind", list(HP))
def test_opt_step_rows_is_the_lazy_sweep_bit_for_bit(gpu_lib, kind, reg):
    """the eight rules x the regulariser terms; the list is a strict superset of the rows with a gradient, one row with a gradient is
    not listed, the buffer is larger than the count with out-of-range garbage behind it"""
    T, rf = 300, 24
    hot = spread(T, 90, 1)
    listed = np.union1d(hot[1:], spread(T, 60, 2))
    listed = listed[listed != hot[0]]
    assert len(listed) > 89 and hot[0] not in listed
    sweep_both(kind, rf, T, listed, hot, REGS[reg], extra=[T + 5, -3, hot[0], 2 ** 31 - 1])


@pytest.mark.parametrize("rf", [4, 8, 256, 260, 2000])
def test_opt_step_rows_row_widths(gpu_lib, rf):
    T = 70
    hot = spread(T, 40, rf)
    sweep_both("adam", rf, T, np.union1d(hot, [0, T - 1]), hot, REGS["p3+p1"])
    sweep_both("adagrad", rf, T, hot[::2], hot, REGS["p2"])


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, "all"])
def test_opt_step_rows_list_lengths(gpu_lib, n):
    T, rf = 41, 12
    listed = np.arange(T) if n == "all" else spread(T, n, 5)
    sweep_both("adam", rf, T, listed, np.arange(T), REGS["p2"])
    sweep_both("sgd", rf, T, listed, np.arange(T), REGS["p2"], extra=[0, 1, 2])     # (the entries behind the count name real rows)


def test_opt_step_rows_more_rows_than_waves(gpu_lib):
    """70 000 listed rows of 4 floats: the grid holds 16 384 waves, every wave strides over several rows"""
    T = 90_000
    listed = spread(T, 70_000, 9)
    x0, x1 = sweep_both("adam", 4, T, listed, np.arange(0, T, 2), REGS["p2"])
    assert int((x0 != x1).any(1).sum()) > 25_000


def test_opt_step_rows_skips_what_is_out_of_range_and_reads_the_count_on_the_device(gpu_lib):
    T, rf = 50, 8
    hot = np.arange(T)
    sweep_both("adam", rf, T, [-(2 ** 31), -1, 3, 7, 49, 50, 2 ** 31 - 1], hot, REGS["p2"])       # inside the count: skipped
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    for count, want in ((-5, 0), (2, 2), (99, 4)):                                                 # a count beyond cap is cap, below zero is zero
        x, g = torch.ones(T, rf, device="cuda"), torch.ones(T, rf, device="cuda")
        lst, cnt = dev(np.array([1, 2, 3, 4], I32)), dev(np.array([count], I64))
        _ffi.check(lib.amdkge_opt_step_rows(C.byref(descriptor("sgd", rf, REGS[""], 0)), x.data_ptr(), g.data_ptr(), None, None, T, lst.data_ptr(),
                                            cnt.data_ptr(), 4, None, None))
        torch.cuda.synchronize()
        assert (x != 1).any(1).nonzero().flatten().tolist() == list(range(1, 1 + want))


# ------------------------------------------------------------------------------------------------------------------ 3. the invariant
# (name, model, k, B, G, M, masked, pool, all over the pool, relation term, N3)
STEPS = [("ComplEx", "ComplEx", 20, 50, 16, 33, False, False, False, False, False),      # a short last group: 50 = 3 * 16 + 2
         ("DistMult M=1", "DistMult", 7, 37, 8, 1, False, False, False, False, False),
         ("TransE", "TransE", 16, 50, 16, 33, False, False, False, False, False),
         ("RotatE M=1 masked", "RotatE", 10, 37, 8, 1, True, False, False, False, False),
         ("ComplEx masked pool", "ComplEx", 20, 50, 16, 33, True, True, False, False, False),
         ("DistMult all over a pool", "DistMult", 12, 50, 16, 40, True, True, True, False, False),
         ("TransE all over a pool", "TransE", 12, 37, 16, 40, False, True, True, False, False),
         ("ComplEx relation term", "ComplEx", 20, 50, 16, 33, False, False, False, True, False),
         ("DistMult N3", "DistMult", 20, 50, 16, 33, True, False, False, False, True)]


@pytest.mark.parametrize("name,model,k,B,G,M,masked,pool,all_list,relation,n3", STEPS, ids=[s[0] for s in STEPS])
def test_the_candidate_rows_cover_every_row_a_step_touches(gpu_lib, name, model, k, B, G, M, masked, pool, all_list, relation, n3):
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.latent_features import optimizers
    from ampligraph_amd.latent_features.negatives import BoundMaskedSharedNegatives, BoundSharedNegatives
    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer, LPRegularizer

    N, R = 400, 5
    eng, _, _ = make_engine(model, k, N, R)
    eng.prepare_training("adam")
    for t in eng.slot_flat.values():        # slots that are not zero: a row that must keep them shows when it does not
        t.copy_(torch.rand_like(t) * 1e-3)
    rng = np.random.default_rng(len(name))
    D = rand_triples(rng, 6 * N, N // 2, R)                     # the graph: the upper half of the entities occurs in no positive
    X = D[rng.integers(0, len(D), B)]
    Xd = dev(X)
    pl = dev(rng.choice(N, M, replace=False).astype(I32)) if pool else None
    al = pl if all_list else None
    distance = model in ("TransE", "RotatE")
    if masked:
        neg = BoundMaskedSharedNegatives(eng, M, G, "uniform", None, pl, al, train=Xd, index=FilterIndex([D], N, R, engine=eng), identity=False,
                                         distance=distance)
    else:
        neg = BoundSharedNegatives(eng, M, G, "uniform", None, pl, all_list=al, distance=distance)
    assert neg.names_rows
    neg.step(Xd, loss_desc("multiclass_nll" if all_list else "nll"), 11, 5)
    if relation:
        eng.train_relation_fwdbwd(Xd, loss_desc("multiclass_nll"), 0.25)
    if n3:
        eng.batch_reg_fwdbwd(Xd, BatchLPRegularizer(3, 0.05), BatchLPRegularizer(3, 0.05))
    lam = None if n3 else LPRegularizer(2, 1e-3)
    desc = optimizers.get("adam", {"learning_rate": 1e-2}).to_ffi(1, 2)
    torch.cuda.synchronize()
    keep = [t.clone() for t in (eng.p_flat, eng.g_flat, *eng.slot_flat.values())]
    reg_0 = float(eng.loss_acc[1].item())                       # (a batch regulariser's penalty shares the slot: the sweeps ADD to it)
    touched = (eng.g_ent != 0).any(1)
    assert 0 < int(touched.sum()) < N // 2 + M + 1 and bool((eng.g_rel != 0).any())
    # (b) the mode: the sampler's candidate rows, then the sweep of those rows
    rows, n_rows = neg.candidate_rows(Xd)
    eng.opt_step_rows(desc, lam, lam, rows, n_rows, int(rows.numel()))
    torch.cuda.synchronize()
    assert desc.lazy == 0
    n = int(n_rows.item())
    cand = rows[:n].cpu().numpy()
    ids_used = (al if all_list else neg._step_ids).cpu().numpy()
    assert np.array_equal(cand, SR.candidate_rows(X, ids_used)) and bool(touched[rows[:n].long()].sum() == touched.sum())
    got = [t.clone() for t in (eng.p_flat, *eng.slot_flat.values())]
    assert not bool(eng.g_flat.any()), "the gradient table is not all zero after the sparse sweep"
    reg_b = float(eng.loss_acc[1].item()) - reg_0
    # (a) the whole-table lazy row sweep on the same state
    for t, t0 in zip((eng.p_flat, eng.g_flat, *eng.slot_flat.values()), keep):
        t.copy_(t0)
    eng.loss_acc[1] = reg_0
    desc.lazy = 1
    eng.opt_step(desc, lam, lam)
    torch.cuda.synchronize()
    for what, u, v in zip(("tables", "slot 0", "slot 1"), got, (eng.p_flat, *eng.slot_flat.values())):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (name, what)
    assert bool((eng.ent != keep[0][:eng.ent.numel()].view_as(eng.ent)).any(1).sum() == touched.sum())       # and the sweep did something
    reg_a = float(eng.loss_acc[1].item()) - reg_0
    assert abs(reg_a - reg_b) <= 1e-5 * abs(reg_a), (reg_a, reg_b)


# ------------------------------------------------------------------------------------------------------------------ 4. fit()
def graph(n=900, N=120, R=3, seed=4):
    from test_gpu_model import toy_graph

    return toy_graph(seed=seed, n=n, N=N, R=R)


def test_fit_leaves_the_rows_no_step_can_touch(gpu_lib):
    """Adam and an LP regulariser with lambda > 0: the dense sweep moves every row of the table every step.  The last 50 entities of
    the id map occur in no training triple of the second fit() and are not in the pool: in sparse mode their rows of the table and of
    both slots keep their bits over 3 epochs; in dense mode they move."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    from ampligraph_amd.datasets.indexer import DataIndexer

    X = graph()
    labels = np.unique(np.concatenate([X[:, 0], X[:, 2]]))
    ents = labels[np.argsort(np.asarray(DataIndexer(X).get_indexes(labels, "e")))]      # the id map fit() builds: entity i is ents[i]
    last, rest = ents[-50:], ents[:-50]
    sub = X[~(np.isin(X[:, 0], last) | np.isin(X[:, 2], last))]
    assert 300 < len(sub) < len(X)
    out = {}
    for mode in ("sparse", "dense"):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="nll", entity_relation_regularizer="l2",
                  negatives={"shared": 24, "group_size": 16, "entities": rest}, optimizer_mode=mode)
        m.fit(X, batch_size=128, epochs=0, verbose=False)                 # the id map and the tables over ALL entities; no step
        idx = torch.as_tensor(np.asarray(m.data_indexer.get_indexes(last, "e"), dtype=np.int64)).cuda()
        assert sorted(idx.tolist()) == list(range(len(ents) - 50, len(ents))) and m._engine.n_ents == len(ents)
        eng = m._engine
        before = eng.ent.clone()
        h = m.fit(sub, batch_size=128, epochs=3, verbose=False)            # the same id map and tables: training continues
        assert m._engine is eng and m.optimizer.sparse is (mode == "sparse") and np.isfinite(h.history["loss"]).all()
        assert m.optimizer.iterations == 3 * -(-len(sub) // 128)
        assert bool(torch.isfinite(eng.ent).all()) and bool(torch.isfinite(eng.rel).all())
        moved_last = (eng.ent[idx].view(torch.int32) != before[idx].view(torch.int32)).any(1)
        slots_last = [bool((eng.slots[s][idx] != 0).any()) for s in ("m_e", "v_e")]
        moved_all = (eng.ent.view(torch.int32) != before.view(torch.int32)).any(1)
        out[mode] = (int(moved_last.sum()), slots_last, int(moved_all.sum()))
        assert not bool(eng.g_flat.any())                                 # either mode leaves the gradient tables zero between steps
    print("rows moved: last 50 / slots of the last 50 touched / all", out)
    assert out["sparse"][0] == 0 and out["sparse"][1] == [False, False] and 0 < out["sparse"][2] <= len(ents) - 50
    assert out["dense"][0] == 50 and out["dense"][1] == [True, True] and out["dense"][2] == len(ents)


@pytest.mark.parametrize("model,spec", [("ComplEx", {"shared": 48, "group_size": 20}), ("TransE", {"shared_distance": 24, "group_size": 20, "mask_known": True})],
                         ids=["ComplEx", "TransE masked"])
def test_fit_in_sparse_mode_equals_the_steps_written_out(gpu_lib, model, spec):
    """fit() against the sampler's step followed by the WHOLE-TABLE lazy row sweep, written out with the engine.  Both runs add their
    gradients with unordered atomics: the bars of test_gpu_shared.py::test_fit_with_shared_negatives_equals_fit_on_the_override_rows."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    X = graph(n=400, N=40)
    epochs, bs = 3, 128

    def new(**kw):
        m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type=model, seed=2)
        m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-2}), loss="multiclass_nll", entity_relation_regularizer="l2", negatives=dict(spec), **kw)
        return m

    m1 = new(optimizer_mode="sparse")
    h1 = m1.fit(X, batch_size=bs, epochs=epochs, verbose=False).history["loss"]
    m2 = new()
    m2.fit(X, batch_size=bs, epochs=0, verbose=False)                     # engine, loop and id map; no step
    eng, loop = m2._engine, m2._loop
    neg = loop.negatives                                                  # bound by fit() to its training tensor
    train = neg.train if hasattr(neg, "train") else torch.as_tensor(np.ascontiguousarray(m2.data_indexer.get_indexes(X), dtype=np.int32)).cuda()
    steps, h2 = -(-len(X) // bs), []
    for ep in range(epochs):
        eng.loss_acc.zero_()
        for s in range(steps):
            m2.optimizer.iterations += 1
            desc = m2.optimizer.to_ffi(m2.optimizer.iterations, 2)
            neg.step(train[s * bs:(s + 1) * bs], loop.loss_ffi, m2.seed, ep * steps + s)
            desc.lazy = 1
            eng.opt_step(desc, m2._regularizers[0], m2._regularizers[1])
        h2.append(float(eng.loss_acc.sum().item()) / steps)
    print("loss histories", h1, h2)
    assert len(h1) == epochs and np.allclose(h1, h2, rtol=2e-4)
    assert np.allclose(m1.predict(X[:80]), m2.predict(X[:80]), rtol=1e-3, atol=1e-4)
    assert not bool(m1._engine.g_flat.any())


def test_sparse_mode_learns_the_planted_graph_and_survives_a_round_trip(gpu_lib, tmp_path):
    from planted import planted_kg

    from ampligraph_amd.evaluation import mrr_score
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers
    from ampligraph_amd.latent_features.negatives import SharedNegatives
    from ampligraph_amd.utils.model_utils import restore_model, save_model

    kg = planted_kg("ComplEx", n_ents=120, n_rels=4, n_test=50, seed=0)
    X, T = kg["train"].astype(str), kg["test"].astype(str)
    m = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=0)
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": 2e-2}), loss="multiclass_nll", negatives={"shared": 32, "mask_known": True},
              optimizer_mode="sparse")
    h = m.fit(X, batch_size=256, epochs=15, verbose=False).history["loss"]
    save_model(m, str(tmp_path / "sparse"))
    r = restore_model(str(tmp_path / "sparse"))
    assert r.optimizer.sparse is True and isinstance(r._negatives, SharedNegatives) and r._negatives.get_config() == m._negatives.get_config()
    assert r.optimizer.iterations == m.optimizer.iterations and np.array_equal(r.predict(X[:20]), m.predict(X[:20]))
    h2 = r.fit(X, batch_size=256, epochs=15, verbose=False).history["loss"]      # continued training takes the sparse step again
    print("planted graph, epoch losses", h, h2)
    assert np.isfinite(h + h2).all() and h[-1] < h[0] and h2[-1] < h[-1]
    assert set(r.negative_sampling_stats_) == {"masked", "unmaskable"} and not bool(r._engine.g_flat.any())
    ranks = r.evaluate(T, batch_size=64, use_filter={"train": X, "test": T}, verbose=False)
    rnd = ScoringBasedEmbeddingModel(eta=2, k=16, scoring_type="ComplEx", seed=0)
    rnd.compile(optimizer="adam", loss="multiclass_nll")
    rnd.fit(X, batch_size=256, epochs=0, verbose=False)
    base = rnd.evaluate(T, batch_size=64, use_filter={"train": X, "test": T}, verbose=False)
    print("planted graph, filtered MRR", mrr_score(ranks), "untrained", mrr_score(base))
    assert mrr_score(ranks) > 2 * mrr_score(base)                          # "learns": at least twice the filtered MRR of the untrained tables
