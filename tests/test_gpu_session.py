"""The session layer of the C ABI (amdkge_session_*, host pointers in / out, all device state behind one handle) driven
with numpy only, against the oracle: what a host without torch gets from libamdkge."""
import numpy as np
import pytest

from margins import rel_gap, within
from oracle import kge_oracle as O

pytestmark = pytest.mark.gpu


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    ids = np.concatenate(lists).astype(np.int32) if off[-1] else np.zeros(0, dtype=np.int32)
    return off, ids


@pytest.mark.parametrize("model,k,opt", [("ComplEx", 8, "adam"), ("DistMult", 7, "adagrad"), ("TransE", 12, "sgd"),
                                         ("RotatE", 8, "rmsprop")])
def test_session_train_score_rank_against_oracle(gpu_lib, model, k, opt):
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.session import Session

    rng = np.random.default_rng(7)
    N, R, B, eta, seed = 90, 4, 150, 5, 11
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    X = np.stack([rng.integers(0, N, 3 * B), rng.integers(0, R, 3 * B), rng.integers(0, N, 3 * B)], 1).astype(np.int32)
    reg = regularizers.get("LP", {"p": 2, "lambda": 1e-3})
    s = Session(model, k, N, R, eta, loss_functions.get("nll"), optimizers.get(opt, {"learning_rate": 1e-2}), reg, seed=seed)
    if opt == "adagrad":   # Keras legacy initial accumulator
        assert np.all(s.get_rows("ent_slot0", row0=3, nrows=2) == np.float32(0.1))
    with pytest.raises(Exception):
        s.get_rows("ent_slot1" if opt != "adam" else "ent_slot0", ids=[N])   # no such state tensor / row outside the table
    s.set_rows("ent", ent)
    s.set_rows("rel", rel)
    assert np.array_equal(s.get_rows("ent", ids=[5, 0, 5]), ent[[5, 0, 5]]) and np.array_equal(s.get_rows("rel"), rel)
    st = O.TrainState(ent, rel, opt, 1e-2)
    for t in range(3):
        xb = X[t * B:(t + 1) * B]
        got = s.train_step(xb)
        ref = float(O.train_step(st, model, xb, eta, "nll", seed, t, max_rel_size=R, reg=dict(p=2, lam_e=1e-3, lam_r=1e-3)))
        assert abs(got - ref) <= 2e-5 * abs(ref), (t, got, ref)
    e, r = s.get_rows("ent"), s.get_rows("rel")
    assert np.mean(np.abs(e - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.995 and np.abs(e - st.ent).max() < 2.5e-2
    assert np.mean(np.abs(r - st.rel) <= 1e-5 + 1e-3 * np.abs(st.rel)) > 0.99
    # predict
    T = X[:40]
    ref_sc = O.compute_scores(model, *O.lookup(e, r, T.astype(np.int64)), max_rel_size=R)
    assert np.allclose(s.score(T), ref_sc, rtol=1e-5, atol=1e-5 * np.abs(ref_sc).max())
    assert s.score(T[:0]).shape == (0,)
    # evaluate: filtered, both sides / s+o / one side / subset, against the oracle on the session's own tables
    fs, fo = O.filter_sets(T, [X])
    ref = O.evaluate_ranks(model, e, r, T, fs, fo, "s,o", "worst", max_rel_size=R)
    got = s.rank(T, _csr(fs), _csr(fo), corrupt_side="s,o")
    assert got.shape == (40, 2) and (np.abs(got - ref) <= 1).mean() > 0.97
    if model != "RotatE":   # identical to the oracle's declared-order fp32 mode (RotatE: hardware cos / sin / sqrt)
        from oracle import rank_ordered as RO

        assert np.array_equal(got, RO.evaluate_ranks(model, e, r, T, fs, fo, "s,o", "worst", max_rel_size=R))
    both = s.rank(T, _csr(fs), _csr(fo), corrupt_side="s+o")
    assert both.shape == (40, 1) and np.array_equal(both[:, 0], got[:, 0] + got[:, 1] - 1)
    assert np.array_equal(s.rank(T, None, _csr(fo), corrupt_side="o")[:, 0], got[:, 1])
    unf = s.rank(T, corrupt_side="s", ranking_strategy="best")
    ref_unf = O.evaluate_ranks(model, e, r, T, None, None, "s", "best", max_rel_size=R)
    assert unf.shape == (40, 1) and (np.abs(unf - ref_unf.reshape(40, -1)) <= 1).mean() > 0.97
    sub = np.array([3, 17, 40, 41, 3, 88], dtype=np.int32)
    rs = s.rank(T, _csr(fs), _csr(fo), entities_subset=sub, corrupt_side="s,o")
    ref_sub = O.evaluate_ranks(model, e, r, T, fs, fo, "s,o", "worst", entities_subset=sub, max_rel_size=R)
    assert rs.max() <= len(sub) + 1 and rs.min() >= 1 and (np.abs(rs - ref_sub) <= 1).mean() > 0.97
    s.close()
    s.close()   # idempotent


def test_session_deterministic_and_hot_rows(gpu_lib):
    """cfg.flags = AMDKGE_TILED_DETERMINISTIC: two sessions fed the same steps hold bitwise equal tables; hot rows declared on a
    session give the same step as the default path up to fp32 summation order."""
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import Session

    rng = np.random.default_rng(3)
    N, R, k, B, eta = 120, 3, 10, 600, 4
    ent = (rng.normal(size=(N, 2 * k)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, 2 * k)) * 0.3).astype(np.float32)
    X = np.stack([rng.integers(0, N, 3 * B), rng.integers(0, R, 3 * B), rng.integers(0, N, 3 * B)], 1).astype(np.int32)
    X[::2, 0] = 5                                   # one hub entity
    outs = {}
    for name, kw, hot in (("det1", dict(deterministic=True), None), ("det2", dict(deterministic=True), None), ("plain", {}, None),
                          ("hot", {}, [5, 7])):
        s = Session("ComplEx", k, N, R, eta, loss_functions.get("self_adversarial"), optimizers.get("adam", {"learning_rate": 1e-2}), seed=1, **kw)
        s.set_rows("ent", ent)
        s.set_rows("rel", rel)
        if hot:
            s.set_hot_rows(hot)
        losses = [s.train_step(X[t * B:(t + 1) * B]) for t in range(3)]
        outs[name] = (s.get_rows("ent"), s.get_rows("rel"), s.get_rows("ent_slot1"), losses)
        s.close()
    for a, b in zip(outs["det1"][:3], outs["det2"][:3]):
        assert np.array_equal(a, b)
    for other in ("plain", "hot"):
        # default mode vs deterministic mode: hardware vs declared transcendentals at step 0 (~1e-7 per positive), then tables that
        # part by fp32 arrival order of the atomic row-adds under Adam; bar = the oracle's own (observed: profiles/r05_margins.json)
        assert within(f"session/{other}_vs_det/loss0", rel_gap(outs[other][3][0], outs["det1"][3][0]), 2e-6)
        assert within(f"session/{other}_vs_det/loss12", rel_gap(outs[other][3][1:], outs["det1"][3][1:]), 2e-5)
        assert np.mean(np.abs(outs[other][0] - outs["det1"][0]) <= 1e-5 + 1e-3 * np.abs(outs["det1"][0])) > 0.97
    with pytest.raises(Exception):
        s = Session("ComplEx", k, N, R, eta, loss_functions.get("nll"), optimizers.get("adam"))
        try:
            s.set_hot_rows([N + 3])
        finally:
            s.close()


@pytest.mark.parametrize("model,k,opt,n_rep", [("ComplEx", 8, "adam", 2), ("TransE", 12, "adagrad", 3), ("RotatE", 200, "adam", 2), ("DistMult", 600, "sgd", 4)])
def test_session_group_matches_single_session(gpu_lib, model, k, opt, n_rep):
    """amdkge_session_group_*: n replicas (here all on device 0: the gradient sum is the library's local kernel instead of
    ncclAllReduce -- everything else of the multi-GPU path) == one session on the whole batch == the oracle; the replicas stay
    bit-identical; a group of one is a plain session; RotatE k = 200 / DistMult k = 600 take the owner-computes pair in its
    gradient-only form (the second one its row-direct tile pass), TransE k = 12 the atomic path."""
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.session import Session, SessionGroup

    rng = np.random.default_rng(3)
    N, R, B, eta, seed = 120, 4, 301, 4, 5   # B not divisible by the replica count: ragged shares
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * (0.3 if k < 100 else 0.08)).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * (0.3 if k < 100 else 0.08)).astype(np.float32)
    X = np.stack([rng.integers(0, N, 3 * B), rng.integers(0, R, 3 * B), rng.integers(0, N, 3 * B)], 1).astype(np.int32)
    reg = regularizers.get("LP", {"p": 3, "lambda": 1e-3})
    mk = lambda: (loss_functions.get("self_adversarial"), optimizers.get(opt, {"learning_rate": 1e-2}))   # noqa: E731
    single = Session(model, k, N, R, eta, *mk(), reg, seed=seed)
    group = SessionGroup([0] * n_rep, model, k, N, R, eta, *mk(), reg, seed=seed)
    one = SessionGroup([0], model, k, N, R, eta, *mk(), reg, seed=seed)
    assert group.size == n_rep and one.size == 1
    for s in (single, group, one):
        s.set_rows("ent", ent)
        s.set_rows("rel", rel)
    st = O.TrainState(ent, rel, opt, 1e-2)
    for t in range(3):
        xb = X[t * B:(t + 1) * B]
        l1, lg, lo = single.train_step(xb), group.train_step(xb), one.train_step(xb)
        ref = float(O.train_step(st, model, xb, eta, "self_adversarial", seed, t, max_rel_size=R, reg=dict(p=3, lam_e=1e-3, lam_r=1e-3)))
        assert abs(lg - ref) <= 3e-5 * abs(ref) and abs(l1 - ref) <= 3e-5 * abs(ref) and abs(lo - ref) <= 3e-5 * abs(ref), (t, l1, lg, lo, ref)
        # a group of one IS a session (kge_session_group.hip).  What is invariant between two runs of the same code: step 0 starts
        # from the same tables, so the losses differ by the arrival order of the fp64 loss partials only (~1e-13); from step 1 on
        # the TABLES differ by the arrival order of fp32 atomic row-adds (TransE k = 12 takes the atomic path), and the
        # optimizer carries that into the loss (driver box, round 4: 1.06e-8 at step 2) -- each run is held to the oracle
        # above, the two runs to each other only as far as that noise allows.
        assert within(f"session/group_of_one/{model}/loss_step{min(t, 1)}", rel_gap(lo, l1), 1e-11 if t == 0 else 3e-6), (t, l1, lo)
    reps = [group.replica(i) for i in range(n_rep)]
    e0, r0 = reps[0].get_rows("ent"), reps[0].get_rows("rel")
    for rp in reps[1:]:
        assert np.array_equal(rp.get_rows("ent"), e0) and np.array_equal(rp.get_rows("rel"), r0)   # replicas: bit-identical
    es = single.get_rows("ent")
    assert np.mean(np.abs(e0 - es) <= 1e-5 + 1e-3 * np.abs(es)) > 0.99 and np.abs(e0 - es).max() < 2.5e-2
    assert np.mean(np.abs(e0 - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.99
    eo = one.replica(0).get_rows("ent")                                                             # a group of one == a session (up to the arrival order of fp32 atomics)
    assert np.mean(np.abs(eo - es) <= 1e-5 + 1e-3 * np.abs(es)) > 0.99
    T = X[:32]
    assert np.allclose(reps[-1].score(T), single.score(T), rtol=1e-4, atol=1e-5)
    for s in (single, group, one):
        s.close()


def test_session_group_of_one_through_rccl(gpu_lib):
    """AMDKGE_GROUP_FORCE_RCCL (VERDICT r3 #2b): a group of ONE replica that takes the multi-replica path -- librccl bound with
    dlopen, ncclCommInitAll over the one device, gradient-only kernels, grouped ncclAllReduce of both gradient tables on the
    replica's stream, dense sweeps, ncclCommDestroy.  On a one-GPU box this is every RCCL call of the group step, for real.
    Must equal a plain session (a one-rank all-reduce is the identity) and the oracle."""
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.session import Session, SessionGroup

    rng = np.random.default_rng(4)
    model, k, N, R, B, eta, seed = "ComplEx", 200, 300, 5, 512, 6, 9
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.08).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.08).astype(np.float32)
    X = np.stack([rng.integers(0, N, 3 * B), rng.integers(0, R, 3 * B), rng.integers(0, N, 3 * B)], 1).astype(np.int32)
    reg = regularizers.get("LP", {"p": 2, "lambda": 1e-3})
    mk = lambda: (loss_functions.get("self_adversarial"), optimizers.get("adam", {"learning_rate": 1e-2}))   # noqa: E731
    single = Session(model, k, N, R, eta, *mk(), reg, seed=seed)
    forced = SessionGroup([0], model, k, N, R, eta, *mk(), reg, seed=seed, force_rccl=True)
    plain = SessionGroup([0], model, k, N, R, eta, *mk(), reg, seed=seed)
    uses, version = forced.info()
    print("session group of one through RCCL: uses_rccl", uses, "ncclGetVersion", version)
    assert uses and version > 0 and plain.info() == (False, 0)
    for s in (single, forced):
        s.set_rows("ent", ent)
        s.set_rows("rel", rel)
    st = O.TrainState(ent, rel, "adam", 1e-2)
    for t in range(3):
        xb = X[t * B:(t + 1) * B]
        l1, lf = single.train_step(xb), forced.train_step(xb)
        ref = float(O.train_step(st, model, xb, eta, "self_adversarial", seed, t, max_rel_size=R, reg=dict(p=2, lam_e=1e-3, lam_r=1e-3)))
        assert abs(lf - ref) <= 3e-5 * abs(ref), (t, lf, ref)
        # (same reasoning as in test_session_group_matches_single_session: bit-equal tables at step 0 only)
        assert within(f"session/rccl_group_of_one/loss_step{min(t, 1)}", rel_gap(lf, l1), 1e-11 if t == 0 else 3e-6), (t, l1, lf)
    ef, es = forced.replica(0).get_rows("ent"), single.get_rows("ent")
    assert np.mean(np.abs(ef - es) <= 1e-5 + 1e-3 * np.abs(es)) > 0.99 and np.abs(ef - es).max() < 2.5e-2
    assert np.mean(np.abs(ef - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.99
    for s in (single, forced, plain):
        s.close()


@pytest.mark.parametrize("model,k", [("ComplEx", 100), ("DistMult", 200), ("TransE", 64)])
def test_session_rank_takes_the_screening_pass(gpu_lib, model, k):
    """amdkge_session_rank counts through amdkge_rank_counts_screened: the contraction models report that the int8
    screening pass ran (amdkge_session_screen_stats), TransE that its exact early exit did (kge_rank_tile.hip, kge_rank_early.h: on these untrained-looking
    tables the device-side probe hands the work to the plain kernel, nothing is re-checked), and the ranks are those of the
    declared-order oracle, bit for bit, either way."""
    from oracle import rank_ordered as RO

    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import Session

    rng = np.random.default_rng(11)
    N, R, n = 1500, 4, 256
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    T = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    F = np.concatenate([T, np.stack([rng.integers(0, N, 4000), rng.integers(0, R, 4000), rng.integers(0, N, 4000)], 1).astype(np.int32)])
    fs, fo = O.filter_sets(T, [F])
    s = Session(model, k, N, R, 2, loss_functions.get("nll"), optimizers.get("adam"), seed=0)
    s.set_rows("ent", ent)
    s.set_rows("rel", rel)
    for strat in ("worst", "middle"):
        got = s.rank(T, _csr(fs), _csr(fo), corrupt_side="s,o", ranking_strategy=strat)
        ref = RO.evaluate_ranks(model, ent, rel, T, fs, fo, corrupt_side="s,o", ranking_strategy=strat)
        assert np.array_equal(got, ref), (model, strat, np.argwhere(got != ref)[:5])
        stats = s.screen_stats()
        if model == "TransE":
            assert stats == (0, False)
        else:
            assert stats is not None and not stats[1] and 0 <= stats[0] < n * N // 20, stats   # ran; a few per cent rechecked at most
    s.close()


def _rows_reference(model, ent, rel, batches, eta, seed, W, negatives, opt, lr, reg):
    """The oracle on ONE process with the whole table following a row-sharded group's schedule: replica r takes the share
    [B r / W, B (r + 1) / W) of every batch; corruptions from the global Philox rows over all N ids ("global") or over the
    replica's own row range ("local": the same Philox rows, range n_local, + lo); gradients summed; one dense step."""
    N, R = ent.shape[0], rel.shape[0]
    st = O.TrainState(ent, rel, opt, lr)
    rows_per = -(-N // W)
    losses = []
    for step, xb in enumerate(batches):
        bg = xb.shape[0]
        Ge, Gr, tot = np.zeros(ent.shape, np.float64), np.zeros(rel.shape, np.float64), 0.0
        for r in range(W):
            lo, hi = bg * r // W, bg * (r + 1) // W
            xr = xb[lo:hi]
            if len(xr) == 0:
                continue
            if negatives == "global":
                ng = O.generate_corruptions(xr, N, eta, seed, step, lo, bg)
            else:
                slo, n_local = r * rows_per, min(N, (r + 1) * rows_per) - r * rows_per
                B = xr.shape[0]
                j = np.repeat(np.arange(eta, dtype=np.uint64), B)
                i = np.tile(np.arange(B, dtype=np.uint64), eta)
                keep, repl = O.sample_corruption_draws(j * np.uint64(bg) + np.uint64(lo) + i, step, seed, n_local)
                data = np.tile(xr, (eta, 1))
                repl = repl.astype(np.int64) + slo
                ng = np.stack([np.where(keep == 1, data[:, 0], repl), data[:, 1], np.where(keep == 1, repl, data[:, 2])], 1).astype(np.int32)
            loss, ge, gr, _ = O.dense_gradients(model, st.ent, st.rel, xr, ng, eta, "self_adversarial", None, "sum", R)
            Ge += ge
            Gr += gr
            tot += float(loss)
        for x, G in ((st.ent, Ge), (st.rel, Gr)):
            xx = x.astype(np.float64)
            tot += reg[1] * float((np.abs(xx) ** reg[0]).sum())
            G += reg[1] * reg[0] * np.abs(xx) ** (reg[0] - 1) * np.sign(xx)
        O.apply_optimizer(st, Ge, Gr)
        losses.append(tot)
    return st, losses


@pytest.mark.parametrize("model,k,opt,W,negatives", [("ComplEx", 8, "adam", 2, "global"), ("ComplEx", 200, "adam", 3, "global"),
                                                     ("DistMult", 64, "adagrad", 2, "local"), ("TransE", 12, "sgd", 4, "local"),
                                                     ("RotatE", 100, "adam", 2, "global"), ("ComplEx", 200, "adam", 1, "local")])
def test_session_group_rows_matches_single_session(gpu_lib, model, k, opt, W, negatives):
    """amdkge_session_group_create_rows: the entity table row-sharded over W replicas through the C ABI, numpy only.
    Here all replicas on device 0 -- device copies ordered by events instead of grouped ncclSend / ncclRecv, everything else
    of the multi-GPU path: device-side routing, request / row / gradient exchanges, gradient-only kernels on the local index
    space, relation all-reduce, per-shard sweeps.  global negatives: == a single session on the whole batch (same corruptions
    by construction) == the oracle; local negatives: == the oracle following the sharded schedule.  N is not a multiple of W
    (ragged last shard), B not a multiple of W (ragged shares), ids repeat (de-duplicated requests), s == o triples."""
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.session import Session, SessionGroup

    rng = np.random.default_rng(13)
    N, R, B, eta, seed, lr = 131, 4, 203, 3, 7, 1e-2
    K = O.internal_k(model, k)
    sc = 0.3 if k < 100 else 0.08
    ent = (rng.normal(size=(N, K)) * sc).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * sc).astype(np.float32)
    X = np.stack([rng.integers(0, N, 3 * B), rng.integers(0, R, 3 * B), rng.integers(0, N, 3 * B)], 1).astype(np.int32)
    X[:9, 2] = X[:9, 0]
    batches = [X[t * B:(t + 1) * B] for t in range(3)]
    reg = regularizers.get("LP", {"p": 2, "lambda": 1e-3})
    mk = lambda: (loss_functions.get("self_adversarial"), optimizers.get(opt, {"learning_rate": lr}))   # noqa: E731
    group = SessionGroup([0] * W, model, k, N, R, eta, *mk(), reg, seed=seed, rows=True, max_batch=B, global_negatives=negatives == "global")
    group.set_rows("ent", ent)
    group.set_rows("rel", rel)
    assert np.array_equal(group.get_rows("ent"), ent) and np.array_equal(group.get_rows("ent", ids=[130, 0, 77, 77, 66]), ent[[130, 0, 77, 77, 66]])
    st, ref_losses = _rows_reference(model, ent, rel, batches, eta, seed, W, negatives, opt, lr, (2, 1e-3))
    single = None
    if negatives == "global":
        single = Session(model, k, N, R, eta, *mk(), reg, seed=seed)
        single.set_rows("ent", ent)
        single.set_rows("rel", rel)
    for t, xb in enumerate(batches):
        lg = group.train_step(xb)
        assert abs(lg - ref_losses[t]) <= 3e-5 * abs(ref_losses[t]), (t, lg, ref_losses[t])
        if single is not None:
            l1 = single.train_step(xb)
            assert abs(lg - l1) <= 3e-5 * abs(l1), (t, lg, l1)
    assert not group.route_overflow()
    eg, rg = group.get_rows("ent"), group.get_rows("rel")
    assert np.mean(np.abs(eg - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.99 and np.abs(eg - st.ent).max() < 2.5e-2
    assert np.mean(np.abs(rg - st.rel) <= 1e-5 + 1e-3 * np.abs(st.rel)) > 0.99
    if single is not None:
        es = single.get_rows("ent")
        assert np.mean(np.abs(eg - es) <= 1e-5 + 1e-3 * np.abs(es)) > 0.99 and np.abs(eg - es).max() < 2.5e-2
        single.close()
    if opt == "adam":   # the optimizer state lives with the rows: m of the entity table, gathered from the owners
        mg = group.get_rows("ent_slot0")
        assert np.mean(np.abs(mg - st.slots["m_e"]) <= 1e-6 + 2e-3 * np.abs(st.slots["m_e"])) > 0.99
    group.close()


def test_session_group_rows_argument_checks(gpu_lib):
    from ampligraph_amd import _ffi
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import SessionGroup

    mk = lambda: (loss_functions.get("nll"), optimizers.get("adam"))   # noqa: E731
    with pytest.raises(_ffi.AmdKgeError):   # the last replica would own no rows
        SessionGroup([0] * 4, "DistMult", 8, 5, 2, 2, *mk(), rows=True, max_batch=16)
    with pytest.raises(ValueError):
        SessionGroup([0] * 2, "DistMult", 8, 50, 2, 2, *mk(), rows=True)
    g = SessionGroup([0] * 2, "DistMult", 8, 50, 2, 2, *mk(), rows=True, max_batch=16)
    X = np.stack([np.arange(32) % 50, np.zeros(32, int), (np.arange(32) * 7) % 50], 1).astype(np.int32)
    with pytest.raises(_ffi.AmdKgeError):   # more than max_batch
        g.train_step(X)
    bad = X[:8].copy()
    bad[3, 2] = 50
    with pytest.raises(_ffi.AmdKgeError):   # id outside the GLOBAL table
        g.train_step(bad)
    g.train_step(X[:16])
    g.close()


def cs_head(csr, n):
    off, ids = csr
    return off[:n + 1], ids[:off[n]]


@pytest.mark.parametrize("model,k,W,max_batch,force_rccl,threads", [
    ("ComplEx", 100, 2, 4000, False, False), ("DistMult", 200, 4, 4000, False, False), ("HolE", 64, 3, 120, False, False),
    ("TransE", 64, 2, 4000, False, False), ("RotatE", 40, 3, 4000, False, False), ("ComplEx", 100, 1, 4000, True, False), ("TransE", 50, 4, 90, False, False),
    # round 6: one host thread per replica (AMDKGE_GROUP_FORCE_THREADS: the path replicas on distinct devices take), per-replica staging
    ("ComplEx", 100, 2, 4000, False, True), ("DistMult", 200, 4, 4000, False, True), ("TransE", 64, 3, 120, False, True), ("RotatE", 40, 2, 4000, False, True),
    ("HolE", 64, 4, 90, False, True)])
def test_session_group_rank_row_sharded_is_bit_identical(gpu_lib, model, k, W, max_batch, force_rccl, threads):
    """amdkge_session_group_rank: evaluation through a ROW-SHARDED group, numpy only.  Every replica counts all
    queries against its own rows (filter ids restricted to the shard), the query rows are gathered from their owners into the scratch
    rows, counts and filter subtractions are summed over the replicas, +1 once -- the reference's partition loop
    (ScoringBasedEmbeddingModel.py:1431-1452,1684; AbstractScoringLayer.py:280-288).  W = 1-4 replicas on device 0 (W = 1 forced
    through RCCL: the int32 ncclAllReduce of rows and counts, for real), ragged last shard, one chunk (the screened / early-exit
    count pass) and many small chunks (max_batch 90 / 120), three strategies x four sides, filtered and not, entities_subset:
    ranks bit-identical to amdkge_session_rank on ONE session holding the whole table and to the declared-order oracle."""
    from oracle import rank_ordered as RO

    from ampligraph_amd import _ffi
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import Session, SessionGroup

    rng = np.random.default_rng(21)
    N, R, n = 2601, 5, 300
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    T = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    T[:7, 2] = T[:7, 0]                                            # s == o queries
    T[7:20, 0] = N - 1                                             # the last row of the ragged last shard, repeated
    F = np.concatenate([T, np.stack([rng.integers(0, N, 6000), rng.integers(0, R, 6000), rng.integers(0, N, 6000)], 1).astype(np.int32)])
    fs, fo = O.filter_sets(T, [F])
    mk = lambda: (loss_functions.get("nll"), optimizers.get("adam"))   # noqa: E731
    single = Session(model, k, N, R, 2, *mk(), seed=0)
    group = SessionGroup([0] * W, model, k, N, R, 2, *mk(), seed=0, rows=True, max_batch=max_batch, force_rccl=force_rccl, force_threads=threads)
    if force_rccl:
        assert group.info()[0]
    for s in (single, group):
        s.set_rows("ent", ent)
        s.set_rows("rel", rel)
    cs, co = _csr(fs), _csr(fo)
    for strat in ("worst", "best", "middle"):
        for side in ("s,o", "s", "o", "s+o"):
            want = single.rank(T, cs, co, corrupt_side=side, ranking_strategy=strat)
            got = group.rank(T, cs, co, corrupt_side=side, ranking_strategy=strat)
            assert got.shape == want.shape and np.array_equal(got, want), (strat, side, np.argwhere(got != want)[:5])
            if strat == "worst" and side == "s,o" and model != "RotatE":
                assert np.array_equal(got, RO.evaluate_ranks(model, ent, rel, T, fs, fo, corrupt_side="s,o", ranking_strategy="worst"))
    assert np.array_equal(group.rank(T, corrupt_side="s,o"), single.rank(T, corrupt_side="s,o"))                       # unfiltered
    assert np.array_equal(group.rank(T, None, co, corrupt_side="o", ranking_strategy="middle"), single.rank(T, None, co, corrupt_side="o", ranking_strategy="middle"))
    sub = np.concatenate([rng.integers(0, N, 700), [N - 1, 0, 0, 5]]).astype(np.int32)   # duplicates, both ends of the table
    for side in ("s,o", "s+o"):
        assert np.array_equal(group.rank(T, cs, co, entities_subset=sub, corrupt_side=side), single.rank(T, cs, co, entities_subset=sub, corrupt_side=side)), side
    few = np.array([3, 4, 5], dtype=np.int32)                      # a subset no candidate of which lives on the later shards
    assert np.array_equal(group.rank(T[:40], cs_head(cs, 40), None, entities_subset=few, corrupt_side="s"),
                          single.rank(T[:40], cs_head(cs, 40), None, entities_subset=few, corrupt_side="s"))
    assert group.rank(T[:0]).shape == (0, 2)
    bad = T[:5].copy()
    bad[2, 0] = N
    with pytest.raises(_ffi.AmdKgeError):
        group.rank(bad)
    # training on the group after an evaluation used the scratch rows, and evaluation of the trained shards
    X = np.stack([rng.integers(0, N, 64), rng.integers(0, R, 64), rng.integers(0, N, 64)], 1).astype(np.int32)
    assert np.isfinite(group.train_step(X))
    single.set_rows("ent", group.get_rows("ent"))
    single.set_rows("rel", group.get_rows("rel"))
    assert np.array_equal(group.rank(T[:100], cs_head(cs, 100), cs_head(co, 100)), single.rank(T[:100], cs_head(cs, 100), cs_head(co, 100)))
    single.close()
    group.close()


@pytest.mark.parametrize("threads", [False, True])
def test_session_group_rank_replicated(gpu_lib, threads):
    """A replicated group splits the queries over its replicas (slices of the filter offsets index the whole id arrays); with
    `threads` every replica is driven from a host thread of its own, as replicas on distinct devices are."""
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import Session, SessionGroup

    rng = np.random.default_rng(5)
    model, k, N, R, n = "ComplEx", 32, 700, 3, 211
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    T = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    fs, fo = O.filter_sets(T, [np.concatenate([T, np.stack([rng.integers(0, N, 3000), rng.integers(0, R, 3000), rng.integers(0, N, 3000)], 1).astype(np.int32)])])
    mk = lambda: (loss_functions.get("nll"), optimizers.get("adam"))   # noqa: E731
    single = Session(model, k, N, R, 2, *mk(), seed=0)
    group = SessionGroup([0, 0, 0], model, k, N, R, 2, *mk(), seed=0, force_threads=threads)
    for s in (single, group):
        s.set_rows("ent", ent)
        s.set_rows("rel", rel)
    for side in ("s,o", "s+o", "o"):
        assert np.array_equal(group.rank(T, _csr(fs), _csr(fo), corrupt_side=side, ranking_strategy="middle"),
                              single.rank(T, _csr(fs), _csr(fo), corrupt_side=side, ranking_strategy="middle")), side
    single.close()
    group.close()


@pytest.mark.parametrize("k,nl", [(8, "tanh"), (200, "linear")])
def test_session_paths_with_focuse_weights_against_oracle(gpu_lib, k, nl):
    """FocusE weights through every session path that sets up the loss of a step: a Session (the complete step), a replicated group
    (gradient-only shares of 203 over 3: the weights of a share start at focus_w + lo) and a row-sharded group (203 over 2, global
    negatives: the corruptions of one GPU), ComplEx k = 8 and the owner-computes shape k = 200.  Every loss and the final tables are
    held to the oracle's step with focus=(w, beta, nl), beta the structural weight of the session's own config."""
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.session import Session, SessionGroup

    rng = np.random.default_rng(17)
    model, N, R, B, eta, seed, lr = "ComplEx", 131, 4, 203, 3, 7, 1e-2
    K = O.internal_k(model, k)
    sc = 0.3 if k < 100 else 0.08
    ent = (rng.normal(size=(N, K)) * sc).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * sc).astype(np.float32)
    X = np.stack([rng.integers(0, N, 3 * B), rng.integers(0, R, 3 * B), rng.integers(0, N, 3 * B)], 1).astype(np.int32)
    Wt = (0.05 + 0.9 * rng.random(3 * B)).astype(np.float32)
    reg = regularizers.get("LP", {"p": 2, "lambda": 1e-3})
    mk = lambda: (loss_functions.get("self_adversarial"), optimizers.get("adam", {"learning_rate": lr}))   # noqa: E731
    beta = float(mk()[0].to_ffi().focus_beta)   # what Session / SessionGroup put into cfg.loss
    runs = {"session": Session(model, k, N, R, eta, *mk(), reg, seed=seed, focus_nonlinearity=nl),
            "replicated": SessionGroup([0, 0, 0], model, k, N, R, eta, *mk(), reg, seed=seed, focus_nonlinearity=nl),
            "rows": SessionGroup([0, 0], model, k, N, R, eta, *mk(), reg, seed=seed, focus_nonlinearity=nl, rows=True, max_batch=B,
                                 global_negatives=True)}
    for s in runs.values():
        s.set_rows("ent", ent)
        s.set_rows("rel", rel)
    st = O.TrainState(ent, rel, "adam", lr)
    for t in range(3):
        xb, wb = X[t * B:(t + 1) * B], Wt[t * B:(t + 1) * B]
        ref = float(O.train_step(st, model, xb, eta, "self_adversarial", seed, t, max_rel_size=R, reg=dict(p=2, lam_e=1e-3, lam_r=1e-3),
                                 focus=(wb, beta, nl)))
        for name, s in runs.items():
            got = s.train_step(xb, focus_w=wb)
            print(f"focuse {name} k={k} step {t}: loss {got!r} oracle {ref!r} rel {abs(got - ref) / abs(ref):.3e}")
            assert abs(got - ref) <= 3e-5 * abs(ref), (name, t, got, ref)
    for name, s in runs.items():
        e, r = (s.replica(0) if name == "replicated" else s).get_rows("ent"), (s.replica(0) if name == "replicated" else s).get_rows("rel")
        print(f"focuse {name} k={k}: ent within {np.mean(np.abs(e - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)):.4f} max {np.abs(e - st.ent).max():.3e}"
              f" rel within {np.mean(np.abs(r - st.rel) <= 1e-5 + 1e-3 * np.abs(st.rel)):.4f}")
        assert np.mean(np.abs(e - st.ent) <= 1e-5 + 1e-3 * np.abs(st.ent)) > 0.99 and np.abs(e - st.ent).max() < 2.5e-2, name
        assert np.mean(np.abs(r - st.rel) <= 1e-5 + 1e-3 * np.abs(st.rel)) > 0.99, name
        s.close()


@pytest.mark.parametrize("mode", ["replicated", "rows", "cols"])
def test_session_group_refuses_a_bad_triple_and_carries_on(gpu_lib, mode):
    """A triple whose entity id equals N, through every group entry: the step (and, for the row-sharded group, the rank call) raises
    before any kernel is launched and the message names the triple's index -- the index within the replica's share where a replicated
    group hands shares to its replicas.  Nothing of the refused step stays behind: the valid steps that follow match a fresh group fed
    only those (two runs of the same code: equal losses up to the arrival order of the loss partials at the first step, of the fp32
    row-adds after it)."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.latent_features import loss_functions, optimizers, regularizers
    from ampligraph_amd.session import SessionGroup

    rng = np.random.default_rng(23)
    model, k, N, R, B, eta, seed = "ComplEx", 16, 131, 4, 203, 3, 7
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N, K)) * 0.3).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.3).astype(np.float32)
    X = np.stack([rng.integers(0, N, 2 * B), rng.integers(0, R, 2 * B), rng.integers(0, N, 2 * B)], 1).astype(np.int32)
    reg = regularizers.get("LP", {"p": 2, "lambda": 1e-3})
    kw = {"replicated": {}, "rows": dict(rows=True, max_batch=B, global_negatives=True), "cols": dict(cols=True)}[mode]
    W = 3 if mode == "replicated" else 2
    mk = lambda: SessionGroup([0] * W, model, k, N, R, eta, loss_functions.get("self_adversarial"),   # noqa: E731
                              optimizers.get("adam", {"learning_rate": 1e-2}), reg, seed=seed, **kw)
    used, fresh = mk(), mk()
    for g in (used, fresh):
        g.set_rows("ent", ent)
        g.set_rows("rel", rel)
    i = B - 5                                        # in the LAST share: the replicas before it have been given theirs
    lo = B * (W - 1) // W
    bad = X[:B].copy()
    bad[i, 2] = N
    with pytest.raises(_ffi.AmdKgeError) as err:
        used.train_step(bad)
    assert f"triple {i - lo if mode == 'replicated' else i} has" in str(err.value), str(err.value)
    if mode == "replicated":                         # in the first share the two numberings agree
        bad0 = X[:B].copy()
        bad0[3, 0] = N
        with pytest.raises(_ffi.AmdKgeError) as err:
            used.train_step(bad0)
        assert "triple 3 has" in str(err.value), str(err.value)
    if mode == "rows":
        with pytest.raises(_ffi.AmdKgeError) as err:
            used.rank(bad[i - 2:i + 3])
        assert "session_group_rank: triple 2 has" in str(err.value), str(err.value)
        assert np.array_equal(used.rank(X[:20]), fresh.rank(X[:20]))
    for t in range(2):
        xb = X[t * B:(t + 1) * B]
        lu, lf = used.train_step(xb), fresh.train_step(xb)
        print(f"after a refused step, {mode} step {t}: {lu!r} vs fresh {lf!r} rel {rel_gap(lu, lf):.3e}")
        assert within(f"session/after_refused_step/{mode}/loss_step{t}", rel_gap(lu, lf), 1e-11 if t == 0 else 3e-6), (t, lu, lf)
    eu, ef = (g.replica(0).get_rows("ent") if mode == "replicated" else g.get_rows("ent") for g in (used, fresh))
    assert np.mean(np.abs(eu - ef) <= 1e-5 + 1e-3 * np.abs(ef)) > 0.99 and np.abs(eu - ef).max() < 2.5e-2
    used.close()
    fresh.close()
