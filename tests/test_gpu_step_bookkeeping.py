"""The bookkeeping of the owner-computes step's tile pass (kge_train_tile.hip, kge_train_direct.hip, kge_train_tiled.hip): the
bucket fills, the overflow count and the tile ticket must be zero again after every launch (one round of tiles or several, with
and without overflow), the forward kernel's loss partials must be folded exactly once per step whoever folds them (a sweep
workgroup, or the tiles when the launch has none), the relation sweep that rides beside the tiles must give the bits of
amdkge_opt_step, and the two cases that keep more of the old epilogue -- the entity
regulariser's fold by the last tile to finish, the touched-rows marks -- must still work over consecutive steps."""
import numpy as np
import pytest
import torch

from margins import within
from oracle import kge_oracle as O
from test_gpu_kernels import dense, dev, loss_desc, make_engine, make_optimizer, rand_triples

pytestmark = pytest.mark.gpu

HOT_ROW = 5


def one_row_override(X, eta, rows=(HOT_ROW,)):
    """Negatives override [eta * B, 3] (row j * B + i = corruption j of positive i): the object of every corruption is replaced
    by ONE row, so every corruption entry of the batch lands in the bucket of the tile that owns it -- far beyond a bucket's
    capacity (twice the mean + slack): the shared overflow list is used.  rows = (a, b): corruption j goes to rows[j % 2], two
    tiles with half of the entries each (the two-round shape: the deterministic mode's sort buffer holds 2 048 entries of a tile
    there, and all 2 048 corruptions + the tile's own entries on one tile would be added unsorted, flagged by the library)."""
    negs = np.tile(X, (eta, 1)).astype(np.int32)
    negs[:, 2] = np.repeat(np.array([rows[j % len(rows)] for j in range(eta)], dtype=np.int32), X.shape[0])
    return negs


def step_and_check(eng, st, w, model, X, eta, t, R, tag, negs=None, reg=None, lazy=False, zero_loss=True, **mode):
    """One whole step on the engine and in the oracle, compared at the bars of test_gpu_kernels.py::test_tiled_step_in_place_parity
    (and test_gpu_lazy.py for the touched-rows mode).  Returns (engine loss incl. regulariser, oracle loss) of the step."""
    oreg = None if reg is None else dict(p=reg[0], lam_e=reg[1], lam_r=reg[1])
    lam = reg[1] if reg else 0.0
    if zero_loss:
        eng.loss_acc.zero_()
    eng.train_step_tiled(dev(X), eta, loss_desc("self_adversarial"), w.to_ffi(t, reg[0] if reg else 2), 77, t, reg_e=lam, reg_r=lam,
                         neg_override=None if negs is None else dev(negs), **mode)
    ref_loss = float(O.train_step(st, model, X, eta, "self_adversarial", 77, t, max_rel_size=R, reg=oreg, negs=negs, lazy=lazy))
    torch.cuda.synchronize()
    assert float(eng.g_rel.abs().max()) == 0.0 and float(eng.g_ent.abs().max()) == 0.0
    got_loss = float(eng.loss_acc[0].item()) + float(eng.loss_acc[1].item())
    if zero_loss:
        assert abs(got_loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (tag, t, got_loss, ref_loss)
    e, r = eng.get_tables()
    fe = float(np.mean(np.abs(e - st.ent) > 1e-5 + 1e-4 * np.abs(st.ent)))
    fr = float(np.mean(np.abs(r - st.rel) > 1e-5 + 1e-4 * np.abs(st.rel)))
    print(f"{tag} step {t}: loss {got_loss!r} oracle {ref_loss!r}; outside: ent {fe:.2e} rel {fr:.2e}; max |d ent| {np.abs(e - st.ent).max():.3e}")
    assert within(f"bookkeeping/{tag}/ent_frac_outside", fe, 0.005) and within(f"bookkeeping/{tag}/rel_frac_outside", fr, 0.01), (tag, t, fe, fr)
    assert np.abs(e - st.ent).max() < 2.5e-2, (tag, t)
    for nme in st.slots:
        ok = np.isclose(dense(eng, eng.slots[nme]), st.slots[nme], rtol=1e-3, atol=1e-6 + 2e-5 * np.abs(st.slots[nme]).max())
        print(f"{tag} step {t}: slot {nme} outside {1.0 - ok.mean():.2e}")
        # (short rows: test_tiled_step_in_place_parity's 0.9999, and test_lazy_tiled_step_parity's 0.998 for the relation slots of
        # the touched-rows mode; rows beyond 2 KB: test_direct_step_in_place_parity's 0.001)
        bar = 0.002 if (lazy and nme.endswith("_r")) else (1e-4 if st.ent.shape[1] < 200 else 0.001)
        assert within(f"bookkeeping/{tag}/slot_{nme}", 1.0 - ok.mean(), bar), (tag, nme, t, ok.mean())
    return got_loss, ref_loss


def override_schedule(rng, B, N, R, eta, override, rows=(HOT_ROW,)):
    """Three batches: the one-row override on steps 1 and 3 (when asked for), ordinary sampling on step 2."""
    out = []
    for t in range(1, 4):
        X = rand_triples(rng, B, N, R)
        out.append((t, X, one_row_override(X, eta, rows) if override and t != 2 else None))
    return out


def default_mode_steps(model, k, N, R, B, eta, override, tag, scale=0.5, rows=(HOT_ROW,), **mode):
    eng, ent, rel = make_engine(model, k, N, R, scale=scale)
    w, mk = make_optimizer("adam", {})
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    for t, X, negs in override_schedule(np.random.default_rng(6), B, N, R, eta, override, rows):
        step_and_check(eng, st, w, model, X, eta, t, R, tag, negs=negs, **mode)
    return eng


def deterministic_steps_equal_fresh_workspace(model, k, N, R, B, eta, override, tag, scale=0.5, rows=(HOT_ROW,)):
    """Deterministic mode: the tables and slots after every step on ONE workspace carried through the steps are, bit for bit,
    those of the same steps each run on a freshly zeroed workspace.  A count or a ticket left behind by a step shows here: the
    next step on the carried workspace would walk stale overflow entries, or never zero its own.  No step may be flagged
    (amdkge_train_tiled_status: a tile with more entries than its sort buffer holds is added in arrival order)."""
    engs = []
    for _ in range(2):
        eng, ent, rel = make_engine(model, k, N, R, scale=scale)
        w, _mk = make_optimizer("adam", {})
        eng.prepare_training(w.name)
        engs.append(eng)
    carried, fresh = engs
    for t, X, negs in override_schedule(np.random.default_rng(6), B, N, R, eta, override, rows):
        fresh._twork = None   # (the engine allocates a zero-filled workspace when it has none)
        for eng in engs:
            eng.train_step_tiled(dev(X), eta, loss_desc("self_adversarial"), w.to_ffi(t, 2), 77, t,
                                 neg_override=None if negs is None else dev(negs), deterministic=True)
            assert eng.tiled_status() == 0, (tag, t)
        torch.cuda.synchronize()
        for nme, a, b in [("ent", carried.ent, fresh.ent), ("rel", carried.rel, fresh.rel)] + [(n, carried.slots[n], fresh.slots[n]) for n in carried.slots]:
            assert torch.equal(a, b), (tag, t, nme, int((a != b).sum()))


# ---------------------------------------------------------------- 1. overflow across consecutive steps
T1 = dict(model="ComplEx", k=16, N=600, R=4, B=256, eta=4)


def test_overflow_across_steps_deterministic(gpu_lib):
    deterministic_steps_equal_fresh_workspace(**T1, override=True, tag="t1/det")


def test_overflow_across_steps_default_mode(gpu_lib):
    default_mode_steps(**T1, override=True, tag="t1/default")


# ---------------------------------------------------------------- 2. more tiles than CUs (two rounds)
T2 = dict(model="ComplEx", k=512, N=12000, R=4, B=512, eta=4)   # 4 KB rows, ~36 per tile: two rounds of tiles on 256 CUs
T2_ROWS = (HOT_ROW, 6000)   # rows of two different tiles (ownership blocks 0 and 750 of 8 rows, dealt round 500 tiles)


@pytest.mark.parametrize("override", [False, True])
def test_two_rounds_of_tiles_deterministic(gpu_lib, override):
    deterministic_steps_equal_fresh_workspace(**T2, override=override, tag=f"t2/det/ovr{int(override)}", scale=0.08, rows=T2_ROWS)


@pytest.mark.parametrize("override", [False, True])
def test_two_rounds_of_tiles_default_mode(gpu_lib, override):
    default_mode_steps(**T2, override=override, tag=f"t2/default/ovr{int(override)}", scale=0.08, rows=T2_ROWS)


@pytest.mark.parametrize("override", [False, True])
def test_row_direct_pass_across_steps(gpu_lib, override):
    """The row-direct pass (kge_train_direct.hip) carries a copy of the epilogue: a shape of tests/test_gpu_tile_direct.py.
    Default mode only: the plan never sends a deterministic step to the row-direct pass (make_plan: `direct_long = ... && !det`;
    a deterministic step at this shape runs tile_backward_kernel, which tests 1 and 2 hold bit for bit)."""
    default_mode_steps("ComplEx", 600, 120, 4, 60, 3, override, f"t2/direct/ovr{int(override)}", scale=0.08)


# ---------------------------------------------------------------- 3. relation sweep
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("opt", ["adam", "adagrad", "sgd"])   # two slots, one slot, none
@pytest.mark.parametrize("N,R", [(600, 3000),     # 200 tiles, a large table: 64 sweep workgroups, 4 - 5 strides per thread
                                 (14505, 237)])   # the headline tables: 255 tiles leave ONE CU for the 24 sweep workgroups
def test_relation_sweep_bits_of_opt_step(gpu_lib, opt, lam, N, R):
    """The sweep workgroups beside the tiles == amdkge_opt_step on the same gradient, bit for bit (x and every slot), whether
    the sweep workgroups run beside the tiles or queue on the one CU the tiles leave free.  Deterministic mode, so that two runs form the
    same relation gradient: one engine takes the whole step, the other the gradient-only step and then the library's plain sweep."""
    model, k, B, eta = "ComplEx", 200, 64, 4
    engs = []
    for _ in range(2):
        eng, ent, rel = make_engine(model, k, N, R, scale=0.08)
        w, _mk = make_optimizer(opt, {})
        eng.prepare_training(w.name)
        engs.append(eng)
    whole, split = engs
    X = dev(rand_triples(np.random.default_rng(3), B, N, R))
    rel_before = rel.astype(np.float64)
    rel_dev_before = whole.rel.clone()
    whole.train_step_tiled(X, eta, loss_desc("self_adversarial"), w.to_ffi(1, 3), 77, 1, reg_e=0.0, reg_r=lam, deterministic=True)
    split.train_step_tiled(X, eta, loss_desc("self_adversarial"), w.to_ffi(1, 3), 77, 1, grad_only=True, deterministic=True)
    assert float(split.g_rel.abs().max()) > 0.0
    split.loss_acc.zero_()
    split.opt_step(w.to_ffi(1, 3), 0.0, lam)
    torch.cuda.synchronize()
    assert whole.tiled_status() == 0
    assert float(whole.g_rel.abs().max()) == 0.0
    assert torch.equal(whole.rel, split.rel), int((whole.rel != split.rel).sum())
    assert not torch.equal(whole.rel, rel_dev_before)
    for nme in whole.slots:
        if nme.endswith("_r"):
            assert torch.equal(whole.slots[nme], split.slots[nme]), nme
    got = float(whole.loss_acc[1].item())
    if lam:
        host = lam * float((np.abs(rel_before) ** 3).sum())
        print(f"relation regulariser: step {got!r} host {host!r} plain sweep {float(split.loss_acc[1].item())!r}")
        assert abs(got - host) <= 1e-5 * host   # (the bar of test_opt_step_parity: fp32 partial sums per thread, fp64 between them)
    else:
        assert got == 0.0


# ---------------------------------------------------------------- 4. loss fold
@pytest.mark.parametrize("model,N,k", [("ComplEx", 150, 12),    # a sweep workgroup folds
                                       ("ComplEx", 40, 200),    # ... fewer tiles than partial slots
                                       ("TransE", 150, 12),     # no sweep workgroup (its sweep is a launch of its own): the tiles fold
                                       ("TransE", 40, 12)])     # ... fewer tiles than partial slots: several slots per tile
def test_loss_partials_folded_once_per_step(gpu_lib, model, N, k):
    R, B, eta = 4, 200, 4
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5 if k < 100 else 0.08)
    w, mk = make_optimizer("adam", {})
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    rng = np.random.default_rng(6)
    eng.loss_acc.zero_()
    ref = 0.0
    for t in range(1, 4):
        X = rand_triples(rng, B, N, R)
        _, ref_t = step_and_check(eng, st, w, model, X, eta, t, R, f"t4/{model}{N}", zero_loss=False)
        ref += ref_t
        got = float(eng.loss_acc[0].item())
        print(f"t4/{model}{N} after step {t}: accumulated {got!r} oracle {ref!r}")
        assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (t, got, ref)
    before = eng.loss_acc.clone()
    eng.train_step_tiled(dev(np.zeros((0, 3), np.int32)), eta, loss_desc("self_adversarial"), w.to_ffi(4, 2), 77, 4)
    torch.cuda.synchronize()
    assert torch.equal(eng.loss_acc, before)   # a step without positives folds nothing
    # ... and left every slot zero: one more step adds exactly its own loss
    X = rand_triples(rng, B, N, R)
    O.apply_optimizer(st, np.zeros_like(st.ent, dtype=np.float64), np.zeros_like(st.rel, dtype=np.float64))   # (the empty step: slots decay)
    _, ref_t = step_and_check(eng, st, w, model, X, eta, 5, R, f"t4/{model}{N}", zero_loss=False)
    got = float(eng.loss_acc[0].item())
    assert abs(got - (ref + ref_t)) <= 2e-5 * max(1.0, abs(ref + ref_t)), (got, ref + ref_t)


# ---------------------------------------------------------------- 5. entity regulariser: the fold by the last tile to finish
def test_entity_regulariser_two_steps(gpu_lib):
    eng, ent, rel = make_engine(T1["model"], T1["k"], T1["N"], T1["R"], scale=0.5)
    w, mk = make_optimizer("adam", {})
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    rng = np.random.default_rng(6)
    for t in (1, 2):
        X = rand_triples(rng, T1["B"], T1["N"], T1["R"])
        # (step 1 with the overflowing bucket: the overflow count is zeroed by this mode's end-of-tile ticket)
        step_and_check(eng, st, w, T1["model"], X, T1["eta"], t, T1["R"], "t5/reg", negs=one_row_override(X, T1["eta"]) if t == 1 else None, reg=(3, 1e-2))
        assert float(eng.loss_acc[1].item()) > 0.0


# ---------------------------------------------------------------- 6. touched-rows mode with atomic positives
def test_touched_rows_marks_cleared(gpu_lib):
    model, k, N, R, B, eta = (T1[x] for x in ("model", "k", "N", "R", "B", "eta"))
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
    w, mk = make_optimizer("adam", {})
    w.lazy = True
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    rng = np.random.default_rng(6)
    for t in (1, 2):
        B_t = B if t == 1 else 16   # the second batch touches few rows: a mark left by the first would move one of the others
        X = rand_triples(rng, B_t, N, R)
        negs = O.generate_corruptions(X, N, eta, 77, t)
        touched = np.zeros(N, dtype=bool)
        touched[np.concatenate([X[:, 0], X[:, 2], negs[:, 0], negs[:, 2]])] = True
        before = eng.ent.clone()
        step_and_check(eng, st, w, model, X, eta, t, R, "t6/lazy", lazy=True, pos_atomic=True)
        un = torch.as_tensor(~touched).cuda()
        assert t == 1 or int(un.sum()) > N // 2
        assert torch.equal(eng.ent[un], before[un]), (t, int((eng.ent[un] != before[un]).any(dim=1).sum()))
