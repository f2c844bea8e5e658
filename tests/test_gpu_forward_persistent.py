"""The persistent forward kernel of the owner-computes step (train_fwdbwd_kernel<STAGE, one wave per positive>): a wave walks the
positives g, g + n_waves, ..., keeps its copy of s, p, o in LDS and sums its loss in its own LDS slot.  The grid cannot be capped
from outside, so the shapes make waves take several positives at any occupancy (B well above 256 CUs x 8 waves x 4 SIMDs = 8 192
positives at k = 8; above 3 072 at the headline width) or fewer positives than one block has waves.  Deterministic mode is held
bit for bit to oracle/train_ordered, the default mode to the bars tests/test_gpu_kernels.py uses for the same quantities."""
import numpy as np
import pytest
import torch

from margins import rel_gap, within
from oracle import kge_oracle as O
from test_gpu_kernels import assert_grads_close, dense, dev, loss_desc, make_engine, make_optimizer, rand_triples, run_tiled_grads

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ deterministic mode, bit for bit
def _det_steps(model, k, N, R, B, eta, loss, steps=1, X=None, seed=6, rng_seed=0, scale=0.2):
    """`steps` deterministic steps (StepLoop, Adam) and the same steps by oracle/train_ordered on the STORED rows.
    -> (engine's stored ent, rel; oracle's; mean-loss sum of the engine; the oracle's loss sum)."""
    from oracle import train_ordered as TO

    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    rng = np.random.default_rng(rng_seed)
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    ent = rng.uniform(-scale, scale, size=(N, eng.K)).astype(np.float32)
    rel = rng.uniform(-scale, scale, size=(R, eng.K)).astype(np.float32)
    eng.set_tables(ent, rel)
    if X is None:
        X = rand_triples(rng, steps * B, N, R)
    assert X.shape[0] == steps * B
    loop = StepLoop(eng, eta, loss_functions.get(loss), optimizers.get("adam", {"learning_rate": 1e-2}), None, seed=seed, dist=None)
    loop.deterministic = True
    st = TO.OptState(eng.ent.cpu().numpy().copy(), eng.rel.cpu().numpy().copy(), "adam", 1e-2)   # stored rows (padded halves)
    Xd = torch.as_tensor(X).cuda()
    loop.reset_loss()
    ref = 0.0
    for step in range(steps):
        loop.step(Xd[step * B:(step + 1) * B], step)
        xb = X[step * B:(step + 1) * B]
        ref += (TO.rotate_step_det(st, xb, eta, seed, step, loss, max_rel_size=R) if model == "RotatE"
                else TO.transe_step_det(st, xb, eta, seed, step, loss=loss) if model == "TransE"
                else TO.trilinear_step_det(model, st, xb, eta, seed, step, loss))
    torch.cuda.synchronize()
    assert eng.tiled_status() == 0
    return eng.ent.cpu().numpy(), eng.rel.cpu().numpy(), st, loop.mean_batch_loss() * steps, ref


def _assert_bitwise(out, loss):
    e, r, st, got, ref = out
    assert np.array_equal(e, st.ent) and np.array_equal(r, st.rel), (int((e != st.ent).sum()), int((r != st.rel).sum()),
                                                                     float(np.abs(e - st.ent).max()))
    # (the fp64 loss partials arrive in any order; multiclass_nll's log is the hardware's in the loss VALUE only)
    assert within(f"persistent/det_vs_ordered_oracle/{loss}", rel_gap(got, ref), 5e-6 if loss == "multiclass_nll" else 1e-12), (got, ref)


@pytest.mark.parametrize("model,k,N,B,eta", [("DistMult", 8, 500, 20011, 3),      # 2.4 positives per wave at 8 waves per SIMD, unequal walks
                                               ("ComplEx", 200, 3000, 7001, 20)],   # the headline width: 2.3 per wave at 3 waves per SIMD
                         ids=["DistMult-8-B20011", "ComplEx-200-B7001"])
def test_unequal_walks_deterministic(gpu_lib, model, k, N, B, eta):
    _assert_bitwise(_det_steps(model, k, N, 7, B, eta, "self_adversarial"), "self_adversarial")


def test_unequal_walks_default_mode(gpu_lib):
    """B = 20 011 in the default mode: one whole step against the oracle at the bars of test_tiled_step_in_place_parity."""
    model, k, N, R, B, eta = "DistMult", 8, 20000, 7, 20011, 3
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
    w, mk = make_optimizer("adam", {})
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    X = rand_triples(np.random.default_rng(1), B, N, R)
    eng.loss_acc.zero_()
    eng.train_step_tiled(dev(X), eta, loss_desc("self_adversarial"), w.to_ffi(1, 2), 77, 1)
    ref_loss = float(O.train_step(st, model, X, eta, "self_adversarial", 77, 1, max_rel_size=R))
    torch.cuda.synchronize()
    got_loss = float(eng.loss_acc[0].item()) + float(eng.loss_acc[1].item())
    print("unequal walks, default mode: loss", got_loss, "oracle", ref_loss)
    assert abs(got_loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (got_loss, ref_loss)
    e, r = eng.get_tables()
    ce = np.abs(e - st.ent) <= 1e-5 + 1e-4 * np.abs(st.ent)
    cr = np.abs(r - st.rel) <= 1e-5 + 1e-4 * np.abs(st.rel)
    assert ce.mean() > 0.995 and cr.mean() > 0.99, (ce.mean(), cr.mean())
    assert np.abs(e - st.ent).max() < 2.5e-2


@pytest.mark.parametrize("B", [1, 3, 5, 4 * 7 + 1])
def test_fewer_positives_than_slots(gpu_lib, B):
    """Waves without a positive leave; the tables and the loss of two steps, the second step's loss counted once."""
    out = _det_steps("ComplEx", 12, 60, 3, B, 5, "self_adversarial", steps=2, scale=0.4)
    _assert_bitwise(out, "self_adversarial")
    # default mode: loss_parts is folded exactly once per step -- the same batch twice from the same tables gives the same loss twice
    eng, ent, rel = make_engine("ComplEx", 12, 60, 3, scale=0.4)
    X = rand_triples(np.random.default_rng(B), B, 60, 3)
    L1 = run_tiled_grads(eng, X, 5, "nll", "sum", 3, 1)[0]
    L2 = run_tiled_grads(eng, X, 5, "nll", "sum", 3, 1)[0]
    negs = O.generate_corruptions(X, 60, 5, 3, 1)
    total = O.dense_gradients("ComplEx", ent, rel, X, negs, 5, "nll", None, "sum", 3)[0]
    assert abs(L1 - float(total)) <= 1e-5 * max(1.0, abs(L1)) and abs(L2 - float(total)) <= 1e-5 * max(1.0, abs(L2)), (L1, L2, float(total))


@pytest.mark.parametrize("model,k", [("TransE", 16), ("ComplEx", 12), ("DistMult", 16)])   # (TransE: one positive per wave, the same property)
def test_scores_do_not_depend_on_which_wave_takes_a_positive(gpu_lib, model, k):
    """Caller-given corruptions: the scores of one call at B = 9 001 are bit-equal to those of three calls on consecutive slices
    (a positive lands on another wave, as another trip of its walk)."""
    from ampligraph_amd import _ffi

    N, R, B, eta = 400, 5, 9001, 5
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3)
    rng = np.random.default_rng(2)
    X = rand_triples(rng, B, N, R)
    negs = O.generate_corruptions(X, N, eta, 11, 0).reshape(eta, B, 3)

    def scores(lo, hi):
        n = hi - lo
        eng.prepare_training("adam")
        eng.loss_acc.zero_()
        ps = torch.empty(n, dtype=torch.float32, device="cuda")
        ns = torch.empty(n * eta, dtype=torch.float32, device="cuda")
        d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, 0.0, 1)
        eng.train_step_tiled(dev(X[lo:hi]), eta, loss_desc("nll"), d, 0, 0, grad_only=True,
                             neg_override=dev(np.ascontiguousarray(negs[:, lo:hi]).reshape(-1, 3)), pos_scores=ps, neg_scores=ns)
        torch.cuda.synchronize()
        return ps.cpu().numpy(), ns.cpu().numpy().reshape(eta, n)

    ps, ns = scores(0, B)
    cuts = [0, 2999, 6002, B]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        p1, n1 = scores(lo, hi)
        assert np.array_equal(p1, ps[lo:hi]) and np.array_equal(n1, ns[:, lo:hi]), (lo, hi)


def _same_subject(rng, B, N, R):
    X = rand_triples(rng, B, N, R)
    X[:, 0] = 5
    return X


def _loops(rng, B, N, R):
    X = rand_triples(rng, B, N, R)
    X[:, 0] = 0
    X[:, 2] = 0
    return X


@pytest.mark.parametrize("model,k,B,batch", [("ComplEx", 12, 60, _loops), ("ComplEx", 12, 60, _same_subject), ("DistMult", 20, 60, _loops),
                                             ("ComplEx", 200, 60, _loops), ("DistMult", 200, 60, _same_subject),   # 50 quads: idle lanes
                                             ("RotatE", 32, 3500, None), ("RotatE", 12, 60, _same_subject)],
                         ids=["ComplEx-0p0", "ComplEx-same-s", "DistMult-0p0", "ComplEx-200-0p0", "DistMult-200-same-s", "RotatE-rel_cs",
                              "RotatE-same-s"])
def test_lds_copy_of_spo(gpu_lib, model, k, B, batch):
    """The gradient transform reads the wave's LDS copy of s, the prepared p and o: positives (0, p, 0), positives that share s,
    RotatE with the per-step phase table (RotatE keeps one positive per wave and reloads its rows: the same batches hold it to the
    same bits).  Two steps, deterministic, bitwise.
    The one-row batches are short: the deterministic tile pass sorts a row's entries in LDS, and thousands of entries on one row
    make it fall back to arrival order (tiled_status 1), which no oracle restates -- the long ones follow in the default mode."""
    N, R, eta = 400, 4, 6
    X = None if batch is None else batch(np.random.default_rng(9), 2 * B, N, R)
    _assert_bitwise(_det_steps(model, k, N, R, B, eta, "nll", steps=2, X=X, scale=0.3 if k < 100 else 0.08), "nll")


@pytest.mark.parametrize("k", [12, 200])   # 200: the headline width, 50 of the 64 lanes hold a quad
@pytest.mark.parametrize("batch", [_loops, _same_subject], ids=["0p0", "same-s"])
def test_lds_copy_of_spo_every_trip_of_a_walk(gpu_lib, batch, k):
    """B = 7 000 at three waves per SIMD: every wave takes two or three positives, all of them (0, p, 0) or with one s, so the
    copy a trip reads is the one the trip before it wrote over.  Default mode, gradients against the oracle at the bars of
    test_tiled_overflow_buckets_and_duplicates (thousands of fp32 terms on one row, unordered)."""
    model, N, R, B, eta = "ComplEx", 400, 4, 7000, 3
    eng, ent, rel = make_engine(model, k, N, R, scale=0.4 if k < 100 else 0.08)
    X = batch(np.random.default_rng(9), B, N, R)
    L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, "nll", "sum", 5, 2)
    negs = O.generate_corruptions(X, N, eta, 5, 2)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, "nll", None, "sum", R)
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max()) and np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
    assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L))
    assert_grads_close(Ge, Te, tol=1e-4)
    assert_grads_close(Gr, Tr, tol=1e-4)


GEOMETRY = [("DistMult", 300, 5), ("ComplEx", 150, 5),    # two quads per lane; padded halves
            ("DistMult", 4, 5),                           # one quad
            ("DistMult", 200, 5),                         # idle lanes
            ("ComplEx", 12, 1), ("ComplEx", 12, 7), ("ComplEx", 12, 64), ("ComplEx", 12, 65)]   # a side with no row; row groups


@pytest.mark.parametrize("model,k,eta", GEOMETRY, ids=[f"{m}-{k}-eta{e}" for m, k, e in GEOMETRY])
def test_geometries_two_steps_bitwise(gpu_lib, model, k, eta):
    _assert_bitwise(_det_steps(model, k, 400, 4, 1500, eta, "self_adversarial", steps=2, scale=0.2 if k < 100 else 0.08), "self_adversarial")


# ------------------------------------------------------------------------------------------------ the step's modes, default bars
def _in_place_two_steps(model, loss, pos_atomic=False, lazy=False, hot=None, reg=None):
    N, R, k, B, eta = 300, 4, 12, 2049, 4
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
    if hot:
        eng.set_hot_rows(hot)
    w, mk = make_optimizer("adam", {})
    w.lazy = lazy
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    rng = np.random.default_rng(6)
    oreg = None if reg is None else dict(p=reg[0], lam_e=reg[1], lam_r=reg[1])
    lam = reg[1] if reg else 0.0
    for t in range(1, 3):
        X = rand_triples(rng, B, N, R)
        if hot:
            X[: B // 2, 0] = hot[0]
            X[::5, 2] = hot[0]
        eng.loss_acc.zero_()
        eng.train_step_tiled(dev(X), eta, loss_desc(loss), w.to_ffi(t, reg[0] if reg else 2), 77, t, reg_e=lam, reg_r=lam, pos_atomic=pos_atomic)
        ref_loss = float(O.train_step(st, model, X, eta, loss, 77, t, max_rel_size=R, reg=oreg, lazy=lazy))
        torch.cuda.synchronize()
        got_loss = float(eng.loss_acc[0].item()) + float(eng.loss_acc[1].item())
        assert abs(got_loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (t, got_loss, ref_loss)
        e, r = eng.get_tables()
        ce = np.abs(e - st.ent) <= 1e-5 + 1e-4 * np.abs(st.ent)
        # (hot rows sum ~1 000 fp32 terms in arrival order: the bar of test_tiled_hot_rows_parity)
        assert ce.mean() > (0.97 if hot else 0.995), (t, ce.mean())
        assert np.abs(e - st.ent).max() < 2.5e-2


@pytest.mark.parametrize("mode", ["touched_rows", "pos_atomic", "hot_rows", "regulariser"])
def test_modes_in_place(gpu_lib, mode):
    _in_place_two_steps("ComplEx", "self_adversarial", pos_atomic=mode == "pos_atomic", lazy=mode == "touched_rows",
                        hot=[7, 11] if mode == "hot_rows" else None, reg=(3, 1e-2) if mode == "regulariser" else None)


@pytest.mark.parametrize("loss", list(O.LOSS_DEFAULTS))
def test_each_loss_gradient_only_two_steps(gpu_lib, loss):
    """apply_update = 0, each of the losses, two consecutive steps on one workspace: scores, loss and gradients against the oracle."""
    model, N, R, k, B, eta = "ComplEx", 300, 4, 12, 2049, 4
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
    rng = np.random.default_rng(3)
    for step in (4, 5):
        X = rand_triples(rng, B, N, R)
        L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, loss, "sum", seed=9, step=step)
        eng.g_rel.zero_()
        negs = O.generate_corruptions(X, N, eta, 9, step)
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, "sum", R)
        assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L)), (step, L)
        assert_grads_close(Ge, Te)
        assert_grads_close(Gr, Tr)


def test_focuse_weights_two_steps(gpu_lib):
    from ampligraph_amd import _ffi

    model, N, R, k, B, eta, beta, nl = "ComplEx", 300, 4, 12, 2049, 4, 0.37, "tanh"
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
    rng = np.random.default_rng(12)
    for step in (7, 8):
        X = rand_triples(rng, B, N, R)
        wmean = rng.random(B).astype(np.float32)
        wd = dev(wmean)
        ld = loss_desc("self_adversarial")
        ld.focus_nonlinearity = _ffi.FOCUS_NONLINEARITY[nl]
        ld.focus_beta = beta
        ld.d_focus_w = wd.data_ptr()
        eng.prepare_training("adam")
        eng.loss_acc.zero_()
        d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, 0.0, 1)
        eng.train_step_tiled(dev(X), eta, ld, d, 3, step, grad_only=True)
        torch.cuda.synchronize()
        negs = O.generate_corruptions(X, N, eta, 3, step)
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, "self_adversarial", None, "sum", R,
                                                         focus=(wmean, beta, nl))
        L = float(eng.loss_acc[0].item())
        assert abs(L - float(per.astype(np.float64).sum())) <= 2e-5 * max(1.0, abs(L)), (step, L)
        assert_grads_close(dense(eng, eng.g_ent), Te, tol=4e-5)
        assert_grads_close(dense(eng, eng.g_rel), Tr, tol=4e-5)
