"""Non-finite scores on the shared-negative train paths (kge_train_shared.hip, its masked form, kge_train_shared_dist.hip): the NaN
rules of tests/test_gpu_nonfinite.py -- a NaN score is a NaN loss VALUE, a coefficient that a clip, a hinge or the MASK zeroes is
still multiplied by the score's Jacobian, 0 * NaN = NaN reaches exactly the rows the reference would poison -- held against the
step's definition: O.dense_gradients on SR.override_rows (masked: MR.masked_step(finite=False)).  The cases and what the oracle says
about them are tests/shared_nonfinite_cases.py and tests/test_shared_nonfinite_host.py; every bar is an existing one of this suite."""
import numpy as np
import pytest
import torch

import shared_nonfinite_cases as NC
import shared_ref as SR
from margins import within
from oracle import kge_oracle as O
from test_gpu_kernels import dense, dev, loss_desc, make_engine, make_optimizer, rand_triples, run_fwdbwd
from test_gpu_nonfinite import compare_grads, same_or_nan
from test_gpu_shared import grad_gap, run_shared
from test_gpu_shared_dist import run_dist
from test_gpu_shared_mask import run_masked

pytestmark = pytest.mark.gpu


def engine_for(case, pad=True):
    eng, _, _ = make_engine(case.model, case.k, case.N, case.R, scale=NC.SCALE, pad=pad)
    assert eng.K == case.ent.shape[1]
    eng.set_tables(case.ent.copy(), case.rel.copy())                       # (the cases are read-only)
    return eng


def run_entry(entry, eng, case, loss, reduction="sum"):
    """-> ((loss sum, dense entity gradient, dense relation gradient, positive scores, corruption scores [M * B]), stats or None)"""
    method, _, _, masked = NC.ENTRIES[entry]
    args = (eng, np.array(case.X), case.G, np.array(case.ids), np.array(case.side), loss, reduction)
    if method == "train_shared_fwdbwd":
        return run_shared(*args), None
    ks, ko = (case.ks, case.ko) if masked else (None, None)
    if method == "train_shared_masked_fwdbwd":
        return run_masked(*args, ks, ko, identity=case.identity)
    return run_dist(*args, ks, ko, identity=case.identity)


def close_where_finite(got, want, tol=1e-5):
    fin = np.isfinite(want)
    return not fin.any() or same_or_nan(got[fin], want[fin], tol, tol * np.abs(want[fin]).max())


# ------------------------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("loss", NC.LOSSES)
@pytest.mark.parametrize("entry,model,plant", NC.all_cases())
def test_shared_nonfinite_loss_and_gradients(gpu_lib, entry, model, plant, loss):
    """The assertions of test_gpu_nonfinite.py::test_nonfinite_rows_loss_and_gradients on every shared entry point; a lone list
    entry must also leave every row that belongs to the other groups alone."""
    masked = NC.ENTRIES[entry][3]
    case = NC.build(entry, model, plant)
    eng = engine_for(case)
    (L, Ge, Gr, ps, ns), stats = run_entry(entry, eng, case, loss)
    ref_loss, Te, Tr, sp, sn = NC.oracle(case, loss, masked)
    bad_e, bad_r = NC.bad_rows(Te), NC.bad_rows(Tr)
    print(f"{entry} {model} {plant} {loss}: loss {L:.9g} / {ref_loss:.9g}, non-finite scores {int((~np.isfinite(ns)).sum())} / {int((~np.isfinite(sn)).sum())}, "
          f"non-finite rows ent {int(NC.bad_rows(Ge).sum())} / {int(bad_e.sum())} rel {int(NC.bad_rows(Gr).sum())} / {int(bad_r.sum())}")
    # scores: non-finite exactly where the oracle's are (-inf at the mask), equal elsewhere
    assert np.array_equal(np.isfinite(ps), np.isfinite(sp)) and np.array_equal(np.isfinite(ns), np.isfinite(sn))
    assert close_where_finite(ps, sp) and close_where_finite(ns, sn)
    if masked:
        mask, n_masked, unmaskable = case.mask_matrix()
        assert np.isneginf(ns[mask.T.reshape(-1)]).all() and stats == [n_masked, unmaskable]
    if case.layout == "given" and case.kind not in NC.OWN:
        # asserted on the kernel's output alone: nothing of group 1's lone list entry reaches a row of the groups 0, 2, 3, 4
        clean_e, clean_r = case.clean_rows()
        assert np.isfinite(Ge[clean_e]).all() and np.isfinite(Gr[clean_r]).all(), (np.asarray(clean_e)[~np.isfinite(Ge[clean_e]).all(1)][:10].tolist(),)
    if NC.is_inf_plant(plant):
        # (test_nonfinite_rows_loss_and_gradients: which non-finite value an inf becomes depends on the algebraic form) the oracle's
        # loss or a non-finite one, and no finite gradient row where the oracle has none
        assert (not np.isfinite(L)) or abs(L - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (L, ref_loss)
        for G, bad_t in ((Ge, bad_e), (Gr, bad_r)):
            bad_g = NC.bad_rows(G)
            assert not (bad_t & ~bad_g).any(), (int(bad_t.sum()), int(bad_g.sum()), np.nonzero(bad_t & ~bad_g)[0][:10].tolist())
        if model == "TransE" and np.isfinite(ref_loss) and not bad_e.any() and not bad_r.any():
            # sign(+-inf) is finite: the oracle's step is a finite one (and -inf here is what a mask writes), so it is compared in full
            assert np.isfinite(L) and abs(L - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (L, ref_loss)
            assert compare_grads(Ge, Te, "entity") + compare_grads(Gr, Tr, "relation") == 0
        return
    assert np.array_equal(np.isnan(ps), np.isnan(sp)) and np.array_equal(np.isnan(ns), np.isnan(sn))
    assert np.isnan(L) == np.isnan(ref_loss), (L, ref_loss)
    if np.isfinite(ref_loss):
        assert abs(L - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (L, ref_loss)
    assert compare_grads(Ge, Te, "entity") + compare_grads(Gr, Tr, "relation") >= 1


# ------------------------------------------------------------------------------------------------------------------ 2. two formulations
@pytest.mark.parametrize("plant", ["own_nan_unit@replaced", "own_nan_unit@kept", "list_nan_row"])
@pytest.mark.parametrize("loss", ["nll", "self_adversarial"])           # a masked zero; a computed coefficient
@pytest.mark.parametrize("entry,model", [(e, m) for e in ("shared", "dist") for m in NC.ENTRIES[e][1]])
def test_shared_nonfinite_equals_the_fused_kernel(gpu_lib, entry, model, loss, plant):
    """amdkge_train_fwdbwd(d_neg_override = the equivalent rows) on the same spoiled tables: the same non-finite rows, and on the
    finite ones the bars of test_shared_equals_the_fused_kernel_on_the_override_rows."""
    case = NC.build(entry, model, plant)
    eng = engine_for(case)
    (L1, Ge1, Gr1, ps1, ns1), _ = run_entry(entry, eng, case, loss, "mean")
    L2, Ge2, Gr2, ps2, ns2 = run_fwdbwd(eng, np.array(case.X), case.M, loss, "mean", seed=0, step=0, negs=case.negs)
    assert np.array_equal(np.isnan(ps1), np.isnan(ps2)) and np.array_equal(np.isnan(ns1), np.isnan(ns2)) and (np.isnan(ps2).any() or np.isnan(ns2).any())
    assert close_where_finite(ps1, ps2) and close_where_finite(ns1, ns2)
    assert np.isnan(L1) == np.isnan(L2), (L1, L2)
    if np.isfinite(L2):
        assert within("shared_nonfinite_vs_fused_loss", abs(L1 - L2) / max(1.0, abs(L2)), 1e-5)
    for what, G1, G2 in (("ent", Ge1, Ge2), ("rel", Gr1, Gr2)):
        b1, b2 = NC.bad_rows(G1), NC.bad_rows(G2)
        assert np.array_equal(b1, b2), (what, int(b1.sum()), int(b2.sum()), np.nonzero(b1 != b2)[0][:10].tolist())
        if what == "ent":
            assert 1 <= b2.sum() < case.N / 2
        if (~b2).any():
            assert within(f"shared_nonfinite_vs_fused_grad_{what}", grad_gap(G1[~b2], G2[~b2]), 2e-5)


# ------------------------------------------------------------------------------------------------------------------ 3. the tile edges
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("M", [33, 65])
@pytest.mark.parametrize("G", [37, 5])
@pytest.mark.parametrize("model,k", list(NC.GEOMETRY_SEEDS))
def test_shared_nonfinite_geometry(gpu_lib, model, k, G, M, pad):
    """A NaN row at list position M - 1 -- the lone column of the second tile (M = 65), the tail of 1 of the backward chunks of 32 --
    and a NaN in the last live unit of the LAST positive's replaced row (G = 5: a last group of 2): the oracle's row sets, and with
    pad the padding floats of both gradient tables exact zeros, not NaN, in every row."""
    case = NC.geometry_case(model, k, G, M)
    entry = "shared" if model in NC.GEMM_MODELS else "dist"
    eng = engine_for(case, pad=pad)
    for loss in ("nll", "self_adversarial"):
        (L, Ge, Gr, ps, ns), _ = run_entry(entry, eng, case, loss)
        ref_loss, Te, Tr, sp, sn = NC.oracle(case, loss, False)
        assert np.array_equal(np.isnan(ps), np.isnan(sp)) and np.array_equal(np.isnan(ns), np.isnan(sn)) and np.isnan(L) and np.isnan(ref_loss)
        assert close_where_finite(ps, sp) and close_where_finite(ns, sn)
        n_bad = compare_grads(Ge, Te, f"entity {loss}") + compare_grads(Gr, Tr, f"relation {loss}")
        assert n_bad >= 2
        if pad:
            for g, n in ((eng.g_ent, case.N), (eng.g_rel, case.R)):
                stored = g.cpu().numpy().reshape(n, -1, eng.ks)
                assert eng.ks > eng.k and not stored[:, :, eng.k:].any(), (loss, np.nonzero(stored[:, :, eng.k:].any((1, 2)))[0][:10].tolist())


# ------------------------------------------------------------------------------------------------------------------ 4. whole steps
@pytest.mark.parametrize("loss", ["nll", "self_adversarial"])
@pytest.mark.parametrize("model", ["ComplEx", "TransE", "RotatE"])
def test_shared_nonfinite_whole_steps(gpu_lib, model, loss):
    """Two complete steps (draw on the device -> forward / backward -> dense Adam) from a table with one NaN row, the entry
    ids[1][2] of the first step's draw: the loss of each step and the set of table rows that hold a non-finite value afterwards
    equal the oracle's on the override rows (test_gpu_nonfinite.py::test_nonfinite_rows_after_whole_steps)."""
    N, R, k, B, G, M, seed = 300, 5, 32, 37, 8, 5, 77
    ent0, rel0 = NC.tables(model, k, N, R, 3)
    rng = np.random.default_rng(5)
    Xs = [rand_triples(rng, B, N, R) for _ in range(2)]
    ids1, _ = SR.sample_shared(Xs[0], G, M, seed, 1, sample_range=N)
    ent = ent0.copy()
    ent[int(ids1[1, 2]), :] = np.nan
    eng, _, _ = make_engine(model, k, N, R, scale=NC.SCALE)
    eng.set_tables(ent, rel0)
    w, mk = make_optimizer("adam", {})
    eng.prepare_training(w.name)
    st = mk(ent, rel0)
    step = eng.train_shared_fwdbwd if model in NC.GEMM_MODELS else eng.train_shared_dist_fwdbwd
    spread = []
    for t, X in enumerate(Xs, start=1):
        Xd = dev(X)
        eng.loss_acc.zero_()
        ids, side = eng.sample_shared(Xd, G, M, seed, t)
        step(Xd, G, M, ids, side, loss_desc(loss))
        eng.opt_step(w.to_ffi(t, 2), 0.0, 0.0)
        torch.cuda.synchronize()
        want_ids, want_side = SR.sample_shared(X, G, M, seed, t, sample_range=N)
        assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(side.cpu().numpy(), want_side)
        with np.errstate(all="ignore"):
            ref_loss = float(O.train_step(st, model, X, M, loss, seed, t, max_rel_size=R, negs=SR.override_rows(X, G, want_ids, want_side)))
        got_loss = float(eng.loss_acc[0].item())
        assert np.isnan(got_loss) == np.isnan(ref_loss), (t, got_loss, ref_loss)
        e, r = eng.get_tables()
        bad_e, bad_o = ~np.isfinite(e).all(1), ~np.isfinite(st.ent).all(1)
        assert np.array_equal(bad_e, bad_o), (t, int(bad_e.sum()), int(bad_o.sum()), np.nonzero(bad_e != bad_o)[0][:10].tolist())
        assert np.array_equal(~np.isfinite(r).all(1), ~np.isfinite(st.rel).all(1)), t
        ok = ~bad_o
        spread.append(int(bad_o.sum()))
        if ok.any():
            frac = float(np.mean(np.abs(e[ok] - st.ent[ok]) <= 1e-5 + 1e-4 * np.abs(st.ent[ok])))
            print(f"{model} {loss} step {t}: {spread[-1]} non-finite rows, finite rows inside the bar {frac:.4f}")
            assert frac > (0.95 if model == "TransE" else 0.99)             # (the bulk criterion of that test, unchanged)
    assert 1 < spread[0] < N


# ------------------------------------------------------------------------------------------------------------------ 5. the workspace
@pytest.mark.parametrize("entry,model", [("shared", "ComplEx"), ("dist", "RotatE")])
def test_step_does_not_depend_on_what_the_workspace_held(gpu_lib, entry, model):
    """A list_nan_row step leaves NaN in Q, dQ, the coefficients and the score buffer of the engine's workspace; a finite step of a
    SMALLER shape (another layout of the same buffer) on that engine == the same step on a fresh engine: scores bit for bit, loss
    and gradients (fp32 atomics in arrival order on both sides) within the bars of the two-formulations tests."""
    case = NC.build(entry, model, "list_nan_row")
    used = engine_for(case)
    (L0, _, _, _, _), _ = run_entry(entry, used, case, "self_adversarial")
    assert np.isnan(L0)
    B, G, M = 23, 8, 12
    ent, rel = NC.tables(model, case.k, case.N, case.R, 11)
    X = rand_triples(np.random.default_rng(12), B, case.N, case.R)
    ids, side = SR.sample_shared(X, G, M, 13, 4, sample_range=case.N)
    small = NC.Case(model=model, X=X, G=G, ids=ids, side=side, ks=None, ko=None, identity=False)
    used.set_tables(ent, rel)
    fresh, _, _ = make_engine(model, case.k, case.N, case.R, scale=NC.SCALE)
    fresh.set_tables(ent, rel)
    (L1, Ge1, Gr1, ps1, ns1), _ = run_entry(entry, used, small, "self_adversarial")
    (L2, Ge2, Gr2, ps2, ns2), _ = run_entry(entry, fresh, small, "self_adversarial")
    assert np.isfinite(L2) and np.isfinite(Ge2).all() and np.isfinite(Gr2).all() and Ge2.any()
    assert np.array_equal(ps1.view(np.uint32), ps2.view(np.uint32)) and np.array_equal(ns1.view(np.uint32), ns2.view(np.uint32))
    assert np.isfinite(Ge1).all() and np.isfinite(Gr1).all()
    assert within("shared_nonfinite_workspace_grad_ent", grad_gap(Ge1, Ge2), 2e-5)
    assert within("shared_nonfinite_workspace_grad_rel", grad_gap(Gr1, Gr2), 2e-5)
    assert within("shared_nonfinite_workspace_loss", abs(L1 - L2) / max(1.0, abs(L2)), 1e-5)


# ------------------------------------------------------------------------------------------------------------------ 6. through fit()
@pytest.mark.parametrize("mask_known", [False, True])
@pytest.mark.parametrize("model", ["ComplEx", "TransE", "RotatE"])
def test_nonfinite_loss_is_reported_by_fit_with_shared_negatives(gpu_lib, model, mask_known):
    """One NaN in the initial entity table is a NaN loss in History from the first epoch on
    (test_gpu_nonfinite.py::test_nonfinite_loss_is_reported_by_fit), with the negatives of a group shared."""
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import BoundSharedNegatives, SharedDistanceNegatives, SharedNegatives

    X = toy_graph(5, n=400, N=40, R=3)
    rng = np.random.default_rng(0)
    K = O.internal_k(model, 10)
    E0 = (rng.normal(size=(40, K)) * 0.3).astype(np.float32)
    R0 = (rng.normal(size=(3, K)) * 0.3).astype(np.float32)
    E0[7, 1] = np.nan
    cls = SharedNegatives if model == "ComplEx" else SharedDistanceNegatives
    m = ScoringBasedEmbeddingModel(eta=5, k=10, scoring_type=model, seed=1)
    # (RotatE insists on Glorot-initialised relations: only its entity table is given)
    m.compile(optimizer="adam", loss="nll", entity_relation_initializer=[E0, "glorot_uniform" if model == "RotatE" else R0],
              negatives=cls(num_negs=24, group_size=16, mask_known=mask_known))
    h = m.fit(X, batch_size=128, epochs=2, verbose=False).history["loss"]
    assert isinstance(m._loop.negatives, BoundSharedNegatives) and hasattr(m._loop.negatives, "mask") == mask_known
    assert len(h) == 2 and np.isnan(h).all(), (model, mask_known, h)
