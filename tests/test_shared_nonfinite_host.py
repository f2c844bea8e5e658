"""The non-finite cases of the shared-negative train paths without a GPU (tests/shared_nonfinite_cases.py): what the fp64 oracle says
about every case that tests/test_gpu_nonfinite_shared.py runs.  These are CONDITIONS on the cases, not measurements of a kernel: the
GPU file may rely on "the set of non-finite rows is small and not empty" or "group 0 stays clean" only because they are proven here
for the definition.  Also: MR.masked_step(finite=False) against O.dense_gradients with -inf written at the mask, and the numpy
restatement of the distance tiles (tests/shared_dist_ref.py) against the oracle's non-finite row sets."""
import numpy as np
import pytest

import shared_dist_ref as DR
import shared_mask_ref as MR
import shared_nonfinite_cases as NC
from oracle import kge_oracle as O

CASES = NC.all_cases()
GEOMETRIES = [(m, k, G, M) for (m, k), v in NC.GEOMETRY_SEEDS.items() for (G, M) in v]


def test_the_case_list():
    """every entry point, its own models, every plant that applies: 8 own-row plants everywhere, the 3 lone list entries where the
    groups have lists of their own, the masked plants where there is a mask"""
    assert len(CASES) == len(set(CASES)) == 3 * 11 + 3 * 12 + 3 * 9 + 2 * 11 + 2 * 13 + 2 * 9
    for entry, (method, models, layout, masked) in NC.ENTRIES.items():
        for model in models:
            plants = NC.plants_of(entry, model)
            assert set(NC.OWN_PLANTS) <= set(plants) and (layout == "identity" or set(NC.LIST) <= set(plants))
            assert ("masked_nan_row" in plants) == masked and ("masked_was_inf" in plants) == (masked and layout == "given" and model in NC.DIST_MODELS)


@pytest.mark.parametrize("entry,model,plant", CASES)
def test_case_conditions(entry, model, plant):
    """(a) a non-finite score, (b) a small, non-empty set of non-finite entity-gradient rows, (c) list plants stay inside group 1,
    (d) the conditioning preconditions over the finite pair-units -- for every loss, on the oracle alone"""
    case = NC.build(entry, model, plant)
    assert NC.case_is_sound(entry, case) is None
    layout, masked = NC.ENTRIES[entry][2:]
    L = NC.LAYOUTS[layout]
    assert (case.N, case.R, case.k, case.B, case.G, case.M) == tuple(L[x] for x in ("N", "R", "k", "B", "G", "M"))
    assert case.ids.shape == (5, case.M) and 0 < case.side.sum() < case.B
    kind, _, where = plant.partition("@")
    if kind in NC.OWN:                                                      # the planted row is positive 0's subject, replaced or kept
        assert case.side[0] == (1 if where == "replaced" else 0)
        row = case.rel[case.X[0, 1]] if kind == "rel_nan_unit" else case.ent[case.X[0, 0]]
        assert not np.isfinite(row).all()
        assert np.isfinite(case.ent).all(1).sum() >= case.N - 1 and np.isfinite(case.rel).all(1).sum() >= case.R - 1
    else:                                                                   # the lone entity: no positive, no other list entry
        assert not np.isfinite(case.ent[case.lone]).all() and np.isfinite(np.delete(case.ent, case.lone, 0)).all() and np.isfinite(case.rel).all()
        assert case.lone not in case.X[:, [0, 2]]
        if layout == "given":
            assert case.ids[1, 2] == case.lone and (case.ids == case.lone).sum() == 1
            clean_e, clean_r = case.clean_rows()
            assert len(clean_e) > 50                                        # the cross-group assertion of the GPU test has rows to look at
        else:
            assert (case.ids[:, 2] == case.lone).all() and (case.ids == case.lone).sum() == 5
    if masked:
        mask, n_masked, unmaskable = case.mask_matrix()
        assert n_masked > 0 and mask[np.arange(case.B) // case.G != 1].any()   # a mask away from group 1 too
        if kind.startswith("masked") and layout == "given":
            assert mask[8:16, 2].tolist() == [True, False] * 4


def test_what_the_oracle_says_about_the_list_plants():
    """the figures the cases were designed around: 8 non-finite corruption scores (group 1's column 2); NaN plants reach 8 - 9
    entity rows under the losses with a per-score mask and more under the two softmax-weighted ones; DistMult leaves the planted
    row's own gradient finite (-0 * finite), TransE and RotatE do not; an inf in a TransE row reaches nothing at all."""
    for model in NC.GEMM_MODELS + NC.DIST_MODELS:
        entry = "shared" if model in NC.GEMM_MODELS else "dist"
        for plant in NC.LIST:
            case = NC.build(entry, model, plant)
            for loss in NC.LOSSES:
                L, Te, Tr, sp, sn = NC.oracle(case, loss, False)
                bad_s = ~np.isfinite(sn).reshape(case.M, case.B)
                assert bad_s.sum() == 8 and bad_s[2, 8:16].all() and np.isfinite(sp).all()
                n = int(NC.bad_rows(Te).sum())
                if model == "TransE" and plant == "list_inf_unit":          # indistinguishable from a mask: compared NUMERICALLY on the GPU
                    assert np.isfinite(L) and n == 0 and not NC.bad_rows(Tr).any()
                    continue
                if "nan" in plant:
                    assert np.isnan(L)
                    assert (8 <= n <= 9) if loss in ("pairwise", "nll", "absolute_margin") else (10 <= n <= 25), (model, plant, loss, n)
                    # (multiclass_nll clips the NaN score itself: a zero coefficient for the planted entry, NaN for its neighbours)
                    assert NC.bad_rows(Te)[case.lone] == (model in NC.DIST_MODELS or loss == "self_adversarial")


def _dense_gradients_with_mask(case, loss, mask, reduction="sum"):
    """O.dense_gradients on the override rows, -inf written over the corruption scores at `mask` (its compute_scores wrapped)"""
    flat = np.asarray(mask).T.reshape(-1)
    plain = O.compute_scores

    def scores(model, s, p, o, **kw):
        sc = np.array(plain(model, s, p, o, **kw), dtype=np.float32)
        if sc.shape[0] == flat.shape[0]:
            sc[flat] = -np.inf
        return sc

    O.compute_scores = scores
    try:
        with np.errstate(all="ignore"):
            _, Te, Tr, (sp, sn, per) = O.dense_gradients(case.model, case.ent, case.rel, case.X, case.negs, case.M, loss, None, reduction, case.R)
    finally:
        O.compute_scores = plain
    return float(per.astype(np.float64).sum()), Te, Tr, sp, sn


@pytest.mark.parametrize("entry,model,plant", [c for c in CASES if NC.ENTRIES[c[0]][3] and (c[2].startswith("masked") or c[2] in ("own_nan_unit@kept", "list_nan_row"))])
def test_masked_step_is_dense_gradients_with_minus_inf_at_the_mask(entry, model, plant):
    case = NC.build(entry, model, plant)
    mask = case.mask_matrix()[0]
    assert mask.any() and mask.shape[0] * mask.shape[1] != case.B
    for loss in NC.LOSSES:
        for reduction in ("sum", "mean"):
            with np.errstate(all="ignore"):
                got = MR.masked_step(case.model, case.ent, case.rel, case.X, case.G, case.ids, case.side, mask, loss, reduction, case.R, finite=False)
            want = _dense_gradients_with_mask(case, loss, mask, reduction)
            assert np.isnan(got[0]) == np.isnan(want[0]) and (np.isnan(want[0]) or got[0] == want[0])
            for a, b in zip(got[1:], want[1:]):                             # gradients and scores: the same NaN, the same numbers
                assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)
            assert np.isneginf(got[4][mask.T.reshape(-1)]).all()


def test_masked_step_still_asserts_finiteness_by_default():
    case = NC.build("masked_given", "DistMult", "masked_nan_row")
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        MR.masked_step(case.model, case.ent, case.rel, case.X, case.G, case.ids, case.side, case.mask_matrix()[0], "nll", "sum", case.R)


@pytest.mark.parametrize("entry,model,plant", [c for c in CASES if c[1] in NC.DIST_MODELS and "nan" in c[2]])
def test_dist_restatement_is_nan_faithful(entry, model, plant):
    """DR.DistStep.step -- the header's arithmetic in numpy -- on the NaN plants: the oracle's non-finite score pattern and row sets"""
    case = NC.build(entry, model, plant)
    masked = NC.ENTRIES[entry][3]
    mask = case.mask_matrix()[0] if masked else None
    for loss in NC.LOSSES:
        with np.errstate(all="ignore"):
            L, Ge, Gr, sp, sn = DR.DistStep(model, case.ent, case.rel, case.X, case.G, case.ids, case.side, case.R).step(loss, "sum", mask=mask)
        want, Te, Tr, wp, wn = NC.oracle(case, loss, masked)
        assert np.array_equal(np.isnan(sp), np.isnan(wp)) and np.array_equal(np.isnan(sn), np.isnan(wn)) and np.array_equal(np.isneginf(sn), np.isneginf(wn))
        assert np.isnan(L) == np.isnan(want)
        assert np.array_equal(NC.bad_rows(Ge), NC.bad_rows(Te)), (loss, np.nonzero(NC.bad_rows(Ge) != NC.bad_rows(Te))[0][:10])
        assert np.array_equal(NC.bad_rows(Gr), NC.bad_rows(Tr)), loss
        ok = ~NC.bad_rows(Te)
        if ok.any():                                                        # (the identity list under a softmax: every row is NaN)
            assert np.allclose(Ge[ok], Te[ok], rtol=1e-4, atol=1e-5 * np.abs(Te[ok]).max())


@pytest.mark.parametrize("model,k,G,M", GEOMETRIES)
def test_geometry_case_conditions(model, k, G, M):
    case = NC.geometry_case(model, k, G, M)
    assert NC.geometry_is_sound(case) is None
    g = min(1, case.ids.shape[0] - 1)
    assert case.ids[g, M - 1] == case.lone and (case.ids == case.lone).sum() == 1 and case.lone not in case.X[:, [0, 2]]
    assert np.isnan(case.ent[case.lone]).all()
    own = case.X[-1, 0] if case.side[-1] else case.X[-1, 2]
    assert np.isnan(case.ent[own, k - 1]) and np.isnan(case.ent[own]).sum() == 1
    assert case.B % G in (0, 2)                                             # G = 5: the last group holds 2 positives


def test_the_seed_tables_are_the_first_sound_seeds():
    """the recorded seeds are what find_seed / find_geometry_seed give on this code (counting from 1)"""
    for (model, layout), seed in NC.SEEDS.items():
        assert NC.find_seed(model, layout, limit=seed + 1) == seed
    for (model, k), v in NC.GEOMETRY_SEEDS.items():
        for (G, M), seed in v.items():
            assert NC.find_geometry_seed(model, k, G, M, limit=seed + 1) == seed
