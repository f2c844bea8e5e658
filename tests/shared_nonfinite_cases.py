"""The non-finite cases of the shared-negative train paths, built once for the CPU conditions (tests/test_shared_nonfinite_host.py) and
the GPU comparisons (tests/test_gpu_nonfinite_shared.py): tables, positives, lists, sides, known ranges and ONE planted NaN / inf.
Test infrastructure: the product does not import it.

Layouts
  "given"    : N = 300, R = 5, k = 32, B = 37, G = 8, M = 5 (five groups, the last of 5 positives), the list drawn by
               SR.sample_shared, both sides in the batch.  The known ranges (used by the masked entry points only) are those of a
               graph the batch is cut from, plus one list entry each for two rows of groups 0 and 2.
  "identity" : N = M = 40, R = 2, k = 8, the all-entities list ids[g][j] = j of every group, ranges as above.
Plants (units 3 and 5 and relation unit 2 as in tests/test_gpu_nonfinite.py::plant)
  own_nan_row | own_nan_unit | own_inf_unit | rel_nan_unit @ replaced | kept : the SUBJECT row (the relation row) of positive 0 is
               spoiled; side[0] is set so that the subject is the replaced (1) or the kept (0) entity.
  list_nan_row | list_nan_unit | list_inf_unit : an entity that no positive and no other list entry uses -- LONE -- is written into
               ids[1, 2] only and its row spoiled: groups 0, 2, 3, 4 must stay clean.
  masked_nan_row : list_nan_row, and LONE is in the known range of rows 8, 10, 12, 14 -- half of group 1.  In the identity layout
               LONE = 2 = ids[g][2] of EVERY group, known to the even rows of the batch.
  masked_was_inf : list_inf_unit with the same four rows masked (TransE, RotatE): both routes to -inf in one score row."""
import functools

import numpy as np

import shared_mask_ref as MR
import shared_ref as SR
from oracle import kge_oracle as O

GEMM_MODELS, DIST_MODELS = ("DistMult", "ComplEx", "HolE"), ("TransE", "RotatE")
LOSSES = list(O.LOSS_DEFAULTS)
SCALE = 0.3
LAYOUTS = {"given": dict(N=300, R=5, k=32, B=37, G=8, M=5), "identity": dict(N=40, R=2, k=8, B=37, G=8, M=40)}
MIN_UNIT = {"TransE": 1e-6, "RotatE": 1e-3}      # tests/test_gpu_shared_dist.py's preconditions, here over the FINITE pair-units
MIN_X = 0.05

OWN = ("own_nan_row", "own_nan_unit", "own_inf_unit", "rel_nan_unit")
LIST = ("list_nan_row", "list_nan_unit", "list_inf_unit")
OWN_PLANTS = tuple(f"{p}@{w}" for p in OWN for w in ("replaced", "kept"))

# entry point -> (engine method, models, layout, masked)
ENTRIES = {"shared": ("train_shared_fwdbwd", GEMM_MODELS, "given", False),
           "masked_given": ("train_shared_masked_fwdbwd", GEMM_MODELS, "given", True),
           "masked_identity": ("train_shared_masked_fwdbwd", GEMM_MODELS, "identity", True),
           "dist": ("train_shared_dist_fwdbwd", DIST_MODELS, "given", False),
           "dist_given": ("train_shared_dist_fwdbwd", DIST_MODELS, "given", True),
           "dist_identity": ("train_shared_dist_fwdbwd", DIST_MODELS, "identity", True)}

# (model, layout) -> the first seed, counting from 1, for which every plant of the layout meets the conditions of
# tests/test_shared_nonfinite_host.py (found by find_seed on the CPU; the contraction models have no conditioning precondition)
SEEDS = {("DistMult", "given"): 1, ("DistMult", "identity"): 1, ("ComplEx", "given"): 1, ("ComplEx", "identity"): 1,
         ("HolE", "given"): 1, ("HolE", "identity"): 1,
         ("TransE", "given"): 4, ("TransE", "identity"): 1, ("RotatE", "given"): 2, ("RotatE", "identity"): 1}


def plants_of(entry, model):
    _, _, layout, masked = ENTRIES[entry]
    if layout == "identity":     # (one list for every group: the lone entry of ONE list does not exist)
        return OWN_PLANTS + ("masked_nan_row",)
    extra = (("masked_nan_row",) + (("masked_was_inf",) if model in DIST_MODELS else ())) if masked else ()
    return OWN_PLANTS + LIST + extra


def all_cases():
    """-> [(entry, model, plant)] of test_shared_nonfinite_loss_and_gradients (each runs every loss)"""
    return [(e, m, p) for e, (_, models, _, _) in ENTRIES.items() for m in models for p in plants_of(e, m)]


def is_inf_plant(plant):
    return "inf" in plant


class Case:
    """What one step takes (ent, rel: the PLANTED tables) and what the tests ask about it."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def negs(self):
        return SR.override_rows(self.X, self.G, self.ids, self.side)

    def mask_matrix(self):
        """-> (mask [B, M], masked, unmaskable) of the masked entry points"""
        return MR.mask_matrix(self.X, self.G, self.ids, self.side, self.ks, self.ko)

    def group_rows(self, groups):
        """-> (entity rows, relation rows) used by the positives or the lists of `groups`"""
        grp = np.arange(self.B) // self.G
        sel = np.isin(grp, list(groups))
        ents = set(self.X[sel, 0].tolist()) | set(self.X[sel, 2].tolist()) | set(self.ids[list(groups)].ravel().tolist())
        return ents, set(self.X[sel, 1].tolist())

    def clean_rows(self):
        """-> (entity rows, relation rows) that belong ONLY to groups other than 1"""
        others = [g for g in range(self.ids.shape[0]) if g != 1]
        e1, r1 = self.group_rows([1])
        eo, ro = self.group_rows(others)
        return sorted(eo - e1), sorted(ro - r1)


def tables(model, k, N, R, seed, scale=SCALE):
    rng = np.random.default_rng(seed)
    K = O.internal_k(model, k)
    return (rng.normal(size=(N, K)) * scale).astype(np.float32), (rng.normal(size=(R, K)) * scale).astype(np.float32)


def spoil(row, kind):
    if kind.endswith("nan_row"):
        row[:] = np.nan
    elif kind.endswith("nan_unit"):
        row[3] = np.nan
    else:
        row[5] = np.inf


def _graph_and_batch(seed, B, N, R, reserved):
    """a graph dense enough that ranges hold several ids, and a batch cut from it; `reserved` is in neither"""
    rng = np.random.default_rng(seed)

    def ents(n):
        v = rng.integers(0, N - 1, n)
        return v + (v >= reserved)

    n = 6 * N
    D = np.stack([ents(n), rng.integers(0, R, n), ents(n)], 1).astype(np.int32)
    return D, D[rng.integers(0, n, B)]


@functools.lru_cache(maxsize=None)
def _build(model, layout, plant, seed):
    L = LAYOUTS[layout]
    N, R, k, B, G, M = (L[x] for x in ("N", "R", "k", "B", "G", "M"))
    ent, rel = tables(model, k, N, R, seed)
    if layout == "identity":
        lone = 2
        D, X = _graph_and_batch(seed, B, N, R, lone)
        ids = np.tile(np.arange(M, dtype=np.int32), (SR.n_groups(B, G), 1))
        side = SR.sample_shared(X, G, 1, seed, 4, sample_range=N)[1]
    else:
        D, X = _graph_and_batch(seed, B, N, R, N - 1)
        ids, side = SR.sample_shared(X, G, M, seed, 4, sample_range=N - 1)
        lone = N - 1
        ids[1, 2] = lone
    assert lone not in X[:, [0, 2]] and (ids == lone).sum() == (ids.shape[0] if layout == "identity" else 1)
    ks, ko = MR.known_lists(X, [D], N, R)
    if layout == "given":        # some mask away from group 1 whatever the draw hit
        for i, j in ((3, 1), (20, 0)):
            ks[i] = np.union1d(ks[i], ids[i // G, j]).astype(np.int32)
            ko[i] = np.union1d(ko[i], ids[i // G, j]).astype(np.int32)
    kind, _, where = plant.partition("@")
    if kind in OWN:
        side[0] = 1 if where == "replaced" else 0
        if kind == "rel_nan_unit":
            rel[int(X[0, 1]), 2] = np.nan
        else:
            spoil(ent[int(X[0, 0])], kind)
    else:
        spoil(ent[lone], "list_inf_unit" if kind == "masked_was_inf" else "list_nan_row" if kind == "masked_nan_row" else kind)
        if kind.startswith("masked"):
            for i in (range(0, B, 2) if layout == "identity" else (8, 10, 12, 14)):
                ks[i] = np.union1d(ks[i], lone).astype(np.int32)
                ko[i] = np.union1d(ko[i], lone).astype(np.int32)
    assert 0 < side.sum() < B                                               # both sides in the batch
    for a in (ent, rel, X, ids, side, *ks, *ko):
        a.setflags(write=False)
    return Case(model=model, layout=layout, plant=plant, kind=kind, seed=seed, N=N, R=R, k=k, B=B, G=G, M=M, ent=ent, rel=rel, X=X, ids=ids,
                side=side, ks=ks, ko=ko, lone=lone, identity=layout == "identity")


def build(entry, model, plant):
    layout = ENTRIES[entry][2]
    return _build(model, layout, plant, SEEDS[model, layout])


# ---------------------------------------------------------------------------------------------------------- the oracle on a case
def oracle(case, loss, masked, reduction="sum"):
    """The definition on the case: O.dense_gradients on the override rows, or MR.masked_step(finite=False) with the case's mask
    -> (loss sum, G_ent, G_rel, positive scores, corruption scores [M * B] with -inf at the mask)"""
    with np.errstate(all="ignore"):
        if masked:
            return MR.masked_step(case.model, case.ent, case.rel, case.X, case.G, case.ids, case.side, case.mask_matrix()[0], loss, reduction, case.R, finite=False)
        _, Te, Tr, (sp, sn, per) = O.dense_gradients(case.model, case.ent, case.rel, case.X, case.negs, case.M, loss, None, reduction, case.R)
        return float(per.astype(np.float64).sum()), Te, Tr, sp, sn


def bad_rows(G):
    return ~np.isfinite(np.asarray(G, dtype=np.float64)).all(1)


def conditioning(model, ent, rel, X, G, ids, side, R, mask=None):
    """-> (the smallest FINITE |s + p - o| / |s o r - o| over every unit of the positives and the override rows, in fp64 -- the figure
    of test_gpu_shared_dist.min_unit_fp64 --, the smallest finite x = (sum eN / M) / eP of assert_softmax_conditioned over the
    positives, masked corruptions out of the sum)"""
    import shared_dist_ref as DR

    rows = np.concatenate([np.asarray(X, dtype=np.int64), SR.override_rows(X, G, ids, side).astype(np.int64)])
    with np.errstate(all="ignore"):
        s, p, o = (a.astype(np.float64) for a in O.lookup(ent, rel, rows))
        if model == "TransE":
            unit = np.abs(s + p - o)
        else:
            k = ent.shape[1] // 2
            phi = (rel[rows[:, 1], :k] / O.rotate_phase_divisor(k, R)).astype(np.float32).astype(np.float64)
            c, sn = np.cos(phi), np.sin(phi)
            re = s[:, :k] * c - s[:, k:] * sn - o[:, :k]
            im = s[:, :k] * sn + s[:, k:] * c - o[:, k:]
            unit = np.sqrt(re * re + im * im)
        st = DR.DistStep(model, ent, rel, X, G, ids, side, R)
        eN = np.exp(st.neg_matrix)
        if mask is not None:
            eN = np.where(mask, 0.0, eN)
        x = eN.sum(1) / st.M / np.exp(st.pos_scores)
    return float(unit[np.isfinite(unit)].min()), float(x[np.isfinite(x)].min(initial=np.inf))


def bad_rows_in_bounds(case, n):
    """condition (b): at least one non-finite entity-gradient row and fewer than N / 2, so that the comparison of the row SETS can
    fail either way.  Two exceptions, both the oracle's own answer: sign(+-inf) is finite, so an inf in a TransE table reaches no
    gradient row unless a whole score row is -inf under self_adversarial; and in the identity layout the spoiled entity is in the
    list of EVERY group (N = M = 40: it touches the kept row of all 37 positives, and with a softmax coefficient all 40 list rows),
    where the bound is N."""
    if case.model == "TransE" and is_inf_plant(case.plant) and n == 0:
        return True
    return 1 <= n <= case.N if case.identity else 1 <= n < case.N / 2


def case_is_sound(entry, case):
    """conditions (a) - (d) of tests/test_shared_nonfinite_host.py on one case, every loss -> None, or what fails"""
    masked = ENTRIES[entry][3]
    e1, r1 = case.group_rows([1])
    _, _, _, sp, sn = oracle(case, "nll", False)                            # (a): the scores before any mask
    if np.isfinite(sp).all() and np.isfinite(sn).all():
        return "every score is finite"
    if masked and case.kind.startswith("masked"):                           # the planted entry is masked for some rows of its list, not for all
        col = case.mask_matrix()[0][:, 2]
        rows = np.nonzero(case.ids[np.arange(case.B) // case.G, 2] == case.lone)[0]
        if not 0 < col[rows].sum() < len(rows):
            return "the planted entry is masked for none or for all of its rows"
    for loss in LOSSES:
        L, Te, Tr, sp, sn = oracle(case, loss, masked)
        bad = np.nonzero(bad_rows(Te))[0]
        if not bad_rows_in_bounds(case, len(bad)):
            return f"{loss}: {len(bad)} non-finite entity-gradient rows"
        if case.kind in LIST and not (set(bad.tolist()) <= e1 and set(np.nonzero(bad_rows(Tr))[0].tolist()) <= r1):
            return f"{loss}: a non-finite row outside group 1"
    if case.model in DIST_MODELS:
        unit, x = conditioning(case.model, case.ent, case.rel, case.X, case.G, case.ids, case.side, case.R, case.mask_matrix()[0] if masked else None)
        if not unit > MIN_UNIT[case.model]:
            return f"a pair-unit of {unit:.3g}"
        if not x > MIN_X:
            return f"a softmax ratio of {x:.3g}"
    return None


def find_seed(model, layout, limit=200):
    """the first seed for which every case of (model, layout), at every entry point that uses the layout, is sound"""
    for seed in range(1, limit):
        ok = True
        for entry, (_, models, lay, _) in ENTRIES.items():
            if lay != layout or model not in models:
                continue
            for plant in plants_of(entry, model):
                if case_is_sound(entry, _build(model, layout, plant, seed)) is not None:
                    ok = False
                    break
            if not ok:
                break
        if ok:
            return seed
    raise RuntimeError((model, layout))


# ---------------------------------------------------------------------------------------------------------- the tile edges
# (model, k) -> {(G, M): seed}: the first, counting from 1, whose finite pair-units meet MIN_UNIT (find_geometry_seed)
GEOMETRY_SEEDS = {("DistMult", 7): {(37, 33): 1, (37, 65): 1, (5, 33): 1, (5, 65): 1},
                  ("ComplEx", 50): {(37, 33): 1, (37, 65): 1, (5, 33): 1, (5, 65): 1},
                  ("TransE", 7): {(37, 33): 1, (37, 65): 1, (5, 33): 1, (5, 65): 2},
                  ("RotatE", 50): {(37, 33): 1, (37, 65): 1, (5, 33): 1, (5, 65): 1}}


@functools.lru_cache(maxsize=None)
def _geometry(model, k, G, M, seed):
    N, R, B = 200, 4, 37
    ent, rel = tables(model, k, N, R, seed)
    lone = N - 1
    _, X = _graph_and_batch(seed, B, N, R, lone)
    ids, side = SR.sample_shared(X, G, M, seed, 4, sample_range=N - 1)
    ids[min(1, ids.shape[0] - 1), M - 1] = lone                              # the lone column of the second tile / the chunks' tail of 1
    ent[lone, :] = np.nan
    own = int(X[B - 1, 0] if side[B - 1] else X[B - 1, 2])                   # the replaced entity of the LAST positive: the short group
    ent[own, k - 1] = np.nan                                                 # ... its last live unit, next to the padding
    assert 0 < side.sum() < B
    for a in (ent, rel, X, ids, side):
        a.setflags(write=False)
    return Case(model=model, layout="geometry", plant="geometry", kind="geometry", seed=seed, N=N, R=R, k=k, B=B, G=G, M=M, ent=ent, rel=rel, X=X,
                ids=ids, side=side, ks=None, ko=None, lone=lone, identity=False)


def geometry_case(model, k, G, M):
    return _geometry(model, k, G, M, GEOMETRY_SEEDS[model, k][G, M])


def geometry_is_sound(case):
    for loss in ("nll", "self_adversarial"):
        L, Te, Tr, sp, sn = oracle(case, loss, False)
        if np.isfinite(sn).all() or not 1 <= bad_rows(Te).sum() < case.N:
            return loss
    if case.model in DIST_MODELS:
        unit, _ = conditioning(case.model, case.ent, case.rel, case.X, case.G, case.ids, case.side, case.R)
        if not unit > MIN_UNIT[case.model]:
            return f"a pair-unit of {unit:.3g}"
    return None


def find_geometry_seed(model, k, G, M, limit=200):
    for seed in range(1, limit):
        if geometry_is_sound(_geometry(model, k, G, M, seed)) is None:
            return seed
    raise RuntimeError((model, k, G, M))
