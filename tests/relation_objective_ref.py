"""The relation-prediction training objective (include/amdkge_relation_objective.h) restated in numpy on top of the oracle: the
override rows (s_i, j, o_i), which relation scores are known statements (with the fully-known exception and both counts) and the
whole step on those rows with the known scores at -inf, times the weight.  Test infrastructure: the product does not import it."""
import numpy as np

from oracle import kge_oracle as O


def override_rows(X, R):
    """-> int64 [R * B, 3]: row j * B + i = (s_i, j, o_i)"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    B = X.shape[0]
    negs = np.tile(X, (R, 1))
    negs[:, 1] = np.repeat(np.arange(R, dtype=np.int64), B)
    return negs


def known_relations(X, datasets):
    """-> per positive the ascending unique relations known between its (s, o) in the concatenation of `datasets` (what
    PairFilterIndex + its range lookup give)"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    D = np.concatenate([np.asarray(d, dtype=np.int64).reshape(-1, 3) for d in datasets], 0) if len(datasets) else np.zeros((0, 3), np.int64)
    return [np.unique(D[(D[:, 0] == s) & (D[:, 2] == o), 1]).astype(np.int32) for s, _, o in X]


def csr(lists):
    """per-row id lists -> (lo int64 [B], hi int64 [B], ids int32 [>= 1]); an empty list is the range (0, 0)"""
    lens = np.array([len(a) for a in lists], dtype=np.int64)
    hi = np.cumsum(lens)
    lo = hi - lens
    lo[lens == 0] = 0
    hi = np.where(lens == 0, 0, hi)
    ids = np.concatenate([np.asarray(a, dtype=np.int32) for a in lists] + [np.zeros(0, np.int32)])
    return lo.astype(np.int64), hi.astype(np.int64), ids if ids.size else np.zeros(1, np.int32)


def mask_matrix(B, R, known):
    """-> (mask bool [B, R], masked count, unmaskable count): mask[i, j] = j in known[i] (ids >= R ignored); a row that would be ALL
    True is all False instead and counted as unmaskable.  known=None: nothing is masked."""
    mask = np.zeros((B, R), dtype=bool)
    unmaskable = 0
    if known is None:
        return mask, 0, 0
    for i in range(B):
        row = np.isin(np.arange(R), np.asarray(known[i]))
        if row.all():
            unmaskable += 1
        else:
            mask[i] = row
    return mask, int(mask.sum()), unmaskable


def relation_step(model, ent, rel, X, mask, loss, reduction, weight=1.0, loss_params=None, finite=True, dtype=np.float64, magnitude=False):
    """The definition: amdkge_train_fwdbwd's step with eta = R on override_rows, the scores at `mask` [B, R] set to -inf before the
    loss, loss and gradients times `weight`.
    -> (weight * loss sum, G_ent, G_rel (accumulated in `dtype`), positive scores [B], relation scores [R * B] with -inf at the mask)
    finite=False is for tables that hold a NaN or an inf: a masked coefficient is an exact zero TIMES the score's Jacobian.
    magnitude=True appends (A_ent, A_rel): the sums of the ABSOLUTE values of the contributions G_ent / G_rel add up -- the scale of a
    gradient whose contributions cancel (R = 1: the one "corruption" is the positive itself, dL/dpos = -dL/dneg)."""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    B, R = X.shape[0], rel.shape[0]
    negs = override_rows(X, R)
    s, p, o = O.lookup(ent, rel, X)
    ns, npr, no = O.lookup(ent, rel, negs)
    with np.errstate(invalid="ignore", over="ignore"):
        sp = O.compute_scores(model, s, p, o, max_rel_size=R)
        sn = np.array(O.compute_scores(model, ns, npr, no, max_rel_size=R), dtype=np.float32)
    flat = np.asarray(mask).T.reshape(-1)                   # row j * B + i
    sn[flat] = -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        total, per, dP, dN = O.loss_and_grads(loss, sp, sn, R, loss_params, reduction)
    if finite:
        assert np.isfinite(per).all() and np.isfinite(dP).all() and np.isfinite(dN).all() and not dN[flat].any()
    Ge = np.zeros(ent.shape, dtype=dtype)
    Gr = np.zeros(rel.shape, dtype=dtype)
    Ae, Ar = np.zeros(ent.shape, dtype=dtype), np.zeros(rel.shape, dtype=dtype)
    w = dtype(weight)
    with np.errstate(invalid="ignore", over="ignore"):
        for tri, (a, b, c), g in ((X, (s, p, o), dP), (negs, (ns, npr, no), dN)):   # (dense_gradients' accumulation)
            gs, gp, go = O.score_grads(model, a, b, c, R)
            g = (w * g.astype(dtype))[:, None]
            np.add.at(Ge, tri[:, 0], (g * gs).astype(dtype))
            np.add.at(Gr, tri[:, 1], (g * gp).astype(dtype))
            np.add.at(Ge, tri[:, 2], (g * go).astype(dtype))
            if magnitude:
                np.add.at(Ae, tri[:, 0], np.abs(g * gs).astype(dtype))
                np.add.at(Ar, tri[:, 1], np.abs(g * gp).astype(dtype))
                np.add.at(Ae, tri[:, 2], np.abs(g * go).astype(dtype))
        L = float(weight) * float(per.astype(np.float64).sum())
    return (L, Ge, Gr, sp, sn, Ae, Ar) if magnitude else (L, Ge, Gr, sp, sn)


def pair_queries(model, ent, X, k):
    """Q [B, K] in fp64: score(s_i, j, o_i) = scale * <Q_i, rel[j]> (scale: HolE's 2 / k, else 1)"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    s, o = ent[X[:, 0]].astype(np.float64), ent[X[:, 2]].astype(np.float64)
    if model == "DistMult":
        return s * o
    s0, s1, o0, o1 = s[:, :k], s[:, k:], o[:, :k], o[:, k:]
    return np.concatenate([s0 * o0 + s1 * o1, s0 * o1 - s1 * o0], 1)
