"""The masked shared-negative step (include/amdkge_shared_mask.h) restated in numpy on top of tests/shared_ref.py and the oracle:
which corruption scores are known statements (mask_matrix, with the fully-known exception and both counts) and the whole step on
the equivalent override rows with those scores at -inf (masked_step).  Test infrastructure: the product does not import it."""
import numpy as np

import shared_ref as SR
from oracle import kge_oracle as O


def known_lists(triples, datasets, N, R):
    """-> (known_s, known_o): per positive the ascending unique subjects known with its (p, o) / objects known with its (s, p) in
    the concatenation of `datasets` (what FilterIndex + its range lookup give)"""
    X = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    D = np.concatenate([np.asarray(d, dtype=np.int64).reshape(-1, 3) for d in datasets], 0) if len(datasets) else np.zeros((0, 3), np.int64)
    ks, ko = [], []
    for s, p, o in X:
        ks.append(np.unique(D[(D[:, 1] == p) & (D[:, 2] == o), 0]).astype(np.int32))
        ko.append(np.unique(D[(D[:, 0] == s) & (D[:, 1] == p), 2]).astype(np.int32))
    return ks, ko


def csr(lists):
    """per-row id lists -> (lo int64 [B], hi int64 [B], ids int32 [>= 1]); an empty list is the range (0, 0)"""
    lens = np.array([len(a) for a in lists], dtype=np.int64)
    hi = np.cumsum(lens)
    lo = hi - lens
    lo[lens == 0] = 0
    hi = np.where(lens == 0, 0, hi)
    ids = np.concatenate([np.asarray(a, dtype=np.int32) for a in lists] + [np.zeros(0, np.int32)])
    return lo.astype(np.int64), hi.astype(np.int64), ids if ids.size else np.zeros(1, np.int32)


def mask_matrix(X, G, ids, side, known_s, known_o):
    """-> (mask bool [B, M], masked count, unmaskable count): mask[i, j] = ids[i // G][j] is in known_i (known_s[i] when side[i],
    else known_o[i]); a row that would be ALL True is all False instead and counted as unmaskable"""
    X = np.asarray(X).reshape(-1, 3)
    B, M = X.shape[0], np.asarray(ids).shape[1]
    G = min(G, max(B, 1))
    mask = np.zeros((B, M), dtype=bool)
    unmaskable = 0
    for i in range(B):
        known = known_s[i] if side[i] else known_o[i]
        row = np.isin(np.asarray(ids)[i // G], np.asarray(known))
        if row.all():
            unmaskable += 1
        else:
            mask[i] = row
    return mask, int(mask.sum()), unmaskable


def masked_step(model, ent, rel, X, G, ids, side, mask, loss, reduction, R, loss_params=None, finite=True):
    """The definition: the shared step on SR.override_rows with the scores at `mask` set to -inf before the loss.
    -> (loss sum float, G_ent fp64, G_rel fp64, positive scores [B], corruption scores [M * B] with -inf at the mask)
    finite=True asserts that the tables gave finite numbers throughout.  finite=False is for tables that hold a NaN or an inf: a
    masked coefficient is an exact zero TIMES the score's Jacobian, so a masked corruption of a non-finite row sends NaN to the
    rows it was computed from, exactly as a clipped score does (tests/test_shared_nonfinite_host.py)."""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    B, M = X.shape[0], ids.shape[1]
    negs = SR.override_rows(X, G, ids, side).astype(np.int64)
    s, p, o = O.lookup(ent, rel, X)
    ns, npr, no = O.lookup(ent, rel, negs)
    sp = O.compute_scores(model, s, p, o, max_rel_size=R)
    sn = np.array(O.compute_scores(model, ns, npr, no, max_rel_size=R), dtype=np.float32)
    sn[np.asarray(mask).T.reshape(-1)] = -np.inf           # row j * B + i
    with np.errstate(invalid="ignore", over="ignore"):
        total, per, dP, dN = O.loss_and_grads(loss, sp, sn, M, loss_params, reduction)
    if finite:
        assert np.isfinite(per).all() and np.isfinite(dP).all() and np.isfinite(dN).all() and not dN[np.asarray(mask).T.reshape(-1)].any()
    Ge = np.zeros(ent.shape, dtype=np.float64)
    Gr = np.zeros(rel.shape, dtype=np.float64)
    with np.errstate(invalid="ignore" if not finite else "warn"):
        for tri, (a, b, c), g in ((X, (s, p, o), dP), (negs, (ns, npr, no), dN)):   # (dense_gradients' accumulation)
            gs, gp, go = O.score_grads(model, a, b, c, R)
            g = g.astype(np.float64)[:, None]
            np.add.at(Ge, tri[:, 0], g * gs)
            np.add.at(Gr, tri[:, 1], g * gp)
            np.add.at(Ge, tri[:, 2], g * go)
    return float(per.astype(np.float64).sum()), Ge, Gr, sp, sn
