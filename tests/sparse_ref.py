"""The sparse optimizer mode (include/ext/amdkge_sparse.h) restated in numpy on top of the oracle (TEST INFRASTRUCTURE): the candidate
rows of a step and the sweep of a list of rows.  The sweep is oracle.kge_oracle.apply_optimizer_lazy restricted to the listed entity
rows -- on a list that covers every entity row with a non-zero gradient it IS apply_optimizer_lazy(ent_mask=None), which
tests/test_sparse_host.py holds it to."""
import numpy as np

from oracle import kge_oracle as O


def candidate_rows(X, ids=None):
    """int triples [B, 3] and the step's list ids (any shape, or None) -> the ascending unique union of s, o and the ids, int32"""
    X = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    parts = [X[:, 0], X[:, 2]] + ([] if ids is None else [np.asarray(ids, dtype=np.int64).reshape(-1)])
    return np.unique(np.concatenate(parts)).astype(np.int32)


def nonzero_rows(G):
    """the oracle's "gradient row is not entirely zero in fp32" (apply_optimizer_lazy's own rule)"""
    return np.any(np.abs(np.asarray(G, dtype=np.float64)) >= float(np.finfo(np.float32).tiny), axis=1)


def sweep_rows(state, Ge, Gr, rows, reg=None):
    """One sweep of the mode on an oracle TrainState, in place: the entity rows that are LISTED and have a non-zero gradient row get
    regulariser and update rule, every other entity row keeps x and slots; the relation table is swept by its non-zero rows.
    -> (regulariser loss, the entity gradient table afterwards: listed rows reset, rows that are not listed untouched)"""
    listed = np.zeros(state.ent.shape[0], dtype=bool)
    listed[np.asarray(rows, dtype=np.int64)] = True
    reg_loss = O.apply_optimizer_lazy(state, Ge, Gr, reg, ent_mask=listed & nonzero_rows(Ge))
    left = np.array(Ge, dtype=np.float32)
    left[listed] = 0.0
    return reg_loss, left
