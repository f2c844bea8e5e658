"""The draw of amdkge_sample_shared (include/amdkge_shared.h) restated in numpy on top of oracle/philox.py, and the DEFINITION of the
shared-negative step: (ids, sides) -> the override rows amdkge_train_fwdbwd and oracle.kge_oracle.dense_gradients take.  Test
infrastructure: the product does not import it."""
import numpy as np

from negatives_ref import BERNOULLI, O_ONLY, S_ONLY, SIDE_NAMES, UNIFORM, mulhi   # noqa: F401  (the side modes are include/amdkge_negatives.h's)
from oracle.philox import philox4x32_10

TAG_IDS, TAG_SIDE = 0xF0 << 24, 0xF1 << 24
MAX_NEGS = (1 << 24) - 1


def _philox_x(c0, c1, step, seed):
    step, seed = int(step), int(seed)
    return philox4x32_10(np.asarray(c0, dtype=np.uint32), np.asarray(c1, dtype=np.uint32), np.uint32(step & 0xFFFFFFFF), np.uint32((step >> 32) & 0xFFFFFFFF),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def n_groups(B, G):
    return 0 if B == 0 else -(-B // min(G, B))


def sample_shared(triples, G, M, seed, step, sample_base=0, sample_range=None, side_mode=UNIFORM, side_thr=None, pool=None):
    """-> (ids int32 [n_groups, M], side int32 [B]; 1 = the subject is replaced)"""
    X = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    B = X.shape[0]
    assert G >= 1 and 1 <= M <= MAX_NEGS
    ng = n_groups(B, G)
    g = np.repeat(np.arange(ng, dtype=np.uint32), M)
    j = np.tile(np.arange(M, dtype=np.uint32), ng)
    x = _philox_x(g, j | np.uint32(TAG_IDS), step, seed)
    ids = np.asarray(pool, dtype=np.int64)[mulhi(x, len(pool))] if pool is not None else sample_base + mulhi(x, sample_range)
    if side_mode in (S_ONLY, O_ONLY):
        subj = np.full(B, side_mode == S_ONLY)
    else:
        i = np.arange(B, dtype=np.uint64)
        c = _philox_x((i & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32) | np.uint32(TAG_SIDE), step, seed)
        subj = c < np.asarray(side_thr, dtype=np.uint32)[X[:, 1]] if side_mode == BERNOULLI else (c & np.uint32(1)) == 0
    return ids.astype(np.int32).reshape(ng, M), subj.astype(np.int32)


def override_rows(triples, G, ids, side):
    """The definition: neg[j * B + i] = positive i with its side[i] entity replaced by ids[i // G][j]  -> int32 [(B * M), 3]"""
    X = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    B, M = X.shape[0], ids.shape[1]
    G = min(G, max(B, 1))
    i = np.tile(np.arange(B), M)
    j = np.repeat(np.arange(M), B)
    repl = np.asarray(ids, dtype=np.int64)[i // G, j]
    subj = np.asarray(side)[i] != 0
    return np.stack([np.where(subj, repl, X[i, 0]), X[i, 1], np.where(subj, X[i, 2], repl)], 1).astype(np.int32)
