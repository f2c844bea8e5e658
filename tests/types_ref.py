"""Relation sets and the typed draw (include/amdkge_types.h), restated in numpy: the set build, the range lookup with min_size and
fallback, and amdkge_sample_negatives_typed's draw on top of tests/negatives_ref.py's Philox blocks.  Test infrastructure: the
product does not import it."""
import numpy as np

import negatives_ref as NR


def build_sets(triples, side):
    """(keys int64, start int64, ids int32): the distinct subjects (side "s") or objects ("o") per relation, relations ascending,
    ids ascending inside a set -- by Python sets, not by the sort the product uses"""
    col = 0 if side == "s" else 2
    sets = {}
    for t in np.asarray(triples).reshape(-1, 3).tolist():
        sets.setdefault(int(t[1]), set()).add(int(t[col]))
    keys = sorted(sets)
    start, ids = [0], []
    for r in keys:
        ids += sorted(sets[r])
        start.append(len(ids))
    return np.array(keys, np.int64), np.array(start, np.int64), np.array(ids, np.int32)


def ranges(keys, start, triples, min_size=0, fallback=(0, 0)):
    """(lo, hi) int64 [n]: the range of each triple's relation; the fallback for an absent relation or a set below min_size"""
    where = {int(r): g for g, r in enumerate(keys)}
    lo, hi = [], []
    for t in np.asarray(triples).reshape(-1, 3).tolist():
        g = where.get(int(t[1]))
        if g is not None and int(start[g + 1] - start[g]) >= min_size:
            lo.append(int(start[g])), hi.append(int(start[g + 1]))
        else:
            lo.append(int(fallback[0])), hi.append(int(fallback[1]))
    return np.array(lo, np.int64), np.array(hi, np.int64)


def sample_negatives_typed(triples, eta, seed, step, sample_base=0, sample_range=None, row_offset=0, b_global=0, side_mode=NR.UNIFORM,
                           side_thr=None, pool=None, s_filter=None, o_filter=None, max_tries=8, s_cand=None, o_cand=None):
    """-> (int32 [(B * eta), 3] with row j * B + i, redraws, exhausted, untyped).  s_filter / o_filter, s_cand / o_cand: (lo [B], hi [B],
    ids) or None.  One corruption at a time, in the header's words."""
    X = np.asarray(triples, dtype=np.int64)
    B = X.shape[0]
    bg = b_global if b_global > 0 else B
    assert eta * bg < 2 ** 56 and 1 <= max_tries <= 32 and (s_filter is None) == (o_filter is None) and (s_cand is None) == (o_cand is None)
    i = np.tile(np.arange(B, dtype=np.int64), eta)
    j = np.repeat(np.arange(eta, dtype=np.int64), B)
    rows = (j * bg + row_offset + i).astype(np.uint64)
    n = B * eta
    n_blocks = (max_tries + 2) // 3
    blocks = [NR.block(rows, step, seed, b) for b in range(n_blocks)] if n else []
    out = np.zeros((n, 3), dtype=np.int32)
    redraws = exhausted = untyped = 0
    for r in range(n):
        q = int(i[r])
        s, p, o = (int(v) for v in X[q])
        x = int(blocks[0][0][r])
        if side_mode == NR.UNIFORM:
            subj = (x & 1) == 0
        elif side_mode == NR.BERNOULLI:
            subj = x < int(np.asarray(side_thr, dtype=np.uint32)[p])
        else:
            subj = side_mode == NR.S_ONLY
        cand = (s_cand if subj else o_cand) if s_cand is not None else None
        clo, chi = (int(cand[0][q]), int(cand[1][q])) if cand is not None else (0, 0)
        if chi == clo:
            untyped += 1
        flt = (s_filter if subj else o_filter) if s_filter is not None else None
        known = set(np.asarray(flt[2][int(flt[0][q]):int(flt[1][q])]).tolist()) if flt is not None else set()
        for t in range(max_tries):
            word = int(blocks[t // 3][1 + t % 3][r])
            if chi > clo:
                repl = int(cand[2][clo + ((word * (chi - clo)) >> 32)])
            elif pool is not None:
                repl = int(pool[(word * len(pool)) >> 32])
            else:
                repl = sample_base + ((word * sample_range) >> 32)
            if repl not in known:
                break
            if t == max_tries - 1:
                exhausted += 1
        redraws += t
        out[r] = (repl, p, o) if subj else (s, p, repl)
    return out, redraws, exhausted, untyped
