"""Per-triple candidate lists for evaluate_candidates(): the two accepted forms -> one CSR (pure numpy, no device)."""
import numpy as np


def _int_ids(a, what):
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros(a.shape, dtype=np.int32)
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: candidate ids must be integers (index the labels first), got dtype {a.dtype}")
    if a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max:
        raise ValueError(f"{what}: candidate ids do not fit int32")
    return a.astype(np.int32, copy=False)


def list_lengths(lists, n):
    """Lengths int64 [n] of the n candidate lists in either accepted form -- a 2-D array [n, C] or a sequence of n 1-D
    arrays -- and the lists' elements flattened in list order (dtype as given: labels or ids).  ValueError when the number of
    lists is not n or a list is not 1-D."""
    n = int(n)
    if isinstance(lists, np.ndarray) and lists.ndim == 2:
        if lists.shape[0] != n:
            raise ValueError(f"{lists.shape[0]} candidate lists for {n} triples")
        return np.full(n, lists.shape[1], dtype=np.int64), lists.reshape(-1)
    if isinstance(lists, np.ndarray) and lists.dtype != object and lists.ndim != 1:
        raise ValueError(f"candidate lists: expected a 2-D array [n, C] or a sequence of n 1-D arrays, got shape {lists.shape}")
    rows = [np.asarray(r) for r in lists]
    if len(rows) != n:
        raise ValueError(f"{len(rows)} candidate lists for {n} triples")
    for i, r in enumerate(rows):
        if r.ndim != 1:
            raise ValueError(f"candidate list {i} is not 1-D (shape {r.shape})")
    lens = np.fromiter((r.shape[0] for r in rows), dtype=np.int64, count=n)
    filled = [r for r in rows if r.shape[0]]
    flat = np.concatenate(filled) if filled else np.zeros(0, dtype=np.int32)
    return lens, flat


def as_csr(lists, n):
    """Candidate lists of n triples -> (offsets int64 [n + 1], ids int32 [offsets[n]], max_len): list i is
    ids[offsets[i]:offsets[i + 1]], max_len the longest list's length (0 when there is none).  `lists` is a 2-D integer array
    [n, C] (every list has C entries; pad a shorter one with -1, which is no candidate) or a sequence of n 1-D integer arrays
    (ragged).  ValueError for a wrong number of lists, a list that is not 1-D, or ids that are not integers."""
    return csr_of(*list_lengths(lists, n))


def csr_of(lens, flat_ids):
    """as_csr's result from the lists' lengths and their ids flattened in list order."""
    off = np.zeros(lens.shape[0] + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = np.ascontiguousarray(_int_ids(flat_ids, "candidate lists"))
    if ids.shape[0] != off[-1]:
        raise ValueError(f"{ids.shape[0]} candidate ids for lists of {int(off[-1])} entries in all")
    return off, ids, int(lens.max()) if lens.size else 0
