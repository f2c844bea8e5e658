"""Discovery helpers on the device: query_topn
(/root/reference/ampligraph/discovery/discovery.py:985-1168), find_nearest_neighbours (:1171-1244), find_duplicates
(:714-982) and find_clusters (:546-711).

The reference materialises one STRING triple per candidate, calls model.predict and argsorts on the host; its nearest
neighbours are sklearn on the host.  Here an entity completion is ONE query through the 1-vs-all corruption-score kernels
of evaluate() (amdkge_corruption_scores: same prep + tile kernels as the ranks) followed by a streaming top-k selection
kernel (amdkge_topk_rows); nearest neighbours are dot products on the same tile kernel with the norms folded into the
selection.  Only top_n ids / scores travel back.  Both work on a row-sharded entity table (per-shard lists, merged).
query_topn_batch (no counterpart in the reference) completes MANY (s, p, ?) or (?, p, o) queries in one call and leaves out the
statements already known to be true: the queries are the rows of chunked amdkge_corruption_scores calls, and each chunk's
selection (amdkge_topk_rows_excluding, kge_complete.hip) looks a column up in the query's range of the evaluate() filter index
before it may enter the list -- an exclusion inside the selection, so a known column is never a filler and -inf / NaN scores
stay scores.  Replicated placement only.
query_topn_relations (no counterpart either) answers "which relation holds between these two entities?" for MANY (s, o) pairs:
a 1-vs-all pass over the relation table that keeps the pairs' rows in registers (amdkge_relation_scores, kge_relation.hip: the
bits of predict on the materialised triples, nothing materialised), the same excluding selection with the relations already
known between a pair left out (PairFilterIndex, amdkge_pair_filter_build).  The relation table is whole on every rank, so it
works on every placement; ScoringBasedEmbeddingModel.evaluate_relations ranks the true relation with the same kernels.
find_duplicates is an exact self-join of the embeddings on the device (amdkge_join_nearest / amdkge_join_radius,
kge_join.hip); its tolerance bisection runs on the host over one nearest distance per row.  find_clusters runs DBSCAN -- its
default, and the reference's documented use -- on the same join (amdkge_join_dbscan: neighbour count, union-find over the core
rows, border pass; no pair list) and returns sklearn's labels; a KMeans of this module -- the estimator of the reference's
documented find_clusters use, Lloyd's iterations with every restart batched into the same launches (amdkge_kmeans_lloyd,
kge_kmeans.hip) -- gets the device matrix; other clustering objects get the downloaded embeddings.
discover_facts (:21-271) and generate_candidates (:274-519) are the reference's procedure on the host -- the same legacy
numpy draws in the same order, so equal inputs and seed give the reference's rows -- ranked by evaluate() on the device.
discover_facts also runs strategy="exhaustive", which the reference documents and then rejects: every (s, o) pair of a
relation, decided by two 1-vs-all score passes (amdkge_corruption_scores), a per-row selection of the columns that can
still rank within the cut-off (amdkge_discover_select, kge_discover.hip), the intersection of the two sides and exact ranks
of the survivors.
Same arguments, validation and error behaviour as the reference."""
import logging

import numpy as np

from . import _ffi

logger = logging.getLogger(__name__)

__all__ = ["discover_facts", "generate_candidates", "query_topn", "query_topn_batch", "query_topn_relations", "find_nearest_neighbours", "find_duplicates", "find_clusters", "KMeans"]


def _known(indexer, values, type_of):
    vals = np.asarray(values).reshape(-1)
    return len(indexer.get_indexes(vals, type_of)) == len(vals)


def _check_to_consider(ix, values, name, kind):
    """query_topn's checks of `ents_to_consider` / `rels_to_consider` (kind "e" / "r")"""
    if not isinstance(values, (list, np.ndarray)):
        raise ValueError("`{}` must be a list or numpy array.".format(name))
    if not _known(ix, values, kind):
        raise ValueError("{} in `{}` have not been seen by the model.".format("Entities" if kind == "e" else "Relations", name))


def query_topn(model, top_n=10, head=None, relation=None, tail=None, ents_to_consider=None, rels_to_consider=None):
    """Score every completion of the two given triple elements and return the top_n (triples (n,3) of raw labels,
    scores (n,) float32), ordered by decreasing score.  True statements are not filtered out (as in the reference)."""
    import torch

    if not model.is_fitted:
        raise ValueError("Model is not fitted.")
    if not np.sum([head is None, relation is None, tail is None]) == 1:
        raise ValueError("Exactly one of `head`, `relation` or `tail` arguments must be None.")
    ix = model.data_indexer
    if head and not _known(ix, [head], "e"):
        raise ValueError("Head entity `{}` not seen by model".format(head))
    if relation and not _known(ix, [relation], "r"):
        raise ValueError("Relation `{}` not seen by model".format(relation))
    if tail and not _known(ix, [tail], "e"):
        raise ValueError("Tail entity `{}` not seen by model".format(tail))
    if ents_to_consider is not None:
        if head and tail:
            raise ValueError("Cannot specify `ents_to_consider` and both `subject` and `object` arguments.")
        _check_to_consider(ix, ents_to_consider, "ents_to_consider", "e")
    if rels_to_consider is not None:
        if relation:
            raise ValueError("Cannot specify both `rels_to_consider` and `relation` arguments.")
        _check_to_consider(ix, rels_to_consider, "rels_to_consider", "r")
    eng, pl = model._engine, model._placement
    dev = eng.device
    one = lambda v, t: int(ix.get_indexes(np.asarray([v]), t)[0])   # noqa: E731

    if relation is None:   # complete the relation: a handful of candidates, scored as ordinary triples
        if rels_to_consider is None or len(rels_to_consider) == 0:
            cand = np.arange(model._n_rels, dtype=np.int32)
        else:
            cand = np.asarray(ix.get_indexes(np.asarray(rels_to_consider), "r"), dtype=np.int32)
        tri = np.stack([np.full_like(cand, one(head, "e")), cand, np.full_like(cand, one(tail, "e"))], 1)
        scores = pl.score(torch.as_tensor(tri).to(dev))
        n = min(int(top_n), len(cand))
        idx, val = eng.topk_rows(scores.view(1, -1), n)
        out = tri[idx[0].cpu().numpy().astype(np.int64)]
        return ix.get_indexes(out, "t", "ind2raw"), val[0].cpu().numpy().astype(np.float32)

    # complete an entity: 1-vs-all corruption scores of ONE query on the rank kernels + a top-k selection on the device
    side = _ffi.SIDE_O if tail is None else _ffi.SIDE_S
    fixed = one(head if tail is None else tail, "e")
    r_id = one(relation, "r")
    q = np.array([[fixed, r_id, fixed]], dtype=np.int32)   # the replaced column is ignored by the corruption scores
    cand_ids = None
    if ents_to_consider is not None and len(ents_to_consider) > 0:
        cand_ids = np.asarray(ix.get_indexes(np.asarray(ents_to_consider), "e"), dtype=np.int64)
    n_cand = model._n_ents if cand_ids is None else len(cand_ids)
    n = min(int(top_n), n_cand)
    # (top_n > 1024: engine.topk_rows sorts the whole score row on the device instead of the streaming selection)
    ql = pl.localise(torch.as_tensor(q).to(dev))   # (row-sharded table: the query's own rows are fetched behind the shard)
    ents, val = pl.select(lambda ids, hi, kk: eng.corruption_topk(ql, side, kk, ent_ids=ids, ent_hi=hi), cand_ids, 1, n)
    ents, val = ents[0], val[0]
    rel_col = np.full(n, r_id, dtype=np.int64)
    fix_col = np.full(n, fixed, dtype=np.int64)
    out = np.stack([fix_col, rel_col, ents], 1) if tail is None else np.stack([ents, rel_col, fix_col], 1)
    return ix.get_indexes(out, "t", "ind2raw"), val.astype(np.float32)


TOPN_BATCH_MAX = 1024   # amdkge_topk_rows_excluding's largest k


def _ids_or_fail(ix, labels, kind):
    """ids of `labels` (a 1-d array), or ValueError naming the ones the model has not seen (get_indexes drops them silently)."""
    got = np.asarray(ix.get_indexes(labels, kind), dtype=np.int64)
    if len(got) != len(labels):
        unseen = [u for u in dict.fromkeys(labels.tolist()) if len(ix.get_indexes(np.asarray([u]), kind)) == 0]
        raise ValueError("{} not seen by the model: {}".format("Entities" if kind == "e" else "Relations", unseen))
    return got


def _fitted_model(model):
    """the model behind a 1.x compat wrapper; it must be fitted"""
    model = getattr(model, "model", model) if getattr(model, "is_backward", False) else model
    if not model.is_fitted:
        raise ValueError("Model is not fitted.")
    return model


def _batch_top_n(top_n):
    top_n = int(top_n)
    if top_n < 1 or top_n > TOPN_BATCH_MAX:
        raise ValueError("`top_n` must be between 1 and {} (the device selection's limit); query_topn takes any top_n for a single "
                         "query. Got {}.".format(TOPN_BATCH_MAX, top_n))
    return top_n


def _known_statements(use_filter):
    """use_filter of the batched queries -> None (no filter) or a dict of datasets; a bare (m, 3) array stands for {"known": array}"""
    if use_filter is True:
        raise ValueError("`use_filter=True` has no meaning here (there is no evaluated set that could filter itself): pass a dict of "
                         "datasets or an (m, 3) array of known statements.")
    if use_filter is None or use_filter is False:
        return None
    if isinstance(use_filter, dict):
        return use_filter
    known = np.asarray(use_filter)
    if known.ndim != 2 or known.shape[1] < 3:
        raise ValueError("`use_filter` must be False, a dict of datasets or an (m, 3) array of known statements.")
    return {"known": known}


def _to_consider_ids(ix, values, name, kind):
    """ids (int64) of a checked `*_to_consider` list; None for None or an empty list: every entity / relation"""
    if values is None:
        return None
    _check_to_consider(ix, values, name, kind)
    return np.asarray(ix.get_indexes(np.asarray(values), kind), dtype=np.int64) if len(values) > 0 else None


def _empty_topn(top_n):
    return np.empty((0, top_n), dtype=object), np.empty((0, top_n), dtype=np.float32)


def _labels_or_none(ix, ids, have, kind):
    """(n, top_n) object array: the labels of ids where `have`, None where a row ran out of candidates"""
    labels = np.empty(ids.shape, dtype=object)
    labels[have] = ix.get_indexes(ids[have], kind, "ind2raw")
    return labels


def query_topn_batch(model, queries, top_n=10, corrupt_side="o", use_filter=False, ents_to_consider=None, exclude_reflexive=False):
    """The top_n best completions of MANY incomplete statements, without the ones already known to be true: what a trained
    link predictor is asked for most (recommendations for every head), and what query_topn -- one query per call, true
    statements on top of every list -- does not give.  (The reference has no counterpart.)

    queries: (n, 2) labels, the triple without its missing column in s, p, o order -- [subject, predicate] for
    corrupt_side="o", [predicate, object] for "s".  use_filter: False, or a dict of datasets as evaluate() takes (their
    union; a bare (m, 3) array stands for {"known": array}): a completion whose statement is in one of them is left out --
    exactly the ids evaluate() would subtract for a test triple with the same two fixed elements.  ents_to_consider: as in
    query_topn (None or empty: every entity).  exclude_reflexive: also leave out the query's own entity.

    Returns (entities (n, top_n) object array of labels, scores (n, top_n) float32), best first, equal scores by increasing
    position in the candidate list; where fewer than top_n candidates remain the tail holds None / -inf.  top_n <= 1024.
    Labels the model has not seen raise ValueError naming them.

    All queries are scored on the device in chunks (amdkge_corruption_scores) and each chunk goes straight into a per-row
    selection that skips the known ids (amdkge_topk_rows_excluding, kge_complete.hip): a known completion never enters the
    selection, so it cannot reappear as a filler, and -inf / NaN scores stay what they are.  Needs the whole entity table on
    one GPU: row- and column-sharded models raise NotImplementedError."""
    import torch

    from .placement import Columns, Rows

    model = _fitted_model(model)
    if corrupt_side not in ("s", "o"):
        raise ValueError("`corrupt_side` must be 's' or 'o', got {!r}.".format(corrupt_side))
    Q = np.asarray(queries)
    if Q.ndim != 2 or Q.shape[1] != 2:
        raise ValueError("`queries` must have shape (n, 2): [subject, predicate] for corrupt_side='o', [predicate, object] for 's'; "
                         "got {}.".format(Q.shape))
    top_n = _batch_top_n(top_n)
    use_filter = _known_statements(use_filter)
    ix = model.data_indexer
    cand_ids = _to_consider_ids(ix, ents_to_consider, "ents_to_consider", "e")
    ent_col, rel_col = (0, 1) if corrupt_side == "o" else (1, 0)
    fixed = _ids_or_fail(ix, Q[:, ent_col], "e")
    r_id = _ids_or_fail(ix, Q[:, rel_col], "r")
    pl = model._placement
    if isinstance(pl, (Rows, Columns)):
        raise NotImplementedError("query_topn_batch selects against the whole entity table on one GPU: row- and column-sharded tables "
                                  "(entity_sharding) are out of its scope; query_topn works there")
    n = int(Q.shape[0])
    if n == 0:
        return _empty_topn(top_n)
    eng = model._engine
    dev = eng.device
    side = _ffi.SIDE_O if corrupt_side == "o" else _ffi.SIDE_S
    q = torch.as_tensor(np.stack([fixed, r_id, fixed], 1).astype(np.int32)).to(dev)   # the replaced column is ignored by the scores and the filter
    flt = None
    if use_filter is not None:
        flt = model._filter_index(use_filter, None).device_filter(eng, q, corrupt_side)
    own = q[:, 0].contiguous() if exclude_reflexive else None
    ql = pl.localise(q)
    missing = []

    def pick(ids, hi, kk):
        pos, val = eng.corruption_topk(ql, side, kk, ent_ids=ids, ent_hi=hi, flt=flt, own=own)
        missing.append(pos < 0)
        return pos, val

    ents, val = pl.select(pick, cand_ids, n, top_n)
    return _labels_or_none(ix, ents, ~missing[0].cpu().numpy(), "e"), val.astype(np.float32)


def query_topn_relations(model, pairs, top_n=10, use_filter=False, rels_to_consider=None):
    """The top_n most plausible relations between MANY pairs of entities, without the ones already known to hold: the batched,
    filtered form of query_topn(head=..., tail=...).  (The reference has no counterpart.)

    pairs: (n, 2) labels [subject, object].  use_filter: False, or a dict of datasets as evaluate() takes (their union; a bare
    (m, 3) array stands for {"known": array}): a relation p with (s, p, o) in one of them is left out of the pair's list.
    rels_to_consider: as in query_topn (None or empty: every relation).

    Returns (relations (n, top_n) object array of labels, scores (n, top_n) float32), best first, equal scores by increasing
    position in the candidate list; where fewer than top_n candidates remain the tail holds None / -inf.  1 <= top_n <= 1024.
    Labels the model has not seen raise ValueError naming them.

    Every score has the bits predict() gives the materialised triple (amdkge_relation_scores: the pairs' rows stay in registers,
    a relation row is read once per group of queries); the selection is amdkge_topk_rows_excluding with the pair's known
    relations as the excluded ids.  Works on replicated, row- and column-sharded models (the relation table is whole on every
    rank; on a row-sharded model it is a collective: call it on every rank)."""
    import torch

    model = _fitted_model(model)
    Q = np.asarray(pairs)
    if Q.ndim != 2 or Q.shape[1] != 2:
        raise ValueError("`pairs` must have shape (n, 2): [subject, object]; got {}.".format(Q.shape))
    top_n = _batch_top_n(top_n)
    use_filter = _known_statements(use_filter)
    ix = model.data_indexer
    cand = _to_consider_ids(ix, rels_to_consider, "rels_to_consider", "r")
    s_id = _ids_or_fail(ix, Q[:, 0], "e")
    o_id = _ids_or_fail(ix, Q[:, 1], "e")
    n = int(Q.shape[0])
    if n == 0:
        return _empty_topn(top_n)
    dev = model._engine.device
    q = torch.as_tensor(np.stack([s_id, np.zeros_like(s_id), o_id], 1).astype(np.int32)).to(dev)   # the predicate column is ignored
    pfi = model._pair_filter_index(use_filter, None) if use_filter is not None else None
    pos, val = model._placement.select_relations(q, top_n, cand, pfi)
    rel = pos if cand is None else cand[np.maximum(pos, 0)]
    return _labels_or_none(ix, rel, pos >= 0, "r"), val.astype(np.float32)


def find_nearest_neighbours(kge_model, entities, n_neighbors=10, entities_subset=None, metric="euclidean"):
    """k nearest neighbours of `entities` in embedding space (:1171-1244; the reference delegates to
    sklearn.neighbors.NearestNeighbors on the host).  "euclidean" / "cosine": on the device -- dot products on the rank
    tile kernel (GEMM form), norms folded into a per-row top-k selection; works with a row-sharded table (partial lists per
    shard, merged).  Other sklearn metrics fall back to sklearn on the downloaded embeddings.  Returns (neighbour labels,
    distances), each (len(entities), n_neighbors), nearest first."""
    import torch

    assert kge_model.is_fitted, "KGE model is not fit!"
    assert isinstance(entities, (list, np.ndarray)), "Invalid type for entities! Must be a list or np.array"
    ix = kge_model.data_indexer
    if entities_subset is not None:
        assert isinstance(entities_subset, (list, np.ndarray)), "Invalid type for entities_subset! Must be a list or np.array"
        all_neighbors = np.asarray(entities_subset)
        cand = np.asarray(ix.get_indexes(all_neighbors, "e"), dtype=np.int64)
    else:
        cand = None
        all_neighbors = None
    n_all = kge_model._n_ents if cand is None else len(cand)
    assert n_neighbors < n_all, "n_neighbors must be less than the number of entities being fit!"
    eng, pl = kge_model._engine, kge_model._placement
    dev = eng.device
    qid = np.asarray(ix.get_indexes(np.asarray(entities), "e"), dtype=np.int64)
    k = int(n_neighbors)
    if metric not in ("euclidean", "l2", "minkowski", "cosine") or k > 1024:
        from sklearn.neighbors import NearestNeighbors

        labels = all_neighbors if cand is not None else ix.get_indexes(np.arange(kge_model._n_ents), "e", "ind2raw")
        E = kge_model.get_embeddings(labels)
        knn = NearestNeighbors(n_neighbors=n_neighbors, metric=metric).fit(E)
        dist, idx = knn.kneighbors(kge_model.get_embeddings(np.asarray(entities)))
        return np.asarray(labels)[idx], dist
    met = "cosine" if metric == "cosine" else "euclidean"
    fake = np.stack([qid, np.zeros_like(qid), qid], 1).astype(np.int32)
    ql = pl.localise(torch.as_tensor(fake).to(dev))          # query rows, fetched behind the shard where remote
    Q = eng.ent[ql[:, 0].to(torch.int64)]
    ids, dist = pl.select(lambda ids_, hi, kk: eng.nearest_rows(Q, kk, met, ent_ids=ids_, ent_hi=hi), cand, len(qid), k, largest=False)
    labels = ix.get_indexes(ids.reshape(-1), "e", "ind2raw").reshape(ids.shape)
    return labels, dist.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- find_duplicates / clusters
_MODES = ("t", "e", "r")
_EUCLIDEAN = ("l2", "euclidean", "minkowski")   # (sklearn's minkowski defaults to p = 2)
_ZERO_NORM = 10 * np.finfo(np.float32).eps      # sklearn's normalize() leaves rows below this norm as they are


def _fail(msg):
    logger.error(msg)
    raise ValueError(msg)


def _validate(X, model, mode, clustering_algorithm=None):
    """The reference's checks, messages and order (discovery.py:673-701, :888-912) -> (unwrapped model, X as an array)."""
    model = getattr(model, "model", model) if getattr(model, "is_backward", False) else model   # 1.x compat wrappers
    if not model.is_fitted:
        _fail("Model has not been fitted.")
    if clustering_algorithm is not None and not hasattr(clustering_algorithm, "fit_predict"):
        _fail("Clustering algorithm does not have the `fit_predict` method.")
    if mode not in _MODES:
        _fail("Argument `mode` must be one of the following: {}.".format(", ".join(_MODES)))
    X = np.asarray(X)
    if mode == "t" and (len(X.shape) != 2 or X.shape[1] != 3):
        _fail("For 't' mode the input X must be a matrix with three columns.")
    if mode in ("e", "r") and len(X.shape) != 1:
        _fail("For 'e' or 'r' mode the input X must be an array.")
    return model, X


def _device_embeddings(model, X, mode):
    """fp32 device matrix of the rows of X: entity / relation embeddings, or [s | p | o] per triple (mode "t").  Entity rows
    come from placement.entity_table() (a collective on a row-sharded table: every rank calls) + engine.unpack, as in
    get_embeddings.  Unseen labels raise ValueError naming them (the reference's get_indexes drops them silently, which
    shifts every later row onto the wrong label); non-finite embeddings raise ValueError, as sklearn does."""
    import torch

    ix, eng = model.data_indexer, model._engine
    cols = [(X[:, 0], "e"), (X[:, 1], "r"), (X[:, 2], "e")] if mode == "t" else [(X, mode)]
    ids = []
    for labels, kind in cols:
        got = np.asarray(ix.get_indexes(labels, kind), dtype=np.int64)
        if len(got) != len(labels):
            unseen = [u for u in dict.fromkeys(labels.tolist()) if len(ix.get_indexes(np.asarray([u]), kind)) == 0]
            raise ValueError("{} not seen by the model: {}".format("Entities" if kind == "e" else "Relations", unseen))
        ids.append(got)
    parts = []
    for (labels, kind), idx in zip(cols, ids):
        tab = model._placement.entity_table() if kind == "e" else eng.rel
        parts.append(eng.unpack(tab[torch.as_tensor(idx).to(tab.device)]))
    emb = parts[0] if len(parts) == 1 else torch.cat(parts, 1).contiguous()
    if not bool(torch.isfinite(emb).all()):
        raise ValueError("Input contains NaN, infinity or a value too large for dtype('float32').")
    return emb


def _labels(X, mode):
    return [tuple(r) for r in X.tolist()] if mode == "t" else X.tolist()


def duplicate_tolerance(near, labels, to_thr, expected_fraction_duplicates, max_d, verbose=False):
    """The reference's tolerance bisection (scipy.optimize.bisect on [0, max_d], xtol=1e-3, maxiter=50) over one number per
    row: near[i] = row i's nearest other row in threshold units (float64).  A row's neighbour set has a partner exactly when
    near[i] <= to_thr(tol), and every partner has one too, so the reference's len(set().union(*dups)) / n is the number of
    distinct labels owning such a row over n."""
    from scipy import optimize

    n = len(near)
    group = {}
    inv = np.fromiter((group.setdefault(lab, len(group)) for lab in labels), dtype=np.int64, count=n)
    per_label = np.full(len(group), np.inf)
    np.minimum.at(per_label, inv, np.asarray(near, dtype=np.float64))
    per_label.sort()
    info = {"Nfeval": 0}

    def f(tol):
        frac = np.searchsorted(per_label, to_thr(tol), side="right") / n
        if verbose:
            info["Nfeval"] += 1
            logger.info("Eval {}: tol: {}, duplicate fraction: {}".format(info["Nfeval"], tol, frac))
        return frac - expected_fraction_duplicates

    return optimize.bisect(f, 0.0, max_d, xtol=1e-3, maxiter=50)


def duplicate_sets(pairs, labels, n):
    """Sorted unordered pairs (i < j, int [m, 2]) -> the reference's result: for every row i with at least one partner,
    frozenset({label(i)} | {label(j) : j partner of i}) -- one element when a repeated label's copies are the only partners."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return set()
    a = np.concatenate([pairs[:, 0], pairs[:, 1]])
    b = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    cut = np.flatnonzero(np.diff(a)) + 1
    out = set()
    for rows, partners in zip(np.split(a, cut), np.split(b, cut)):
        out.add(frozenset([labels[rows[0]]] + [labels[j] for j in partners.tolist()]))
    return out


def _join_nearest_units(eng, E, cosine, zero):
    """Nearest other row of every row in threshold units (float64 numpy), the largest euclidean pair distance of the RAW rows
    E (the reference's distance_matrix(emb, emb).max(), whatever the metric).  cosine: units of d2 between unit rows
    (cosine distance = d2 / 2); rows in `zero` (numpy bool) have distance 1 (d2 = 2) to every other row, as in sklearn."""
    import torch

    d2, _, mx = eng.join_nearest(E)
    max_d = float(np.sqrt(np.float64(mx.item())))
    if not cosine:
        return d2.cpu().numpy().astype(np.float64), max_d
    n = int(E.shape[0])
    keep = np.flatnonzero(~zero)
    near = np.full(n, np.inf)
    if len(keep):
        U = _unit_rows(E[torch.as_tensor(keep).to(E.device)])
        near[keep] = eng.join_nearest(U)[0].cpu().numpy().astype(np.float64)
    if zero.any() and n > 1:
        near = np.minimum(near, 2.0)
    return near, max_d


def _unit_rows(E):
    import torch

    return (E / torch.linalg.vector_norm(E, dim=1, keepdim=True)).contiguous()


def _join_radius_pairs(eng, E, cosine, zero, thr):
    """Sorted unordered pairs within thr (threshold units) -> int64 numpy [m, 2]."""
    import torch

    if not cosine:
        return eng.join_radius(E, thr).cpu().numpy().astype(np.int64)
    n = int(E.shape[0])
    keep = np.flatnonzero(~zero)
    pairs = [np.zeros((0, 2), np.int64)]
    if len(keep) > 1:
        p = eng.join_radius(_unit_rows(E[torch.as_tensor(keep).to(E.device)]), thr).cpu().numpy().astype(np.int64)
        pairs.append(keep[p])
    if zero.any() and 2.0 <= thr:   # a zero row is at cosine distance 1 from every other row
        z = np.flatnonzero(zero)
        i, j = np.meshgrid(z, np.arange(n), indexing="ij")
        zp = np.stack([np.minimum(i, j).ravel(), np.maximum(i, j).ravel()], 1)
        pairs.append(zp[zp[:, 0] != zp[:, 1]])
    p = np.unique(np.concatenate(pairs), axis=0)
    return p


def find_duplicates(X, model, mode="e", metric="l2", tolerance="auto", expected_fraction_duplicates=0.1, verbose=False):
    """Duplicate entities / relations / triples by distance in embedding space (:714-982): returns (set of frozensets of
    labels, tolerance).  Two rows are duplicates when their distance under `metric` is <= tolerance; tolerance="auto"
    bisects (scipy.optimize.bisect on [0, largest euclidean pair distance], xtol=1e-3) for the tolerance at which the
    fraction of distinct labels with a duplicate reaches expected_fraction_duplicates.

    "l2" / "euclidean" / "minkowski" (p = 2) and "cosine" run on the device as an exact self-join of the embeddings
    (kge_join.hip): one pass gives every row's nearest other row and the bisection runs on the host over those n numbers;
    one more pass emits the pairs at the chosen tolerance.  Other sklearn metrics fall back to sklearn NearestNeighbors on
    the downloaded embeddings, as the reference does.  For every row with at least one partner the result holds
    frozenset({its label} | {its partners' labels}); a label repeated in X whose copies are its only partners gives a
    one-element set (the reference's code does the same, though its docstring says "at least two").  Differences from the
    reference: labels the model has not seen raise ValueError naming them (the reference drops them silently and then
    labels later rows wrongly); cosine rows of (near) zero norm are at distance 1 from every other row, as in sklearn."""
    import torch

    model, X = _validate(X, model, mode)
    E = _device_embeddings(model, X, mode)
    labels = _labels(X, mode)
    n = int(E.shape[0])
    eng = model._engine
    if metric not in _EUCLIDEAN and metric != "cosine":
        return _find_duplicates_sklearn(eng, E, X, mode, labels, metric, tolerance, expected_fraction_duplicates, verbose)
    cosine = metric == "cosine"
    to_thr = (lambda t: 2.0 * float(t)) if cosine else (lambda t: float(t) * float(t))
    zero = np.zeros(n, dtype=bool)
    if cosine:
        zero = (torch.linalg.vector_norm(E, dim=1) < _ZERO_NORM).cpu().numpy()
    if tolerance == "auto":
        near, max_d = _join_nearest_units(eng, E, cosine, zero)
        tolerance = duplicate_tolerance(near, labels, to_thr, expected_fraction_duplicates, max_d, verbose)
    pairs = _join_radius_pairs(eng, E, cosine, zero, to_thr(tolerance))
    return duplicate_sets(pairs, labels, n), tolerance


def _find_duplicates_sklearn(eng, E, X, mode, labels, metric, tolerance, expected_fraction_duplicates, verbose):
    """The reference's procedure for metrics the join does not cover (sklearn on the host); the "auto" upper bound (largest
    euclidean pair distance) still comes from the device join."""
    from scipy import optimize
    from sklearn.neighbors import NearestNeighbors

    emb = E.cpu().numpy()

    def get_dups(tol):
        neighbors = NearestNeighbors(metric=metric, radius=tol).fit(emb).radius_neighbors(emb)[1]
        return {frozenset(labels[j] for j in row) for row in neighbors if len(row) > 1}

    if tolerance == "auto":
        info = {"Nfeval": 0}

        def opt(tol):
            frac = len(set().union(*get_dups(tol))) / len(emb)
            if verbose:
                info["Nfeval"] += 1
                logger.info("Eval {}: tol: {}, duplicate fraction: {}".format(info["Nfeval"], tol, frac))
            return frac - expected_fraction_duplicates

        max_d = float(np.sqrt(np.float64(eng.join_nearest(E)[2].item())))
        tolerance = optimize.bisect(opt, 0.0, max_d, xtol=1e-3, maxiter=50)
    return get_dups(tolerance), tolerance


def _device_dbscan_params(algo):
    """(eps, min_samples, cosine) when `algo` is an sklearn.cluster.DBSCAN whose result the device join computes exactly, else
    None.  Covered: metric euclidean / l2 / minkowski with p in (None, 2) / cosine, no metric_params, and eps / min_samples that
    sklearn's own parameter check accepts (anything else goes to sklearn, whose error then surfaces).  algorithm, leaf_size and
    n_jobs choose how sklearn finds the neighbours, not which rows they are."""
    import numbers

    from sklearn.cluster import DBSCAN

    if type(algo) is not DBSCAN or algo.metric_params is not None:
        return None
    if not (isinstance(algo.metric, str) and (algo.metric in _EUCLIDEAN or algo.metric == "cosine")):
        return None
    if algo.metric == "minkowski" and algo.p not in (None, 2):
        return None
    if algo.metric == "cosine" and algo.algorithm not in ("auto", "brute"):   # (sklearn's trees refuse the metric)
        return None
    eps, ms = algo.eps, algo.min_samples
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not (0.0 < float(eps) < np.inf):
        return None
    if isinstance(ms, bool) or not isinstance(ms, numbers.Integral) or not (1 <= int(ms) <= 0x7FFFFFFF):
        return None
    return float(eps), int(ms), algo.metric == "cosine"


def dbscan_labels(core, parent, border):
    """sklearn.cluster.DBSCAN's labels_ from the three per-row results of the device passes (torch tensors on any one device;
    the restatement of join_rank_kernel / join_labels_kernel in kge_join.hip, which the tests hold the kernels to).  core: bool [n];
    parent: int [n], for a core row the lowest core row of its component; border: int [n], for a non-core row the lowest such root
    among the core rows within its radius, or INT32_MAX.  Clusters are numbered by their lowest core row; a border row takes the
    lowest-numbered cluster it touches; noise is -1.  -> int64 [n]."""
    import torch

    n = int(core.shape[0])
    idx = torch.arange(n, device=core.device)
    parent, border = parent.to(torch.int64), border.to(torch.int64)
    root = core & (parent == idx)
    rank = torch.cumsum(root.to(torch.int64), 0) - root.to(torch.int64)   # exclusive: the number of roots below each row
    target = torch.where(core, parent, border)
    noise = target == 0x7FFFFFFF
    return torch.where(noise, torch.full_like(target, -1), rank[torch.where(noise, torch.zeros_like(target), target)])


# ---------------------------------------------------------------------------------------------------- KMeans
_STANDALONE = {}


def _standalone_engine():
    """The engine a KMeans uses outside find_clusters: a minimal KgeEngine on the current GPU, one per device (raises without one)."""
    import torch

    from .engine import KgeEngine

    dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
    if dev not in _STANDALONE:
        _STANDALONE[dev] = KgeEngine("DistMult", 4, 4, 2)   # (the tables are not used)
    return _STANDALONE[dev]


def _run_rng(seed, run):
    """Run `run`'s generator: a function of (seed, run) alone, so a run does not depend on n_init."""
    return np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(run,)))


class KMeans:
    """Lloyd's k-means on the device, with sklearn.cluster.KMeans' interface: pass it to find_clusters in sklearn's place (the
    reference's documented use is KMeans(n_clusters=6, n_init=100, max_iter=500)), or call fit / fit_predict / predict on a numpy
    array or a device tensor anywhere -- a standalone call runs on the current GPU.  A sklearn.cluster.KMeans object given to
    find_clusters still runs on the host; KMeans.from_sklearn(km) copies its parameters into one of these.

    All n_init restarts advance in lock-step in the same kernel launches (engine.kmeans, kge_kmeans.hip): an assignment pass on the
    self-join's distance tile, per-block sums of the rows by label in row order and a fixed-order reduction -- no floating-point
    atomics, so equal inputs and seed give equal bits, whatever n_init.  Stop rules and `tol` (tol x the mean of the column
    variances, computed on the device) are sklearn's: no label changed, or the centres moved by no more than the tolerance, or
    max_iter.  cluster_centers_ (float32), labels_ (int32), inertia_, n_iter_ and n_features_in_ describe the restart of least
    inertia (ties: the lowest restart).

    init: "k-means++" (run r draws u = default_rng(SeedSequence(seed, spawn_key=(r,))).random(k); its first centre is row
    floor(u_0 n), centre j the first row whose fp64 cumulative squared distance to the chosen centres exceeds u_j x the total, or row
    floor(u_j n) when that total is 0), "random" (k distinct rows) or an array [k, d] (one run: n_init must be 1).

    Differences from sklearn: a cluster that loses all its rows keeps its centre (sklearn moves it to a far row); k-means++ is the
    plain D^2 sampling with one trial per step, not the greedy variant; Lloyd only (no elkan), no sample_weight.  With a different
    seeding the restarts differ from sklearn's; from equal initial centres, and where no row lies within fp32 rounding of a tie
    between two centres, labels and iteration counts are sklearn's."""

    def __init__(self, n_clusters=8, *, init="k-means++", n_init=10, max_iter=300, tol=1e-4, random_state=None):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state

    @classmethod
    def from_sklearn(cls, km):
        """A device KMeans with the six parameters of the sklearn.cluster.KMeans object km (algorithm="elkan", a callable init and
        a RandomState object are refused; n_init="auto" becomes sklearn's value for it: 1 for k-means++ or an array, 10 for random)."""
        if getattr(km, "algorithm", "lloyd") not in ("lloyd", "auto", "full"):
            raise ValueError("KMeans.from_sklearn: algorithm=%r is not supported (Lloyd only)" % (km.algorithm,))
        if callable(km.init):
            raise ValueError("KMeans.from_sklearn: a callable init is not supported")
        n_init = km.n_init
        if isinstance(n_init, str):
            if n_init != "auto":
                raise ValueError("KMeans.from_sklearn: n_init=%r" % (n_init,))
            n_init = 10 if isinstance(km.init, str) and km.init == "random" else 1
        return cls(km.n_clusters, init=km.init, n_init=n_init, max_iter=km.max_iter, tol=km.tol, random_state=km.random_state)

    # ------------------------------------------------------------------ parameters
    def _check_params(self):
        for name in ("n_clusters", "n_init", "max_iter"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("KMeans: %s must be a positive integer, got %r" % (name, v))
        if isinstance(self.tol, bool) or not isinstance(self.tol, (int, float, np.integer, np.floating)) or not self.tol >= 0:
            raise ValueError("KMeans: tol must be a non-negative number, got %r" % (self.tol,))
        if isinstance(self.init, str):
            if self.init not in ("k-means++", "random"):
                raise ValueError("KMeans: init must be 'k-means++', 'random' or an array [n_clusters, n_features], got %r" % (self.init,))
        elif callable(self.init) or self.init is None:
            raise ValueError("KMeans: init must be 'k-means++', 'random' or an array [n_clusters, n_features]")
        elif self.n_init != 1:
            raise ValueError("KMeans: an explicit init array is one run: n_init must be 1, got %r" % (self.n_init,))
        rs = self.random_state
        if rs is not None and (isinstance(rs, bool) or not isinstance(rs, (int, np.integer)) or rs < 0):
            raise ValueError("KMeans: random_state must be None or a non-negative integer, got %r" % (rs,))

    def _seed(self):
        return int(self.random_state) if self.random_state is not None else int(np.random.SeedSequence().entropy)

    @staticmethod
    def _matrix(X, eng):
        """X as an fp32 matrix on the engine's device (numpy arrays are uploaded, device tensors are used where they are)."""
        import torch

        t = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
        if t.dim() != 2:
            raise ValueError("KMeans: X must be a matrix [n_samples, n_features], got shape %s" % (tuple(t.shape),))
        if not (t.is_floating_point() or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
            raise ValueError("KMeans: X must be numeric, got %s" % (t.dtype,))
        if int(t.shape[0]) == 0 or int(t.shape[1]) == 0:
            raise ValueError("KMeans: X is empty (shape %s)" % (tuple(t.shape),))
        t = t.to(getattr(eng, "device", t.device), torch.float32).contiguous()
        if not bool(torch.isfinite(t).all()):
            raise ValueError("KMeans: X contains NaN or infinity")
        return t

    # ------------------------------------------------------------------ initial centres
    def _initial_centres(self, eng, X, seed):
        """centres0 [runs, k, d] on X's device."""
        import torch

        n, d = int(X.shape[0]), int(X.shape[1])
        k = int(self.n_clusters)
        if not isinstance(self.init, str):
            c = self.init if isinstance(self.init, torch.Tensor) else torch.as_tensor(np.asarray(self.init))
            if tuple(c.shape) != (k, d):
                raise ValueError("KMeans: init has shape %s, expected (%d, %d)" % (tuple(c.shape), k, d))
            c = c.to(X.device, torch.float32)
            if not bool(torch.isfinite(c).all()):
                raise ValueError("KMeans: init contains NaN or infinity")
            return c[None].contiguous()
        runs = int(self.n_init)
        if self.init == "random":
            rows = np.stack([_run_rng(seed, r).choice(n, size=k, replace=False) for r in range(runs)])
            return X[torch.as_tensor(rows, device=X.device)].contiguous()
        return _kmeans_plusplus(eng, X, k, runs, seed)

    # ------------------------------------------------------------------ sklearn's methods
    def fit(self, X, y=None, engine=None):
        """Fit on the rows of X (numpy array or device tensor).  engine: the KgeEngine to run on (find_clusters passes the model's)."""
        import torch

        self._check_params()
        eng = engine if engine is not None else _standalone_engine()
        Xd = self._matrix(X, eng)
        n, d = int(Xd.shape[0]), int(Xd.shape[1])
        if self.n_clusters > n:
            raise ValueError("KMeans: n_samples=%d should be >= n_clusters=%d" % (n, self.n_clusters))
        tol_abs = float(self.tol) * float(Xd.to(torch.float64).var(dim=0, unbiased=False).mean().item())
        centres0 = self._initial_centres(eng, Xd, self._seed())
        centres, labels, inertia, n_iter, _ = eng.kmeans(Xd, centres0, int(self.max_iter), tol_abs)
        best = int(np.argmin(inertia.cpu().numpy()))   # (ties: the lowest run)
        self.cluster_centers_ = centres[best].cpu().numpy().astype(np.float32)
        self.labels_ = labels[best].cpu().numpy().astype(np.int32)
        self.inertia_ = float(inertia[best].item())
        self.n_iter_ = int(n_iter[best].item())
        self.n_features_in_ = d
        self._engine = eng
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        """The nearest of cluster_centers_ for every row of X (int32 numpy; equal distances: the lowest centre)."""
        import torch

        if not hasattr(self, "cluster_centers_"):
            raise ValueError("KMeans: this instance is not fitted yet")
        eng = getattr(self, "_engine", None) or _standalone_engine()
        Xd = self._matrix(X, eng)
        if int(Xd.shape[1]) != self.n_features_in_:
            raise ValueError("KMeans: X has %d features, the fit had %d" % (int(Xd.shape[1]), self.n_features_in_))
        labels, _ = eng.kmeans_assign(Xd, torch.as_tensor(self.cluster_centers_))
        return labels.cpu().numpy().astype(np.int32)


def _kmeans_plusplus(eng, X, k, runs, seed):
    """k-means++ seeding of `runs` restarts at once -> centres [runs, k, d], every one a row of X.  Plain D^2 sampling, one trial per
    step; the distance pass is engine.kmeans_assign on the newest centre of every run, the draw a cumulative sum and a search."""
    import torch

    n = int(X.shape[0])
    u = np.stack([_run_rng(seed, r).random(k) for r in range(runs)])                      # [runs, k], host
    pick = lambda col: np.minimum((u[:, col] * n).astype(np.int64), n - 1)                 # noqa: E731   row floor(u n)
    rows = torch.as_tensor(pick(0), device=X.device)
    chosen = [rows]
    mind2 = None
    for j in range(1, k):
        _, m2 = eng.kmeans_assign(X, X[rows][:, None, :])
        mind2 = m2 if mind2 is None else torch.minimum(mind2, m2)
        cum = torch.cumsum(mind2.to(torch.float64), dim=1)
        total = cum[:, -1]
        target = torch.as_tensor(u[:, j], device=X.device) * total
        rows = torch.searchsorted(cum, target[:, None], right=True).reshape(-1).clamp_(max=n - 1)   # the first row with cum > target
        rows = torch.where(total > 0, rows, torch.as_tensor(pick(j), device=X.device))
        chosen.append(rows)
    return X[torch.stack(chosen, 1)].contiguous()


def find_clusters(X, model, clustering_algorithm=None, mode="e"):
    """Cluster labels of the embeddings of X (:546-711): entities, relations or [s | p | o] per triple.  Same validation and
    embedding assembly as find_duplicates.

    clustering_algorithm=None (sklearn.cluster.DBSCAN() with its defaults) or a DBSCAN instance with metric "euclidean" / "l2" /
    "minkowski" (p = 2) / "cosine" and no metric_params runs on the device (engine.dbscan, kge_join.hip): a neighbour count, a
    lock-free union-find over the core rows and a border pass on the exact self-join of find_duplicates, O(n) memory and no
    pair list; the thresholds are eps^2, or 2 eps between unit rows for cosine.  The labels are sklearn's, numbering included,
    and labels_, core_sample_indices_, components_ and n_features_in_ are set on the object as its fit_predict sets them.
    A KMeans of this module (the reference's documented use of find_clusters clusters with KMeans) is fitted on the device matrix,
    with no download: clustering_algorithm.fit(E, engine=model._engine); its labels_ come back as int64.  An empty X is a ValueError.
    Any other object -- sklearn.cluster.KMeans objects among them: they run on the host with sklearn's exact labels; see
    KMeans.from_sklearn --, other DBSCAN parameters, an empty X or a cosine call with a row of (near) zero norm go through
    clustering_algorithm.fit_predict on the downloaded embeddings, as in the reference."""
    import torch

    if clustering_algorithm is None:
        from sklearn.cluster import DBSCAN

        clustering_algorithm = DBSCAN()
    model, X = _validate(X, model, mode, clustering_algorithm)
    E = _device_embeddings(model, X, mode)
    if isinstance(clustering_algorithm, KMeans):
        if int(E.shape[0]) == 0:
            raise ValueError("find_clusters: X is empty")
        return clustering_algorithm.fit(E, engine=model._engine).labels_.astype(np.int64)
    params = _device_dbscan_params(clustering_algorithm)
    if params is not None and int(E.shape[0]) > 0:
        eps, min_samples, cosine = params
        if not cosine or not bool((torch.linalg.vector_norm(E, dim=1) < _ZERO_NORM).any()):
            labels, core, _ = model._engine.dbscan(_unit_rows(E) if cosine else E, 2.0 * eps if cosine else eps * eps, min_samples)
            algo = clustering_algorithm
            algo.core_sample_indices_ = torch.nonzero(core).reshape(-1).cpu().numpy()
            algo.components_ = E[core].cpu().numpy()
            algo.labels_ = labels.cpu().numpy().astype(np.int64)
            algo.n_features_in_ = int(E.shape[1])
            return algo.labels_
    return clustering_algorithm.fit_predict(E.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- discover_facts
_SAMPLED = ("random_uniform", "entity_frequency", "graph_degree", "cluster_coefficient", "cluster_triangles", "cluster_squares")


def _row_keys(A, B):
    """One int64 key per row of A and of B; two rows get the same key exactly when all their columns are equal."""
    both = [np.asarray(M).astype(str) if np.asarray(M).dtype == object else np.asarray(M) for M in (A, B)]
    M = np.concatenate(both, 0)
    key = np.zeros(M.shape[0], dtype=np.int64)
    for c in range(M.shape[1]):   # (re-numbered after every column: the keys stay below the row count)
        uniq, code = np.unique(M[:, c], return_inverse=True)
        key = np.unique(key * len(uniq) + code.reshape(-1), return_inverse=True)[1].reshape(-1).astype(np.int64)
    return key[:len(A)], key[len(A):]


def _setdiff2d(A, B):
    """Rows of A that are not in B, in A's order (:522-543) -- with the reference's quirk: only the FIRST copy of a row of A
    that occurs in B is removed, later copies of the same row survive.  The reference builds an |A| x |B| x columns comparison
    array for this; here a row key (np.unique per column) and "first occurrence in A" give the same rows in O((|A| + |B|) log)."""
    A, B = np.asarray(A), np.asarray(B)
    if len(A.shape) != 2 or len(B.shape) != 2:
        raise RuntimeError("Input arrays must be 2-dimensional.")
    if len(A) == 0 or len(B) == 0:
        return A[np.ones(len(A), dtype=bool)]
    ka, kb = _row_keys(A, B)
    first = np.zeros(len(A), dtype=bool)
    first[np.unique(ka, return_index=True)[1]] = True
    return A[~(first & np.isin(ka, kb))]


def generate_candidates(X, strategy, target_rel, max_candidates, consolidate_sides=False, seed=0):
    """Candidate statements (n, 3) for `target_rel` from the entities of X under a sampling strategy (:274-519): the grid of
    sqrt(max_candidates) + 10 sampled subjects x sampled objects, minus the rows of X and the reflexive rows, up to five
    rounds until max_candidates rows are collected.  "random_uniform" samples without replacement; "entity_frequency",
    "graph_degree", "cluster_coefficient", "cluster_triangles" and "cluster_squares" (networkx) sample WITH replacement,
    weighted by that statistic.  The draws are the reference's -- np.random.seed(seed), then np.random.choice for the subjects
    and the objects of each round -- so equal inputs and seed give its rows, row for row.  That includes what its
    _setdiff2d does: only the first copy of a row that occurs in X is removed, so the weighted strategies can return
    duplicate rows and, now and then, a row of X."""
    if X.shape[1] > 3:   # (weights beside the triples)
        X = X[:, :3]
    if strategy not in _SAMPLED:
        raise ValueError("%s is not a valid candidate generation strategy." % strategy)
    if not np.isin(target_rel, np.unique(X[:, 1])).all():   # (also for a list of relations, where the reference's `in` depends on numpy's broadcasting)
        logger.warning("Target relation is not found in triples.")   # (no error: the relation may be absent from X)
    if not isinstance(max_candidates, (float, int)):
        raise ValueError("Parameter max_candidates must be a float or int.")
    if max_candidates <= 0:
        raise ValueError("Parameter max_candidates must be a positive integer or float in range (0,1].")
    if isinstance(max_candidates, float):
        max_candidates = int(max_candidates * len(X))

    np.random.seed(seed)
    if consolidate_sides:
        e_s = e_o = np.unique(np.concatenate((X[:, 0], X[:, 2])))
    else:
        e_s, e_o = np.unique(X[:, 0]), np.unique(X[:, 2])
    logger.info("Generating candidates using {} strategy.".format(strategy))

    w_s = w_o = None
    if strategy == "entity_frequency":
        if consolidate_sides:
            n_s = n_o = np.unique(X[:, [0, 2]], return_counts=True)[1].astype(np.float64)
        else:
            n_s = np.unique(X[:, 0], return_counts=True)[1].astype(np.float64)
            n_o = np.unique(X[:, 2], return_counts=True)[1].astype(np.float64)
        w_s, w_o = n_s / np.sum(n_s), n_o / np.sum(n_o)
    elif strategy != "random_uniform":
        import networkx as nx

        G = nx.Graph()
        for s, p, o in X:
            G.add_nodes_from([s, o])
            G.add_edge(s, o, name=p)
        stat = {"graph_degree": lambda g: dict(g.degree()), "cluster_coefficient": nx.algorithms.cluster.clustering,
                "cluster_triangles": nx.algorithms.cluster.triangles, "cluster_squares": nx.algorithms.cluster.square_clustering}[strategy](G)
        w_s = np.array([stat[e] for e in e_s], dtype=np.float64)
        w_o = np.array([stat[e] for e in e_o], dtype=np.float64)
        w_s, w_o = w_s / np.sum(w_s), w_o / np.sum(w_o)

    sample_size = int(np.sqrt(max_candidates) + 10)   # (+ 10: the filter below shrinks the grid)
    out = np.zeros([max_candidates, 3], dtype=object)
    filled = 0
    for _ in range(5):
        if filled > max_candidates - 1:
            break
        if w_s is None:
            pick_s = np.random.choice(e_s, size=sample_size, replace=False)
            pick_o = np.random.choice(e_o, size=sample_size, replace=False)
        else:
            pick_s = np.random.choice(e_s, size=sample_size, replace=True, p=w_s)
            pick_o = np.random.choice(e_o, size=sample_size, replace=True, p=w_o)
        grid = np.array(np.meshgrid(pick_s, target_rel, pick_o)).T.reshape(-1, 3)   # [s, rel, o] rows, subjects fastest
        grid = _setdiff2d(grid, X)
        grid = grid[grid[:, 0] != grid[:, 2]]
        take = min(len(grid), max_candidates - filled)
        out[filled:filled + take] = grid[:take]
        filled += take
    return out[:filled]


def discover_facts(X, model, top_n=10, strategy="random_uniform", max_candidates=100, target_rel=None, seed=0):
    """New statements the model ranks highly (:21-271): candidates for `target_rel` (a label, a list of labels, or None for
    every relation of the model, one after the other) are ranked against their corruptions on both sides by
    model.evaluate(candidates, use_filter={"test": X}, corrupt_side="s,o"), and those whose mean rank is <= top_n are
    returned as (triples (n, 3) of labels, mean ranks (n,)).  A candidate is not in the filter, so it counts among its own
    corruptions: with the default "worst" ties every rank is at least 2.

    The sampled strategies draw the candidates with generate_candidates, as the reference does (a given list of target
    relations goes there in one call).  strategy="exhaustive" -- documented and then rejected by the reference -- takes
    every (s, r, o) with s != o that is not in X, for every target relation r and all entities of the model, and returns
    exactly those whose mean rank is <= top_n, ordered by relation, subject id, object id; max_candidates is ignored.  It
    runs on the device (two 1-vs-all score passes and a selection per relation, exact ranks of the survivors) and needs
    the whole entity table on one GPU: row- and column-sharded models raise NotImplementedError.

    Differences from the reference: (1) it returns np.hstack of the per-relation (n, 3) arrays, which is wrong or raises as
    soon as there are two relations; here the rows are stacked vertically into one (n, 3) array (the same result when the
    loop runs once).  (2) evaluate() drops candidates with labels the model has not seen, which shifts the ranks against
    the candidates; here such candidates are dropped before ranking, so rows and ranks stay aligned."""
    model = getattr(model, "model", model) if getattr(model, "is_backward", False) else model   # 1.x compat wrappers
    if not model.is_fitted:
        _fail("Model is not fitted.")
    if strategy not in _SAMPLED + ("exhaustive",):
        _fail("%s is not a valid strategy." % strategy)
    if strategy == "exhaustive":
        logger.info("Strategy is `exhaustive`, ignoring max_candidates.")
    X = np.asarray(X)
    if isinstance(max_candidates, float):
        logger.debug("Converting max_candidates float value {} to int value {}".format(max_candidates, int(max_candidates * len(X))))
        max_candidates = int(max_candidates * len(X))
    if isinstance(target_rel, str):
        target_rel = [target_rel]
    ix = model.data_indexer
    known = ix.get_indexes(np.arange(ix.get_relations_count()), "r", "ind2raw").tolist()
    if target_rel is None:
        logger.info("No target relation specified. Using all relations to generate candidate statements.")
        rel_list = known
    else:
        missing = [rel for rel in target_rel if rel not in known]
        if len(missing) > 0:
            _fail("Target relation(s) not found in model: {}".format(missing))
        rel_list = [target_rel]
    if strategy == "exhaustive":
        return _discover_exhaustive(X, model, top_n, known if target_rel is None else list(target_rel))
    np.random.seed(seed)
    found, found_ranks = [], []
    for relation in rel_list:
        logger.info("Generating candidates for relation: %s" % relation)
        candidates = generate_candidates(X, strategy, relation, max_candidates, seed=seed)
        logger.debug("Generated %d candidate statements." % len(candidates))
        if len(candidates):
            candidates = candidates[ix.valid_row_mask(candidates)]
        ranks = model.evaluate(candidates, use_filter={"test": X}, corrupt_side="s,o", verbose=False) if len(candidates) else np.zeros((0, 2))
        mean = np.mean(np.asarray(ranks).reshape(len(candidates), -1), axis=1)
        keep = mean <= top_n
        found.append(candidates[keep])
        found_ranks.append(mean[keep])
    logger.info("Discovered %d facts" % sum(len(f) for f in found))
    return np.vstack(found), np.concatenate(found_ranks)


def _discover_exhaustive(X, model, top_n, rel_labels, stats=None):
    """strategy="exhaustive" of discover_facts.  Per relation: R = max(1, floor(2 top_n) - 1) bounds each side's rank (the
    mean of two ranks >= 1 is <= top_n only if both are <= R); engine.corruption_select emits, for the queries (s, r, .) of
    every s and (., r, o) of every o, the columns that can rank <= R (a superset: kge_discover.hip); the two lists are
    intersected on s * N + o; placement.rank gives the survivors' exact ranks and the cut is applied to those, so the
    result is evaluate()'s by construction.  stats: a dict that receives per-relation counts and (synchronised) phase times."""
    import time

    import torch

    from .placement import Columns, Rows

    pl = model._placement
    if isinstance(pl, (Rows, Columns)):
        raise NotImplementedError("strategy='exhaustive' scores every (s, o) pair against the whole entity table on one GPU: "
                                  "row- and column-sharded tables (entity_sharding) are out of its scope; the sampled strategies work there")
    eng, ix = model._engine, model.data_indexer
    dev, N = eng.device, int(model._n_ents)
    R = max(1, int(np.floor(2 * top_n)) - 1)
    fi = model._filter_index({"test": X}, None)
    ents = torch.arange(N, dtype=torch.int32, device=dev)
    zero = torch.zeros_like(ents)
    triples, mean_ranks = [np.zeros((0, 3), dtype=np.int64)], [np.zeros(0, dtype=np.float64)]

    def tick():
        if stats is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    for r_id in np.asarray(ix.get_indexes(np.asarray(rel_labels), "r"), dtype=np.int64).tolist():
        rel = torch.full_like(ents, r_id)
        t0 = tick()
        margin_q = eng.select_margin(r_id)
        lists = {}
        for side, name, q in ((_ffi.SIDE_O, "o", torch.stack([ents, rel, zero], 1).contiguous()),
                              (_ffi.SIDE_S, "s", torch.stack([zero, rel, ents], 1).contiguous())):
            lists[name] = eng.corruption_select(q, side, R, margin_q, fi.device_filter(eng, q, name))[0].to(torch.int64)
        t1 = tick()
        k_o = lists["o"][:, 0] * N + lists["o"][:, 1]   # (query s, column o)
        k_s = lists["s"][:, 1] * N + lists["s"][:, 0]   # (query o, column s)
        keys = torch.sort(k_o[torch.isin(k_o, k_s)]).values
        t2 = tick()
        kept = 0
        if keys.numel():
            tri = torch.stack([keys // N, torch.full_like(keys, r_id), keys % N], 1).to(torch.int32).cpu().numpy()
            mean = pl.rank(tri, ["s", "o"], fi, None, "worst").cpu().numpy().astype(np.float64).mean(1)
            keep = mean <= top_n
            kept = int(keep.sum())
            triples.append(tri[keep].astype(np.int64))
            mean_ranks.append(mean[keep])
        t3 = tick()
        if stats is not None:
            stats.setdefault("relations", []).append({
                "relation": int(r_id), "R": R, "margin_q": int(margin_q), "emitted_o": int(k_o.numel()), "emitted_s": int(k_s.numel()),
                "survivors": int(keys.numel()), "found": kept, "t_score_select": t1 - t0, "t_intersect": t2 - t1, "t_exact_ranks": t3 - t2})
    logger.info("Discovered %d facts" % (sum(len(t) for t in triples)))
    return ix.get_indexes(np.concatenate(triples), "t", "ind2raw"), np.concatenate(mean_ranks)
