"""Per-relation DOMAIN and RANGE sets: which entities may stand as a relation's subject / object.

`RelationTypes` describes them -- observed in datasets (the local closed world of Krompass et al. 2015: a relation's domain is the
subjects seen with it, its range the objects) or given explicitly per relation label -- and `bind()` turns them into a
`BoundRelationTypes`: two CSRs on the engine's device in the filter index's layout (ascending relation keys, start offsets, one id
array with ascending duplicate-free ids per set; include/amdkge_types.h).  The typed negative sampler
(latent_features/negatives.TypedNegatives) and evaluate_typed() take a triple's candidates as a [lo, hi) range into that id array:
nothing per triple is ever built on the host."""
import numpy as np


def sets_csr(triples, side, n_rels=None):
    """The host restatement of the device build (numpy): (keys int64, start int64, ids int32) of the distinct subjects (side "s")
    or objects ("o") per relation of the id triples."""
    X = np.asarray(triples).reshape(-1, 3).astype(np.int64)
    pv = np.unique(np.stack([X[:, 1], X[:, 0 if side == "s" else 2]], 1), axis=0) if X.shape[0] else np.zeros((0, 2), np.int64)
    keys, first = np.unique(pv[:, 0], return_index=True)
    return keys.astype(np.int64), np.append(first, pv.shape[0]).astype(np.int64), pv[:, 1].astype(np.int32)


class RelationTypes:
    """RelationTypes({rel_label: (domain_labels | None, range_labels | None)}): explicit sets; None, or a relation that is not
    listed, means unconstrained on that side.  RelationTypes.observed(datasets=None): the sets are what the datasets show."""

    def __init__(self, sets):
        if not isinstance(sets, dict):
            raise ValueError("types: explicit relation types are a dict {relation label: (domain labels | None, range labels | None)}")
        self.sets, self.datasets, self.is_observed = {}, None, False
        for rel, pair in sets.items():
            if isinstance(pair, (str, bytes)) or not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError("types: relation {!r} needs a pair (domain labels | None, range labels | None)".format(rel))
            both = []
            for what, labels in zip(("domain", "range"), pair):
                if labels is not None:
                    if isinstance(labels, (str, bytes)) or np.ndim(labels) != 1 or len(labels) < 1:
                        raise ValueError("types: the {} of relation {!r} must be None or a non-empty 1-D sequence of entity labels".format(what, rel))
                    labels = np.asarray(labels)
                both.append(labels)
            self.sets[rel] = tuple(both)

    @classmethod
    def observed(cls, datasets=None):
        """datasets: None (the training set: valid for training only), one array of triples, or a dict / sequence of them in the
        form evaluate(use_filter=...) takes.  With fit()'s training tensor at hand (TypedNegatives) the training set always counts."""
        self = cls({})
        self.is_observed = True
        if datasets is not None:
            if isinstance(datasets, dict):
                datasets = list(datasets.values())
            elif isinstance(datasets, np.ndarray) or isinstance(datasets, str):
                datasets = [datasets]
            datasets = list(datasets)
            if not datasets:
                raise ValueError("types: observed() needs None or at least one dataset")
        self.datasets = datasets
        return self

    def get_config(self):
        return {"observed": self.is_observed, "datasets": self.datasets, "sets": self.sets}

    def bind(self, model, engine, train=None):
        """-> BoundRelationTypes on engine's device, in the id map of `model`.  train: fit()'s int32 device tensor of id triples
        (observed sets: it counts next to the datasets) or None."""
        import torch

        N, R = int(model._n_ents), int(model._n_rels)
        if self.is_observed:
            from ..latent_features.models import _load_triples

            parts = [] if train is None else [train[:, :3].to(device=engine.device, dtype=torch.int32)]
            for d in self.datasets or []:
                ids = np.ascontiguousarray(model.data_indexer.get_indexes(_load_triples(d)[:, :3]), dtype=np.int32)
                parts.append(torch.as_tensor(ids).to(engine.device))
            if not parts:
                raise ValueError("types: RelationTypes.observed() without datasets only has the training set to observe: it is valid "
                                 "in compile(negatives=...); give evaluate_typed() observed(datasets)")
            X = torch.cat(parts, 0).contiguous()
            csr = {sd: engine.relation_sets_build(X, sd, N, R) for sd in ("s", "o")}
        else:
            csr = {sd: tuple(torch.as_tensor(a).to(engine.device) for a in self._explicit_csr(model, col)) for col, sd in enumerate(("s", "o"))}
        return BoundRelationTypes(engine, N, R, csr)

    def _explicit_csr(self, model, col):
        """host CSR (keys, start, ids) of side col (0: domains, 1: ranges): sorted unique ids per listed relation"""
        ix = model.data_indexer
        rows = []
        for rel, pair in self.sets.items():
            r = np.asarray(ix.get_indexes(np.asarray([rel]), "r"))
            if r.shape[0] != 1:
                raise ValueError("types: relation {!r} is unknown to the model".format(rel))
            if pair[col] is None:
                continue
            ids = np.asarray(ix.get_indexes(pair[col], "e"), dtype=np.int64)
            if ids.shape[0] != pair[col].shape[0]:
                raise ValueError("types: {} of the {} labels of relation {!r} are unknown to the model".format(
                    pair[col].shape[0] - ids.shape[0], "domain" if col == 0 else "range", rel))
            rows.append((int(r[0]), np.unique(ids)))
        rows.sort(key=lambda t: t[0])
        if len({r for r, _ in rows}) != len(rows):
            raise ValueError("types: two labels of the explicit sets name the same relation")
        keys = np.array([r for r, _ in rows], dtype=np.int64)
        start = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(v) for _, v in rows], out=start[1:])
        ids = np.concatenate([v for _, v in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
        return keys, start, ids


class BoundRelationTypes:
    """The two relation-set CSRs on a device.  The id array of each side carries the ids 0 .. N-1 appended ONCE behind the sets:
    the range a lookup falls back to with fallback="all" (evaluation: an unconstrained relation is ranked against every entity).
    largest_set: {side: the longest set}, read back once here; max_len: the longest range a lookup can return (the appended block)."""

    def __init__(self, engine, n_ents, n_rels, csr):
        import torch

        self.engine, self.n_ents, self.n_rels = engine, int(n_ents), int(n_rels)
        self._csr, self._n_ids, sizes = {}, {}, []
        everyone = torch.arange(self.n_ents, dtype=torch.int32, device=engine.device)
        for sd in ("s", "o"):
            keys, start, ids = csr[sd]
            self._n_ids[sd] = int(ids.shape[0])
            self._csr[sd] = (keys, start, torch.cat([ids.to(torch.int32), everyone]))
            sizes.append((start[1:] - start[:-1]).max() if int(keys.shape[0]) else torch.zeros((), dtype=torch.int64, device=engine.device))
        ls, lo = (int(v) for v in torch.stack(sizes).tolist())   # the one read-back
        self.largest_set = {"s": ls, "o": lo}
        self.max_len = self.n_ents

    def ranges(self, triples_dev, side, min_size=1, fallback="all"):
        """(lo, hi, ids) device tensors: the candidates of each int32 device triple on `side` ("s": its relation's domain, "o": its
        range).  A relation without a set of at least min_size ids gets fallback "all" (the appended 0 .. N-1) or "none" (the empty
        range (0, 0): the typed sampler's "draw by the untyped rule")."""
        if fallback not in ("all", "none"):
            raise ValueError("types: fallback must be 'all' or 'none'")
        sd = "s" if side == "s" else "o"
        keys, start, ids = self._csr[sd]
        n0 = self._n_ids[sd]
        lo, hi = self.engine.relation_sets_ranges(keys, start, triples_dev, min_size, (n0, n0 + self.n_ents) if fallback == "all" else (0, 0))
        return lo, hi, ids

    def host_sets(self):
        """{"s": {relation id: ascending int32 ids of its domain}, "o": {... of its range}} (tests, inspection)"""
        out = {}
        for sd, (keys, start, ids) in self._csr.items():
            k, st, i = keys.cpu().numpy(), start.cpu().numpy(), ids.cpu().numpy()
            out[sd] = {int(r): i[st[g]:st[g + 1]].copy() for g, r in enumerate(k)}
        return out
