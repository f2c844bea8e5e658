"""True-positive filter sets for evaluate(use_filter=...), as sort-based CSR instead of the
reference's pandas groupby + Python `sum(lists, [])` per batch
(/root/reference/ampligraph/datasets/graph_data_loader.py:287-350,382-439).

Semantics kept: for a test triple (s,p,o) the subject-side filter is the SET {s' : (s',p,o) in any
filter dataset} and the object-side filter the SET {o' : (s,p,o') in any filter dataset}; all ids are
the training id map's.  The index is built once per evaluate() call; a test triple's filter is a
[lo, hi) range into one shared id array, so no per-batch host work remains."""
import numpy as np

from .. import _ffi

# The three key forms of the CSR index -- the same definition as filter_group_key (kge_filter.hip): the GROUP a triple belongs
# to and the triple column listed under it.  The packed sort key is group * divisor + value, the divisor being the value's range.
#   "s": group (p, o), values s      "o": group (s, p), values o      "pair": group (s, o), values p
_VALUE_COLUMN = {"s": 0, "o": 2, "pair": 1}


def _group_key(form, s, p, o, N, R):
    return s * N + o if form == "pair" else p * N + o if form == "s" else s * R + p


class _CsrIndex:
    """What FilterIndex and PairFilterIndex share: one CSR per key form of _FORMS = {form: (keys, start, ids attribute names)},
    built on the host (engine=None) or on the device, the device copies in self._dev with host views on demand."""

    _FORMS = {}
    _OVERFLOW_HINT = ""

    def __init__(self, datasets, n_ents, n_rels, engine=None):
        self.n_ents, self.n_rels = int(n_ents), int(n_rels)
        N, R = self.n_ents, self.n_rels
        if R * N * N >= 2 ** 63:   # (python ints: no wrap) the packed int64 sort keys would overflow silently
            raise ValueError(f"{type(self).__name__}: n_rels * n_ents^2 = {R * N * N} does not fit the packed int64 keys"
                             + self._OVERFLOW_HINT)
        if engine is not None:
            self._init_device(datasets, engine)
            return
        X = np.concatenate([np.asarray(d)[:, :3].astype(np.int64) for d in datasets], 0) if len(datasets) else \
            np.zeros((0, 3), dtype=np.int64)
        for form, (keys, start, ids) in self._FORMS.items():
            div = R if form == "pair" else N
            k = np.unique(_group_key(form, X[:, 0], X[:, 1], X[:, 2], N, R) * div + X[:, _VALUE_COLUMN[form]])   # unique values per group
            g, first = np.unique(k // div, return_index=True)
            setattr(self, keys, g)
            setattr(self, start, np.append(first, k.size).astype(np.int64))
            setattr(self, ids, (k % div).astype(np.int32))

    def _init_device(self, datasets, engine):
        import torch

        dev = engine.device
        parts = []
        for d in datasets:
            if isinstance(d, torch.Tensor):
                parts.append(d[:, :3].to(device=dev, dtype=torch.int32))
            else:
                parts.append(torch.as_tensor(np.ascontiguousarray(np.asarray(d)[:, :3], dtype=np.int32)).to(dev))
        X = torch.cat(parts, 0).contiguous() if parts else torch.zeros(0, 3, dtype=torch.int32, device=dev)
        self._dev, self._dev_sizes = {"device": str(dev)}, {}
        for form, names in self._FORMS.items():
            built = engine.pair_filter_build(X, self.n_ents, self.n_rels) if form == "pair" else \
                engine.filter_build(X, form, self.n_ents, self.n_rels)
            self._store(names, *built)

    def _store(self, names, keys, start, ids):
        """one form's device tensors into the device cache; an empty id array is kept as a one-element placeholder (the kernels
        refuse a NULL id pointer), its true length in _dev_sizes"""
        import torch

        n = int(ids.numel())
        self._dev.update({names[0]: keys, names[1]: start, names[2]: ids if n else torch.zeros(1, dtype=torch.int32, device=ids.device)})
        self._dev_sizes[names[2]] = n

    def __getattr__(self, name):
        # host views of a device-built index, on demand (tests, bench's host-side range lookups)
        d = self.__dict__
        if "_dev" in d and any(name in names for names in self._FORMS.values()):
            t = d["_dev"][name]
            if name in d["_dev_sizes"]:
                t = t[:d["_dev_sizes"][name]]
            a = d[name] = t.cpu().numpy()
            return a
        raise AttributeError(name)

    @staticmethod
    def _ranges(keys, start, q):
        if keys.size == 0:
            z = np.zeros(q.shape[0], dtype=np.int64)
            return z, z.copy()
        pos = np.searchsorted(keys, q)
        pos_c = np.minimum(pos, keys.size - 1)
        hit = keys[pos_c] == q
        lo = np.where(hit, start[pos_c], 0).astype(np.int64)
        hi = np.where(hit, start[pos_c + 1], 0).astype(np.int64)
        return lo, hi

    def _host_ranges(self, triples, form):
        t = np.asarray(triples)[:, :3].astype(np.int64)
        keys, start, _ = self._FORMS[form]
        return self._ranges(getattr(self, keys), getattr(self, start), _group_key(form, t[:, 0], t[:, 1], t[:, 2], self.n_ents, self.n_rels))

    def _device_filter(self, engine, triples_dev, form):
        import torch

        device = engine.device
        if self.__dict__.get("_dev", {}).get("device") != str(device):
            # another device than the one the index lives on (or a host-built index): the host copies first -- for a
            # device-built index they exist only through __getattr__, which reads the very cache replaced here
            host = {f: [getattr(self, nm) for nm in names] for f, names in self._FORMS.items()}
            self._dev, self._dev_sizes = {"device": str(device)}, {}
            for f, names in self._FORMS.items():
                self._store(names, *(torch.as_tensor(a).to(device) for a in host[f]))
        keys, start, ids = (self._dev[nm] for nm in self._FORMS[form])
        if form == "pair":
            lo, hi = engine.pair_filter_ranges(keys, start, triples_dev, self.n_ents)
        else:
            lo, hi = engine.filter_ranges(keys, start, triples_dev, _ffi.SIDE_S if form == "s" else _ffi.SIDE_O, self.n_ents, self.n_rels)
        return lo, hi, ids


class FilterIndex(_CsrIndex):
    """engine=None: the index is built on the host (numpy sorts; the checker of the device build and what GPU-less callers
    get).  With a KgeEngine the id triples are uploaded once and the index is built ON THE DEVICE by amdkge_filter_build
    (kge_filter.hip: key generation, radix sort, scan, scatter) -- evaluate() then does no host sort at all; the host arrays
    (po_keys, ...) are downloaded lazily only if somebody asks for them."""

    _FORMS = {"s": ("po_keys", "po_start", "s_ids"), "o": ("sp_keys", "sp_start", "o_ids")}
    _OVERFLOW_HINT = " (n_ents up to ~96 M at 1 000 relations)"

    def subject_ranges(self, triples):
        return self._host_ranges(triples, "s")

    def object_ranges(self, triples):
        return self._host_ranges(triples, "o")

    def device_filter(self, engine, triples_dev, side):
        """(lo, hi, ids) device tensors for amdkge_rank_filter: the range lookup of subject_ranges / object_ranges done on
        the engine's device by amdkge_filter_ranges (keys, starts and ids are uploaded once per index and kept), so an
        evaluate() call does no per-triple host work.  triples_dev: (n,3) int32 device tensor; side "s" | "o"."""
        return self._device_filter(engine, triples_dev, "s" if side == "s" else "o")

    def device_keys(self, engine):
        """(po_keys, sp_keys) int64 device tensors of an index built on `engine`'s device: what the Bernoulli thresholds of the
        training negative sampler count (amdkge_negatives_side_thresholds)."""
        if self.__dict__.get("_dev", {}).get("device") != str(engine.device):
            raise ValueError("FilterIndex.device_keys: the index was not built on this engine's device")
        return self._dev["po_keys"], self._dev["sp_keys"]

    def as_lists(self, triples):
        """Materialise per-triple id arrays (what the reference yields as a RaggedTensor); tests only."""
        slo, shi = self.subject_ranges(triples)
        olo, ohi = self.object_ranges(triples)
        return ([self.s_ids[a:b] for a, b in zip(slo, shi)], [self.o_ids[a:b] for a, b in zip(olo, ohi)])


class PairFilterIndex(_CsrIndex):
    """The known relations of every (s, o) pair, for relation prediction (evaluate_relations(use_filter=...),
    discovery.query_topn_relations): for a query (s, ?, o) the filter is the SET {p : (s, p, o) in any filter dataset}, as a CSR
    over the sorted pair keys s * n_ents + o with the relation ids ascending inside a group -- FilterIndex's layout with a third
    key form.  engine=None builds it on the host (numpy; the checker of the device build and what GPU-less callers get); with a
    KgeEngine the id triples are uploaded once and amdkge_pair_filter_build builds it on the device (kge_filter.hip), the host
    arrays (so_keys, so_start, r_ids) being downloaded only if somebody asks for them."""

    _FORMS = {"pair": ("so_keys", "so_start", "r_ids")}

    def relation_ranges(self, triples):
        """(lo, hi) int64: the range of each triple's (s, o) pair in r_ids ((0, 0) for a pair no dataset holds)."""
        return self._host_ranges(triples, "pair")

    def device_filter(self, engine, triples_dev):
        """(lo, hi, ids) device tensors for relation_rank / relation_topk: relation_ranges done on the engine's device by
        amdkge_pair_filter_ranges (keys, starts and ids are uploaded once per index and kept).  triples_dev: (n,3) int32 device
        tensor of GLOBAL entity ids."""
        return self._device_filter(engine, triples_dev, "pair")
