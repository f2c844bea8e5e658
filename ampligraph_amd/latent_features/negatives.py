"""Training negative samplers: compile(negatives=...).

Without the setting every corruption is drawn inside the train kernels: a fair coin for the side, a uniform entity id
(draw_corruption, kge_device.h).  `NegativeSampling` describes the three things that rule lacks -- rejection of KNOWN statements
(PyKEEN / LibKGE / DGL-KE's filtered negatives), the per-relation Bernoulli side choice of TransH, and a caller's pool of
replacement entities (AmpliGraph 1.x's negative_corruption_entities) -- and `bind()` turns it, once per fit(), into a
`BoundNegatives`: the object trainer.StepLoop calls each step for its override rows.  It runs amdkge_sample_negatives
(kge_negatives.hip; the draw is defined in include/amdkge_negatives.h) and hands the rows to the train step as its neg_override: the
train kernels and the loss are the ones of the default path.

`TypedNegatives` is a NegativeSampling whose replacements come from the positive's own relation's domain / range set
(datasets/types.py; amdkge_sample_negatives_typed, include/amdkge_types.h): it binds to a `BoundTypedNegatives`, the same step.

`SharedNegatives` is the other kind: one list of replacement entities per GROUP of positives, scored by a matrix product
(kge_train_shared.hip).  It binds to a `BoundSharedNegatives`, which owns the step's backward call -- trainer.StepLoop asks its step() to
draw and to run engine.train_shared_fwdbwd, instead of asking for override rows --; with
`mask_known` to a `BoundMaskedSharedNegatives`, whose step is engine.train_shared_masked_fwdbwd (include/amdkge_shared_mask.h: the
scores of corruptions that are known statements are -inf before the loss).  num_negs="all" makes every list every entity.

`SharedDistanceNegatives` is SharedNegatives for TransE and RotatE, whose score against a shared list is a tile of distances instead
of a matrix product (kge_train_shared_dist.hip, include/amdkge_shared_dist.h).  It binds to the same two classes, constructed with
distance=True: their step is engine.train_shared_dist_fwdbwd.

`KvsAll` is the shared step on the all-entities list with LABELS instead of a mask: every known answer of a row's query is labelled
1 and the loss is binary cross-entropy (loss_functions.BCELoss; include/amdkge_shared_labels.h).  It binds to a `BoundKvsAll`, whose
step is engine.train_shared_labels_fwdbwd, or engine.train_shared_dist_labels_fwdbwd for TransE / RotatE.
"""
import numpy as np

from .. import _ffi
from ..datasets.filters import FilterIndex
from ..trainer import SHARED_STEP, fit_modes, refuse_modes


# ---- the argument checks every setting shares (relation_prediction.py too); `who` is the message prefix, `name` the caller's argument
def check_side(side, who="negatives"):
    if not isinstance(side, str) or side not in _ffi.NEG_SIDE_MODES:
        raise ValueError("{}: `side` must be 'uniform', 'bernoulli', 's' or 'o', got {!r}".format(who, side))
    return side


def check_entities(entities, who="negatives"):
    """None or a non-empty 1-D sequence of labels -> None or their numpy array"""
    if entities is None:
        return None
    if isinstance(entities, (str, bytes)) or np.ndim(entities) != 1 or len(entities) < 1:
        raise ValueError("{}: `entities` must be None or a non-empty 1-D sequence of entity labels".format(who))
    return np.asarray(entities)


def check_datasets(value, name, who="negatives", allow_false=True):
    """False (where the caller has an off state) | True (the training set) | a non-empty dict of datasets next to it -> bool or the dict"""
    if isinstance(value, dict) and len(value) > 0:
        return value
    if isinstance(value, (bool, np.bool_)) and (allow_false or bool(value)):
        return bool(value)
    raise ValueError("{}: `{}` must be {}True (the training set) or a non-empty dict of datasets known next to it".format(
        who, name, "False, " if allow_false else ""))


# ---- what every bind() does with them, once per fit()
def known_index(model, engine, train, datasets, index_cls=FilterIndex):
    """The device index of class `index_cls` over the known statements: the training tensor and, when `datasets` is a dict, its
    datasets in the training id map (rows with labels the training set does not hold are dropped)."""
    extra = []
    if isinstance(datasets, dict):
        from .models import _load_triples

        extra = [model.data_indexer.get_indexes(_load_triples(v)[:, :3]) for v in datasets.values()]
    return index_cls([train] + extra, int(model._n_ents), int(model._n_rels), engine=engine)


def entity_pool(model, engine, labels):
    """None, or the int32 device ids of the entity labels replacements are drawn from (the train kernels do not check ids)"""
    if labels is None:
        return None
    import torch

    N = int(model._n_ents)
    ids = np.asarray(model.data_indexer.get_indexes(labels, "e"), dtype=np.int64)
    if ids.shape[0] != labels.shape[0]:
        raise ValueError("negatives: {} of the `entities` are not in the training set".format(labels.shape[0] - ids.shape[0]))
    if ids.min() < 0 or ids.max() >= N:
        raise ValueError("negatives: entity ids outside [0, {})".format(N))
    return torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32)).to(engine.device)


def batch_slice(train, batch, lo=0, hi=None):
    """slice(r0, r1): where rows [lo, hi) of `batch` (all of it by default) lie in an array over ALL training rows -- fit()'s batches
    are row slices of the tensor `train` a sampler was bound to, so a step slices what bind() looked up and runs no lookup of its own"""
    if batch.untyped_storage().data_ptr() != train.untyped_storage().data_ptr() or batch.dtype != train.dtype or not batch.is_contiguous():
        raise ValueError("negatives: the batch is not a row slice of the training tensor this sampler was bound to")
    off = batch.storage_offset() - train.storage_offset()
    if off < 0 or off % 3 or off // 3 + int(batch.shape[0]) > int(train.shape[0]):
        raise ValueError("negatives: the batch is not a row slice of the training tensor this sampler was bound to")
    r0 = off // 3 + int(lo)
    return slice(r0, r0 + (int(batch.shape[0]) if hi is None else int(hi)) - int(lo))


def _cut(ranges, rows):
    """a (lo, hi, ids) of all training rows -> that of the rows"""
    return ranges[0][rows], ranges[1][rows], ranges[2]


class NegativeSampling:
    """filter: False (no rejection) | True (a corruption that is a TRAINING triple is redrawn) | dict of datasets, in the form
    evaluate(use_filter=...) takes (their triples are known statements too, next to the training set; rows with labels the
    training set does not hold are dropped).
    side: "uniform" (a fair coin per corruption) | "bernoulli" (the subject with probability tph / (tph + hpt) of the
    positive's relation, Wang et al. 2014) | "s" | "o" (always that side).
    entities: None (every entity) or the labels of the entities replacements are drawn from.
    max_tries: draws per corruption before the last rejected one is kept (1 .. 32; 1 with a filter only counts)."""

    def __init__(self, filter=False, side="uniform", entities=None, max_tries=8):
        self.filter, self.side = check_datasets(filter, "filter"), check_side(side)
        if isinstance(max_tries, bool) or not isinstance(max_tries, (int, np.integer)) or not 1 <= int(max_tries) <= _ffi.NEG_MAX_TRIES:
            raise ValueError("negatives: `max_tries` must be an integer in [1, {}]".format(_ffi.NEG_MAX_TRIES))
        self.entities, self.max_tries = check_entities(entities), int(max_tries)

    @classmethod
    def get(cls, spec):
        """compile()'s `negatives` argument -> None or a sampler: None, a NegativeSampling or SharedNegatives (or anything with .bind()), a dict of
        NegativeSampling's keywords, {"shared": num_negs, ...} for a SharedNegatives or {"shared_distance": num_negs, ...} for a
        SharedDistanceNegatives."""
        if spec is None or hasattr(spec, "bind"):
            return spec
        if isinstance(spec, dict) and "shared" in spec:   # {"shared": M, ...}: SharedNegatives(num_negs=M, ...)
            return SharedNegatives.from_dict(spec)
        if isinstance(spec, dict) and "shared_distance" in spec:   # {"shared_distance": M, ...}: SharedDistanceNegatives(num_negs=M, ...)
            return SharedDistanceNegatives.from_dict(spec)
        if isinstance(spec, dict) and "kvsall" in spec:   # {"kvsall": "all", ...}: KvsAll
            return KvsAll.from_dict(spec)
        if isinstance(spec, dict) and "types" in spec:    # {"types": "observed" | RelationTypes, ...}: TypedNegatives
            return TypedNegatives.from_dict(spec)
        if isinstance(spec, dict):
            unknown = set(spec) - {"filter", "side", "entities", "max_tries"}
            if unknown:
                raise ValueError("negatives: unknown keys {}".format(sorted(unknown)))
            return cls(**spec)
        raise ValueError("negatives must be None, a dict or a NegativeSampling")

    def get_config(self):
        """The constructor arguments (datasets and labels as given)."""
        return {"filter": self.filter, "side": self.side, "entities": self.entities, "max_tries": self.max_tries}

    def bind(self, model, engine, train):
        """train: the int32 device tensor [n, 3] of id triples fit() slices its batches from -> BoundNegatives."""
        index, pool = self._bind_parts(model, engine, train)
        return BoundNegatives(engine, train, index, self.side, pool, self.max_tries, reject=self.filter is not False)

    def _bind_parts(self, model, engine, train):
        """(the FilterIndex over the known statements or None, the pool's int32 device ids or None)"""
        pool = entity_pool(model, engine, self.entities)
        index = known_index(model, engine, train, self.filter) if self.filter is not False or self.side == "bernoulli" else None
        return index, pool


class BoundNegatives:
    """A sampler bound to one fit(): the FilterIndex over the training set (and the filter datasets), the four range arrays of ALL
    training rows -- two range lookups at bind time; a batch is then a slice of them, no lookup kernel runs per step --, the
    Bernoulli thresholds, the pool tensor and the stats tensor.

    Called by trainer.StepLoop.step as negatives(global_batch, lo, hi, eta, seed, step) -> int32 device rows [(hi - lo) * eta, 3],
    the corruptions of rows [lo, hi) of the global batch, keyed by the GLOBAL row (row_offset = lo, b_global = the batch's size):
    every rank of a data-parallel run draws its own slice of the same rows."""

    N_STATS = 2

    def __init__(self, engine, train, index, side, pool, max_tries, reject):
        self.engine, self.train, self.index = engine, train, index
        self.side, self.pool, self.max_tries = side, pool, int(max_tries)
        import torch

        self.stats_dev = torch.zeros(self.N_STATS, dtype=torch.int64, device=engine.device)
        self.s_filter = self.o_filter = self.side_thr = None
        if index is not None and reject:
            self.s_filter = index.device_filter(engine, train, "s")
            self.o_filter = index.device_filter(engine, train, "o")
        if side == "bernoulli":
            self.side_thr = engine.negatives_side_thresholds(*index.device_keys(engine), index.n_ents, index.n_rels)

    def _first_row(self, batch):
        """the training row `batch` starts at: fit()'s batches are row slices of the tensor this sampler was bound to"""
        return batch_slice(self.train, batch).start

    def _step_args(self, global_batch, lo, hi):
        """(the batch rows, the keywords both samplers take, cut): cut slices a (lo, hi, ids) of all training rows to the batch's"""
        rows = batch_slice(self.train, global_batch, lo, hi)
        cut = lambda f: None if f is None else _cut(f, rows)   # noqa: E731
        kw = dict(row_offset=lo, b_global=int(global_batch.shape[0]), side=self.side, side_thr=self.side_thr, pool=self.pool,
                  s_filter=cut(self.s_filter), o_filter=cut(self.o_filter), max_tries=self.max_tries, stats=self.stats_dev)
        return global_batch[lo:hi], kw, cut

    def __call__(self, global_batch, lo, hi, eta, seed, step):
        rows, kw, _ = self._step_args(global_batch, lo, hi)
        return self.engine.sample_negatives(rows, eta, seed, step, **kw)

    def stats(self):
        """{"redraws", "exhausted"} since the bind: one device read (synchronises the stream)."""
        rd, ex = (int(v) for v in self.stats_dev.tolist())
        return {"redraws": rd, "exhausted": ex}


class TypedNegatives(NegativeSampling):
    """Type-constrained negatives: a corruption of (s, p, o) replaces s by a member of p's DOMAIN or o by a member of p's RANGE
    (PyKEEN's / LibKGE's type-constrained sampling, AmpliGraph 1.x's corruption_entities per relation, the local closed world of
    Krompass et al. 2015) -- (s, born_in, ?) gets a place, not a film.

    types: "observed" (the sets are the subjects / objects the training set shows with each relation) or a
    datasets.types.RelationTypes (observed in more datasets, or explicit sets per relation label).
    min_size: a relation whose set on the replaced side has fewer ids is corrupted by the untyped rule instead (every entity, or
    `entities`); 2 by default, because a set of one entity can only reproduce the positive.
    filter, side, entities, max_tries: NegativeSampling's -- rejection of known statements works inside the set as it does outside.

    compile(negatives=TypedNegatives(...)) or compile(negatives={"types": ..., "filter": ..., "side": ..., "entities": ..., "max_tries": ...,
    "min_size": ...}).  After fit(): model.relation_types_ (the bound sets, what evaluate_typed() takes by default) and
    model.negative_sampling_stats_ with a third count, "untyped"."""

    def __init__(self, types, filter=False, side="uniform", entities=None, max_tries=8, min_size=2):
        from ..datasets.types import RelationTypes

        super().__init__(filter, side, entities, max_tries)
        if isinstance(types, str) and types == "observed":
            types = RelationTypes.observed()
        if not isinstance(types, RelationTypes):
            raise ValueError("negatives: `types` must be 'observed' or a RelationTypes, got {!r}".format(types))
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or int(min_size) < 1:
            raise ValueError("negatives: `min_size` must be an integer >= 1")
        self.types, self.min_size = types, int(min_size)

    @classmethod
    def from_dict(cls, spec):
        unknown = set(spec) - {"types", "filter", "side", "entities", "max_tries", "min_size"}
        if unknown:
            raise ValueError("negatives: unknown keys {} for typed negatives".format(sorted(unknown)))
        return cls(**spec)

    def get_config(self):
        return dict(super().get_config(), types=self.types, min_size=self.min_size)

    def bind(self, model, engine, train):
        """-> BoundTypedNegatives: BoundNegatives' work plus the candidate ranges of ALL training rows, once"""
        index, pool = self._bind_parts(model, engine, train)
        return BoundTypedNegatives(engine, train, index, self.side, pool, self.max_tries, reject=self.filter is not False,
                                   relation_types=self.types.bind(model, engine, train), min_size=self.min_size)


class BoundTypedNegatives(BoundNegatives):
    """BoundNegatives with the two candidate ranges of every training row (two lookups at bind time; a step slices them) and a
    third counter.  relation_types: the BoundRelationTypes, which fit() publishes as model.relation_types_."""

    N_STATS = 3

    def __init__(self, engine, train, index, side, pool, max_tries, reject, relation_types, min_size):
        super().__init__(engine, train, index, side, pool, max_tries, reject)
        self.relation_types, self.min_size = relation_types, int(min_size)
        self.s_cand = relation_types.ranges(train, "s", self.min_size, "none")
        self.o_cand = relation_types.ranges(train, "o", self.min_size, "none")

    def __call__(self, global_batch, lo, hi, eta, seed, step):
        rows, kw, cut = self._step_args(global_batch, lo, hi)
        return self.engine.sample_negatives_typed(rows, eta, seed, step, s_cand=cut(self.s_cand), o_cand=cut(self.o_cand), **kw)

    def stats(self):
        """{"redraws", "exhausted", "untyped"} since the bind: one device read (synchronises the stream)."""
        rd, ex, ut = (int(v) for v in self.stats_dev.tolist())
        return {"redraws": rd, "exhausted": ex, "untyped": ut}


class SharedNegatives:
    """Shared-negative training (PyTorch-BigGraph's batch negatives, DGL-KE's chunked sampling): the positives of a batch are cut
    into groups of `group_size` consecutive rows, every group shares ONE list of `num_negs` replacement entities, every positive
    has one replaced side.  The step is the default one on those corruptions (same losses, `num_negs` takes the place of eta), but
    the scores of a group are one matrix product on the matrix cores and a positive costs three row reads whatever `num_negs` is
    (include/amdkge_shared.h, kge_train_shared.hip).  DistMult, ComplEx and HolE only.

    num_negs: corruptions per positive, 1 .. 2^24 - 1, or "all": every group's list is EVERY entity in id order (or the `entities`
    pool in the order given), only the sides are drawn -- 1-vs-all training; with multiclass_nll and mask_known the filtered softmax
    cross-entropy.  group_size: the positives per group; None = num_negs, or ALL_GROUP_SIZE = 4 096 with "all" (the result then does
    not depend on it: it only sets how the matrix products are cut, and the score buffer's 4 * group_size * N bytes -- lower it for a
    large entity table).
    side: "uniform" | "bernoulli" | "s" | "o", decided per POSITIVE.  entities: None or the labels replacements are drawn from.
    mask_known: False | True (the training set) | a non-empty dict of datasets in the form NegativeSampling(filter=...) takes
    (known next to the training set).  The score of a corruption that is a known statement -- the positive itself among them --
    is set to -inf before the loss (PyTorch-BigGraph's masking): it adds no loss term and gets no gradient, the reduction
    divisors stay; a positive whose WHOLE list is known keeps its row (include/amdkge_shared_mask.h).  After fit():
    model.negative_sampling_stats_ = {"masked", "unmaskable"}.
    There is no `filter`: a rejection per positive would give every positive its own list.

    compile(negatives=SharedNegatives(...)) or compile(negatives={"shared": num_negs | "all", "group_size": ..., "side": ...,
    "entities": ..., "mask_known": ...})."""

    shared = True   # what trainer.StepLoop.step looks for
    KEY = "shared"  # the key of the dict form that carries num_negs
    DISTANCE = False   # the bound sampler's entry points: matrix products (kge_train_shared.hip) or distance tiles (kge_train_shared_dist.hip)
    ALL_GROUP_SIZE = 4096   # measured: the products want >= 4 096 rows per chunk; the score buffer is 4 * group_size * num_negs bytes

    def __init__(self, num_negs, group_size=None, side="uniform", entities=None, mask_known=False):
        def count(v, name, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
                raise ValueError("negatives: `{}` must be an integer in [1, {}]".format(name, hi))
            return int(v)

        if isinstance(num_negs, str):
            if num_negs != "all":
                raise ValueError("negatives: `num_negs` must be an integer in [1, {}] or 'all', got {!r}".format(_ffi.SHARED_MAX_NEGS, num_negs))
            self.num_negs = "all"
        else:
            self.num_negs = count(num_negs, "num_negs", _ffi.SHARED_MAX_NEGS)
        default_g = self.ALL_GROUP_SIZE if self.num_negs == "all" else self.num_negs
        self.group_size = default_g if group_size is None else count(group_size, "group_size", 2 ** 31 - 1)
        self.side, self.entities, self.mask_known = check_side(side), check_entities(entities), check_datasets(mask_known, "mask_known")

    @classmethod
    def from_dict(cls, spec):
        if "filter" in spec and spec["filter"] is not False:
            raise ValueError("negatives: shared negatives take no `filter`: a rejection per positive breaks the sharing")
        unknown = set(spec) - {cls.KEY, "group_size", "side", "entities", "filter", "mask_known"}
        if unknown:
            raise ValueError("negatives: unknown keys {} for shared negatives".format(sorted(unknown)))
        return cls(spec[cls.KEY], spec.get("group_size"), spec.get("side", "uniform"), spec.get("entities"), spec.get("mask_known", False))

    def get_config(self):
        """The dict form compile(negatives=...) takes (labels and datasets as given; `mask_known` only when it is set)."""
        cfg = {self.KEY: self.num_negs, "group_size": self.group_size, "side": self.side, "entities": self.entities}
        if self.mask_known is not False:
            cfg["mask_known"] = self.mask_known
        return cfg

    @property
    def names_rows(self):
        """what optimizer_mode="sparse" asks (trainer.refuse_sparse): are the lists finite -- not every entity?"""
        return self.num_negs != "all" or self.entities is not None

    def check_model(self, model, optimizer_mode="dense"):
        """compile()'s refusals: everything that is known before a GPU is touched."""
        if model.scoring_type not in ("DistMult", "ComplEx", "HolE"):
            raise NotImplementedError("negatives: shared negatives need a score that is a contraction with the replaced row "
                                      "(DistMult, ComplEx, HolE); {} scores a distance: its shared step is "
                                      "SharedDistanceNegatives".format(model.scoring_type))
        check_shared_modes(model, optimizer_mode)

    def bind(self, model, engine, train):
        import torch

        refuse_modes(*SHARED_STEP, **fit_modes(model))
        pool = entity_pool(model, engine, self.entities)
        index, side_thr = None, None
        if self.mask_known is not False or self.side == "bernoulli":
            index = known_index(model, engine, train, self.mask_known)
        if self.side == "bernoulli":   # (thresholds over the index's statements: the training set, and the mask's datasets when given)
            side_thr = engine.negatives_side_thresholds(*index.device_keys(engine), index.n_ents, index.n_rels)
        num_negs, all_list = self.num_negs, None
        if num_negs == "all":   # the list every group shares: every entity in id order, or the pool in the order given
            all_list = pool if pool is not None else torch.arange(int(model._n_ents), dtype=torch.int32, device=engine.device)
            num_negs = int(all_list.numel())
            if num_negs > _ffi.SHARED_MAX_NEGS:
                raise ValueError("negatives: 'all' needs at most {} entities".format(_ffi.SHARED_MAX_NEGS))
        if self.mask_known is False:
            return BoundSharedNegatives(engine, num_negs, self.group_size, self.side, side_thr, pool, all_list=all_list, distance=self.DISTANCE)
        return BoundMaskedSharedNegatives(engine, num_negs, self.group_size, self.side, side_thr, pool, all_list=all_list, train=train, index=index,
                                          identity=all_list is not None and pool is None, distance=self.DISTANCE)


def check_shared_modes(model, optimizer_mode):
    """compile()'s mode refusals of every sampler that owns its step (entity_sharding is refused for every sampler, in compile() itself)"""
    refuse_modes(*SHARED_STEP, deterministic=model._deterministic, lazy=optimizer_mode == "lazy")


class SharedDistanceNegatives(SharedNegatives):
    """SharedNegatives for the DISTANCE models, TransE and RotatE: the same groups, lists, sides, losses, `mask_known` and
    num_negs="all", the same constructor arguments.  A distance against a shared list is no matrix product, so the step runs on
    distance tiles instead (include/amdkge_shared_dist.h, kge_train_shared_dist.hip): a group's query vectors and its gathered rows
    are read once and the group_size x num_negs x k work is arithmetic on operands in LDS and registers.  RotatE with the subject
    replaced is scored as |e - o o conj(r)|, which differs from the reference's |e o r - o| by fp32 rounding only (|r| = 1).
    DistMult, ComplEx and HolE are refused: theirs is SharedNegatives.

    compile(negatives=SharedDistanceNegatives(...)) or compile(negatives={"shared_distance": num_negs | "all", "group_size": ...,
    "side": ..., "entities": ..., "mask_known": ...})."""

    KEY = "shared_distance"
    DISTANCE = True

    def check_model(self, model, optimizer_mode="dense"):
        if model.scoring_type not in ("TransE", "RotatE"):
            raise NotImplementedError("negatives: SharedDistanceNegatives is the shared step of the models that score a distance (TransE, RotatE); "
                                      "{} scores a contraction: use SharedNegatives".format(model.scoring_type))
        check_shared_modes(model, optimizer_mode)


class BoundSharedNegatives:
    """A SharedNegatives bound to one fit().  It owns the step's backward call: trainer.StepLoop.step calls step(global_batch, loss,
    seed, rng_step), which draws -- draw(global_batch, seed, step) -> (ids int32 [n_groups, num_negs], side int32 [B]) -- and hands
    both to engine.train_shared_fwdbwd, or with distance=True (SharedDistanceNegatives) to engine.train_shared_dist_fwdbwd.
    all_list: None, or the int32 device list [num_negs] of num_negs="all": every group's row of ids is that list -- the id tensor
    is built once (and again only for a batch with more groups than any before), a step draws the sides alone.
    candidate_rows(global_batch) -> (rows, n_rows): the entity rows the step just run on that batch can have touched
    (engine.step_rows on the batch and the ids draw() kept; one copy of an all_list), what optimizer_mode="sparse" sweeps.
    names_rows: False where the list is every entity (all_list without a pool) -- every row is a candidate then and
    candidate_rows refuses."""

    shared = True   # what trainer.StepLoop.step looks for: the sampler runs the backward call itself

    def __init__(self, engine, num_negs, group_size, side, side_thr, pool, all_list=None, distance=False):
        self.engine, self.num_negs, self.group_size = engine, int(num_negs), int(group_size)
        self.side, self.side_thr, self.pool = side, side_thr, pool
        self.distance, self.all_list, self._all_ids = bool(distance), all_list, None
        self.names_rows, self._step_ids = all_list is None or pool is not None, None

    def candidate_rows(self, global_batch):
        if not self.names_rows:
            raise NotImplementedError("negatives: the list is every entity: every row is a candidate")
        return self.engine.step_rows(global_batch, self._step_ids if int(global_batch.shape[0]) > 0 else None)

    def step(self, global_batch, loss, seed, rng_step):
        """loss: the step's amdkge_loss descriptor"""
        ids, side = self.draw(global_batch, seed, rng_step)
        fwdbwd = self.engine.train_shared_dist_fwdbwd if self.distance else self.engine.train_shared_fwdbwd
        fwdbwd(global_batch, self.group_size, self.num_negs, ids, side, loss)

    def draw(self, global_batch, seed, step):
        if self.all_list is None:
            ids, side = self.engine.sample_shared(global_batch, self.group_size, self.num_negs, seed, step, side=self.side,
                                                  side_thr=self.side_thr, pool=self.pool)
            self._step_ids = ids   # (kept for candidate_rows: the engine's buffer, valid until the next draw)
            return ids, side
        B = int(global_batch.shape[0])
        n_groups = -(-B // min(self.group_size, B)) if B > 0 else 0
        if self._all_ids is None or int(self._all_ids.shape[0]) < n_groups:
            self._all_ids = self.all_list.reshape(1, -1).repeat(n_groups, 1).contiguous()
        # the side of a positive does not depend on the list's length (include/amdkge_shared.h, THE DRAW): one id per group is drawn and dropped
        _, side = self.engine.sample_shared(global_batch, self.group_size, 1, seed, step, side=self.side, side_thr=self.side_thr)
        self._step_ids = self.all_list   # (every group's row is this list: one copy names its rows)
        return self._all_ids[:n_groups], side


class BoundMaskedSharedNegatives(BoundSharedNegatives):
    """BoundSharedNegatives with the mask of known statements: the FilterIndex over the training set (and mask_known's datasets) and
    the range arrays of ALL training rows -- two range lookups at bind time, as in BoundNegatives; mask(global_batch) slices them.
    step() hands them to engine.train_shared_masked_fwdbwd (distance=True: train_shared_dist_fwdbwd) with `identity` (the list is
    0 .. N - 1) and `stats_dev`."""

    def __init__(self, engine, num_negs, group_size, side, side_thr, pool, all_list, train, index, identity, distance=False):
        import torch

        super().__init__(engine, num_negs, group_size, side, side_thr, pool, all_list=all_list, distance=distance)
        self.train, self.index, self.identity = train, index, bool(identity)
        self.stats_dev = torch.zeros(2, dtype=torch.int64, device=engine.device)
        self.s_filter = index.device_filter(engine, train, "s")
        self.o_filter = index.device_filter(engine, train, "o")

    def mask(self, global_batch):
        """-> (s_filter, o_filter) of the batch's rows: (lo, hi, ids) each"""
        rows = batch_slice(self.train, global_batch)
        return _cut(self.s_filter, rows), _cut(self.o_filter, rows)

    def step(self, global_batch, loss, seed, rng_step):
        ids, side = self.draw(global_batch, seed, rng_step)
        s_filter, o_filter = self.mask(global_batch)
        fwdbwd = self.engine.train_shared_dist_fwdbwd if self.distance else self.engine.train_shared_masked_fwdbwd
        fwdbwd(global_batch, self.group_size, self.num_negs, ids, side, loss, s_filter=s_filter, o_filter=o_filter, identity=self.identity,
               stats=self.stats_dev)

    def stats(self):
        """{"masked", "unmaskable"} since the bind -- the corruption scores set to -inf and the positives whose whole list was known
        (left unmasked): one device read (synchronises the stream)."""
        mk, un = (int(v) for v in self.stats_dev.tolist())
        return {"masked": mk, "unmaskable": un}


class KvsAll:
    """KvsAll training (ConvE, LibKGE): a training row is a QUERY (s, p, ?) or (?, p, o) -- the side is drawn per row, as in
    SharedNegatives --, EVERY entity is a binary classification, and all KNOWN answers of the query are labelled 1 instead of being
    masked away.  The loss is loss_functions.BCELoss (binary cross-entropy with logits, optional label smoothing), and only that one;
    the softmax over the same list is SharedNegatives("all", mask_known=True) + multiclass_nll.  The step is the shared step on the
    all-entities list in id order (include/amdkge_shared_labels.h: labels and loss are one pass over a chunk's scores), for all five
    models: matrix products for DistMult / ComplEx / HolE, distance tiles for TransE / RotatE.

    side: "uniform" | "bernoulli" | "s" | "o", decided per row.
    weight: "triple" (every training triple is a row of weight 1) | "query" (a row weighs 1 / the number of training rows that share
    its query -- (s, p) when the object is asked for, (p, o) when the subject is: with a fixed side an epoch's loss is then exactly
    the loss over the UNIQUE queries, LibKGE's KvsAll objective, without touching the batch loop).
    known: True (the training set) | a non-empty dict of datasets known next to it, in SharedNegatives(mask_known=...)'s form.
    group_size: the rows per group; None = SharedNegatives.ALL_GROUP_SIZE.  The result does not depend on it.
    There is no `entities`: the list is every entity.  After fit(): model.negative_sampling_stats_ = {"labelled", "unlabelled_rows"}.

    compile(negatives=KvsAll(...), loss=BCELoss({...})) or compile(negatives={"kvsall": "all", "side": ..., "weight": ..., "known": ...,
    "group_size": ...}, ...)."""

    shared = True   # what trainer.StepLoop.step looks for
    kvsall = True   # what compile() looks for
    names_rows = False   # the list is every entity: optimizer_mode="sparse" has nothing to leave out
    KEY = "kvsall"

    def __init__(self, side="uniform", weight="triple", known=True, group_size=None):
        if not isinstance(weight, str) or weight not in ("triple", "query"):
            raise ValueError("negatives: `weight` must be 'triple' or 'query', got {!r}".format(weight))
        if group_size is not None and (isinstance(group_size, bool) or not isinstance(group_size, (int, np.integer)) or not 1 <= int(group_size) <= 2 ** 31 - 1):
            raise ValueError("negatives: `group_size` must be None or an integer in [1, {}]".format(2 ** 31 - 1))
        self.side, self.weight, self.known = check_side(side), weight, check_datasets(known, "known", allow_false=False)
        self.group_size = SharedNegatives.ALL_GROUP_SIZE if group_size is None else int(group_size)

    @classmethod
    def from_dict(cls, spec):
        if spec[cls.KEY] != "all":
            raise ValueError("negatives: {{'kvsall': 'all'}} is the one list KvsAll has, got {!r}".format(spec[cls.KEY]))
        unknown = set(spec) - {cls.KEY, "side", "weight", "known", "group_size"}
        if unknown:
            raise ValueError("negatives: unknown keys {} for KvsAll (there is no `entities`: the list is every entity)".format(sorted(unknown)))
        return cls(spec.get("side", "uniform"), spec.get("weight", "triple"), spec.get("known", True), spec.get("group_size"))

    def get_config(self):
        """The dict form compile(negatives=...) takes (datasets as given)."""
        return {self.KEY: "all", "side": self.side, "weight": self.weight, "known": self.known, "group_size": self.group_size}

    def check_model(self, model, optimizer_mode="dense"):
        """compile()'s refusals: everything that is known before a GPU is touched (all five models take part)."""
        check_shared_modes(model, optimizer_mode)

    @staticmethod
    def query_weights(train):
        """train: int [n, 3] id triples -> (w_s, w_o) float32 [n]: 1 / the number of rows sharing the row's (p, o) / (s, p)."""
        t = np.asarray(train, dtype=np.int64).reshape(-1, 3)
        out = []
        for a, b in ((1, 2), (0, 1)):
            _, inv, cnt = np.unique(t[:, [a, b]], axis=0, return_inverse=True, return_counts=True)
            out.append((1.0 / cnt[inv.reshape(-1)]).astype(np.float32))
        return out[0], out[1]

    def bind(self, model, engine, train):
        import torch

        refuse_modes(*SHARED_STEP, **fit_modes(model))
        N = int(model._n_ents)
        if N > _ffi.SHARED_MAX_NEGS:
            raise ValueError("negatives: KvsAll needs at most {} entities".format(_ffi.SHARED_MAX_NEGS))
        index = known_index(model, engine, train, self.known)
        side_thr = None
        if self.side == "bernoulli":
            side_thr = engine.negatives_side_thresholds(*index.device_keys(engine), index.n_ents, index.n_rels)
        weights = None
        if self.weight == "query":   # both arrays once, in numpy
            weights = tuple(torch.as_tensor(w).to(engine.device) for w in self.query_weights(train.cpu().numpy()))
        all_list = torch.arange(N, dtype=torch.int32, device=engine.device)
        return BoundKvsAll(engine, N, self.group_size, self.side, side_thr, None, all_list=all_list, train=train, index=index, identity=True,
                           weights=weights, distance=model.scoring_type in ("TransE", "RotatE"))


class BoundKvsAll(BoundMaskedSharedNegatives):
    """A KvsAll bound to one fit(): BoundMaskedSharedNegatives' index and range arrays (mask(global_batch) slices them: here they
    are the LABELS), the all-entities list, and the row weights of weight="query" (weights(global_batch) slices them).
    step() hands them to engine.train_shared_labels_fwdbwd, or with distance=True (TransE, RotatE) to train_shared_dist_labels_fwdbwd."""

    labelled = True   # what trainer.StepLoop.step pairs with loss_functions.BCELoss

    def __init__(self, engine, num_negs, group_size, side, side_thr, pool, all_list, train, index, identity, weights=None, distance=False):
        super().__init__(engine, num_negs, group_size, side, side_thr, pool, all_list, train, index, identity, distance=distance)
        self.row_weights = weights

    def weights(self, global_batch):
        """-> None or (w_s, w_o) of the batch's rows"""
        if self.row_weights is None:
            return None
        rows = batch_slice(self.train, global_batch)
        return tuple(w[rows] for w in self.row_weights)

    def step(self, global_batch, loss, seed, rng_step):
        """loss: the BCELoss object -- the labelled entry points take its two hyper-parameters as arguments"""
        ids, side = self.draw(global_batch, seed, rng_step)
        s_filter, o_filter = self.mask(global_batch)
        lp = loss._loss_parameters
        fwdbwd = self.engine.train_shared_dist_labels_fwdbwd if self.distance else self.engine.train_shared_labels_fwdbwd
        fwdbwd(global_batch, self.group_size, self.num_negs, ids, side, s_filter, o_filter, label_smoothing=lp["label_smoothing"],
               reduction=lp["reduction"], weights=self.weights(global_batch), identity=self.identity, stats=self.stats_dev)

    def stats(self):
        """{"labelled", "unlabelled_rows"} since the bind -- the entries labelled 1 and the rows without one: one device read
        (synchronises the stream)."""
        lb, un = (int(v) for v in self.stats_dev.tolist())
        return {"labelled": lb, "unlabelled_rows": un}
