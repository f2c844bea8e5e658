"""ScoringBasedEmbeddingModel: the reference's public model class
(/root/reference/ampligraph/latent_features/models/ScoringBasedEmbeddingModel.py:47) re-hosted on the
MI355X engine.  Same constructor / compile / fit / predict / evaluate / get_embeddings surface,
argument meaning and error behaviour; the Keras/TF machinery underneath is replaced by libamdkge
(HIP kernels, C ABI) driven from plain Python.  No TensorFlow, no CPU fallback.

Intentional, documented differences: negatives come from a counter-based Philox stream
keyed by (seed, step, row) instead of TF's stateful stream; tables are always HBM-resident, so
`partitioning_k > 1` is rejected; FocusE's structural weight really decays per epoch (in the reference the
tf.function captures the first epoch's value at trace time).
"""
import json
import os

import numpy as np

from .. import _ffi
from ..datasets.filters import FilterIndex, PairFilterIndex
from ..datasets.indexer import DataIndexer
from ..evaluation.metrics import hits_at_n_score, mr_score, mrr_score
from ..trainer import BATCH_REG, StepLoop, fit_modes, refuse_modes, refuse_sparse
from . import loss_functions, optimizers, regularizers
from .initializers import RowSource, initialise, stream_cost

SCORING_LAYER_REGISTRY = dict(_ffi.SCORING_TYPES)  # AbstractScoringLayer.py:15 (Random is out of scope)


class History:
    """Keras-History look-alike returned by fit(): `.history[name]` lists, `.epoch` list."""

    def __init__(self):
        self.history = {}
        self.epoch = []

    def _log(self, epoch, logs):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(v)


def _load_triples(x):
    """Accept what the reference's GraphDataLoader accepts for in-memory data
    (datasets/graph_data_loader.py:129-181): ndarray, list, DataFrame, or a csv/tsv file name."""
    if isinstance(x, str):
        import pandas as pd

        x = pd.read_csv(x, sep="\t", header=None, dtype=str).values
    elif hasattr(x, "values") and not isinstance(x, np.ndarray):
        x = x.values
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] < 3:
        raise ValueError("triples must have shape (n, 3) (or (n, >3) with numeric edge values)")
    return x


class ScoringBasedEmbeddingModel:
    def __init__(self, eta, k, scoring_type="DistMult", seed=0, max_ent_size=None, max_rel_size=None):
        if scoring_type not in SCORING_LAYER_REGISTRY:
            raise KeyError(scoring_type)  # the reference indexes SCORING_LAYER_REGISTRY directly (:146)
        self.eta = int(eta)
        self.k = int(k)
        self.scoring_type = scoring_type
        self.seed = int(seed)
        self.max_ent_size = max_ent_size
        self.max_rel_size = max_rel_size
        self.internal_k = 2 * self.k if scoring_type in ("ComplEx", "HolE", "RotatE") else self.k
        self.data_indexer = None
        self.is_fitted = False
        self.is_calibrated = False
        self.is_compiled = False
        self.use_focusE = False
        self.history = None
        self.stop_training = False
        self._placement = None       # ampligraph_amd/placement.py: where the tables live across the ranks
        self._loop = None
        self._sharding = "replicated"
        self._sharded_negatives = "local"
        self._deterministic = False
        self._negatives = None       # compile(negatives=...): latent_features/negatives.py
        self._relation_prediction = None   # compile(relation_prediction=...): latent_features/relation_prediction.py
        self._dist_override = None   # tests: an object with the torch.distributed collective surface

    @property
    def _engine(self):
        """The engine predict / evaluate / checkpoints read (row-sharded: this rank's rows and the scratch rows behind them)."""
        return None if self._placement is None else self._placement.engine

    # ------------------------------------------------------------------------------------ config (:56-98)
    @classmethod
    def from_config(cls, config):
        config = dict(config)
        regs = config.pop("entity_relation_regularizer", None)
        negs = config.pop("negatives", None)
        relp = config.pop("relation_prediction", None)
        model = cls(**config)
        if relp is not None:   # the relation-prediction term in its dict form: carried until compile() (restore_model compiles with it)
            from .relation_prediction import RelationPrediction

            model._relation_prediction = RelationPrediction.get(relp)
        if regs is not None:   # carried until compile() sets its own
            model._regularizers = [regularizers.from_config(r) for r in regs]
        if negs is not None:   # a KvsAll sampler, or the sampler of optimizer_mode="sparse", in its dict form: carried the same way
            from .negatives import NegativeSampling

            model._negatives = NegativeSampling.get(negs)
        return model

    def get_config(self):
        """The constructor arguments, like the reference's Keras config (:84-98) -- and, for a model whose [entity, relation]
        regularisers include a batch regulariser (regularizers.BatchLPRegularizer), the pair in its JSON form: the step it
        trains with differs in kind, not in a number; for a model compiled with a KvsAll sampler, the sampler's dict form under
        "negatives" (its loss, BCELoss, compiles with nothing else), and so for a model compiled with optimizer_mode="sparse" (the mode
        compiles with nothing else); for a model compiled with relation_prediction=..., the term's dict
        form under "relation_prediction".  Every other model's config is the constructor arguments alone."""
        cfg = {"eta": self.eta, "k": self.k, "scoring_type": self.scoring_type, "seed": self.seed,
               "max_ent_size": self.max_ent_size, "max_rel_size": self.max_rel_size}
        regs = getattr(self, "_regularizers", None)
        if regs and any(regularizers.is_batch(r) for r in regs):
            cfg["entity_relation_regularizer"] = [regularizers.to_config(r) for r in regs]
        # KvsAll: its loss (BCELoss) cannot be compiled without it; optimizer_mode="sparse": neither can the mode without its sampler
        if getattr(self._negatives, "kvsall", False) or (getattr(getattr(self, "optimizer", None), "sparse", False)
                                                         and self._negatives is not None):
            cfg["negatives"] = self._negatives.get_config()
        if self._relation_prediction is not None:   # the relation-prediction term: the step it trains with has one call more
            cfg["relation_prediction"] = self._relation_prediction.get_config()
        return cfg

    def get_invalid_keys(self, X, data_type="raw", **kwargs):
        """:2279-2306 -- subjects / predicates / objects of X that the model's id maps do not know."""
        return self.data_indexer.get_invalid_keys(X, data_type, **kwargs)

    def save(self, filepath, **kwargs):
        """Keras' model.save(filepath) in the reference (SavedModel directory + metadata, :1002-1044): here the same directory
        form written by ampligraph_amd.utils.save_model (flat .npz / .json)."""
        from ..utils.model_utils import save_model

        save_model(self, filepath)

    # ------------------------------------------------------------------------------------ compile
    def compile(self, optimizer="adam", loss=None, entity_relation_initializer="glorot_uniform",
                entity_relation_regularizer=None, **kwargs):
        """:1145-1152.  optimizer: name | OptimizerWrapper; loss: name | Loss; initializer: one value or
        [entity_init, relation_init]; regularizer: None | 'LP'/'l1'/'l2'/'l3' | LPRegularizer | pair.  A member may also be a
        BatchLPRegularizer ('N3', 'batch_LP': latent_features/regularizers.py), which penalises the rows of each step's positives
        once per occurrence instead of the whole table -- the regulariser that goes with SharedNegatives("all", mask_known=True) +
        multiclass_nll.  One GPU, replicated tables; no deterministic, lazy or FocusE mode.  With the train kernels' own
        per-corruption negatives it takes the dense-gradient step (train_fwdbwd -> batch_reg_fwdbwd -> opt_step) instead of the
        owner-computes one, which never materialises an entity gradient: measured once at ComplEx k = 200, B = 10 000, eta = 20,
        0.41 instead of 0.15 ms per step; on a shared-negative step it adds 0.06 ms.

        Extra keywords of this engine: optimizer_mode="dense" (default, the reference's semantics) | "lazy" (touched rows
        only; see amdkge_opt.lazy) | "sparse" (the result of "lazy" for a SharedNegatives / SharedDistanceNegatives step with finite
        lists -- num_negs a number, or "all" over an `entities` pool; mask_known or not --, whose closing sweep visits only the step's
        candidate rows: its positives' s and o and its list ids, include/ext/amdkge_sparse.h; refused without such a sampler;
        save_model / restore_model carry the mode and its sampler); deterministic=True: bitwise reproducible training (AMDKGE_TILED_DETERMINISTIC);
        negatives=None (the train kernels' own draw: a fair coin for the side, a uniform entity) | NegativeSampling | a dict of its
        keywords {"filter", "side", "entities", "max_tries"} (latent_features/negatives.py: rejection of known statements, Bernoulli
        side choice, an entity pool; replicated tables only; model.negative_sampling_stats_ after fit()) | TypedNegatives | its dict
        form {"types": "observed" | RelationTypes, "filter", "side", "entities", "max_tries", "min_size"} (type-constrained: a
        corruption replaces the subject / object by a member of the relation's domain / range set, datasets/types.py; replicated
        tables only; model.relation_types_ after fit(), which evaluate_typed() ranks against) | SharedNegatives | its dict
        form {"shared": num_negs | "all", "group_size", "side", "entities", "mask_known"} (mask_known: False | True | dict of datasets -- the
        scores of corruptions that are known statements are -inf before the loss; "all": every list is every entity, 1-vs-all training;
        model.negative_sampling_stats_ = {"masked", "unmaskable"} after fit(); groups of positives share one list of replacements, scored by a
        matrix product: DistMult / ComplEx / HolE on one GPU, no deterministic, lazy or FocusE mode) | SharedDistanceNegatives | its dict form
        {"shared_distance": num_negs | "all", "group_size", "side", "entities", "mask_known"} (the same step for TransE / RotatE, scored on
        distance tiles; the same refusals) | KvsAll | its dict form {"kvsall": "all", "side", "weight", "known", "group_size"} (KvsAll training,
        all five models: every entity is a binary classification, all known answers of a row's query are labelled 1; only with
        loss=BCELoss({"reduction", "label_smoothing"}), which in turn compiles with nothing else; weight="query" weighs a row by 1 / the rows
        sharing its query; model.negative_sampling_stats_ = {"labelled", "unlabelled_rows"} after fit(); the same refusals).  Multi-GPU, one process per GPU under torch.distributed:
        entity_sharding="replicated" (default: tables replicated, gradient all-reduce) | "rows" (entity table
        row-sharded over the ranks, ampligraph_amd/sharded.py; sharded_negatives="local" | "global" chooses where its corruptions
        are drawn from) | "columns" (tables that fit every GPU: rank r TRAINS on k / W units of every row and the whole batch, one
        all-reduce of the partial scores per step -- ampligraph_amd/colsharded.py.  Memory and host cost of that mode: every rank
        keeps the WHOLE tables and their whole optimizer slots next to its slice -- predict / evaluate / save_weights / callbacks
        read them -- and they are refreshed from the slices through host numpy (all_gather + column merge) after each fit(),
        before each validation pass and, when any rank's fit() was given callbacks, on every rank before the callbacks of every epoch).
        relation_prediction=None (default: nothing changes) | RelationPrediction | its dict form {"weight", "loss", "loss_params",
        "known"} (latent_features/relation_prediction.py): the auxiliary objective of Chen et al. 2021 -- every step adds weight *
        loss over the scores of each positive's (s, o) pair against EVERY relation (loss: "multiclass_nll" by default; known: True --
        the other relations the training set holds for the pair are masked --, a dict of further datasets, or False), computed by
        three fp32 matrix products over the relation table between the step's backward call and the optimizer sweep
        (include/amdkge_relation_objective.h); its weighted loss is part of the epoch loss; model.relation_prediction_stats_ =
        {"masked", "unmaskable"} after fit().  DistMult / ComplEx / HolE on one GPU with replicated tables; no deterministic, lazy or
        FocusE mode.  Like a batch regulariser it makes per-corruption training take the dense-gradient step (train_fwdbwd ->
        train_relation_fwdbwd -> opt_step) instead of the owner-computes one.  Measured once at ComplEx k = 200, B = 10 000, R = 237
        (DESIGN.md section 5): the term adds 0.44 ms per step (DistMult 0.36) -- 0.40 -> 0.83 ms on SharedNegatives(256), 15.1 -> 15.6 ms
        on the all-entities step, 0.15 -> 0.79 ms on the per-corruption step, of which 0.20 are the dense-gradient step's."""
        optimizer_mode = kwargs.pop("optimizer_mode", "dense")
        if optimizer_mode not in ("dense", "lazy", "sparse"):
            raise ValueError("optimizer_mode must be 'dense' (the reference's behaviour), 'lazy' (touched rows only) or 'sparse' (the lazy "
                             "result on the candidate rows of a shared-negative step)")
        self._deterministic = bool(kwargs.pop("deterministic", False))
        self._sharding = kwargs.pop("entity_sharding", "replicated")
        self._sharded_negatives = kwargs.pop("sharded_negatives", "local")
        if self._sharding not in ("replicated", "rows", "columns"):
            raise ValueError("entity_sharding must be 'replicated', 'rows' or 'columns'")
        if self._sharded_negatives not in ("local", "global"):
            raise ValueError("sharded_negatives must be 'local' or 'global'")
        from .negatives import NegativeSampling

        self._negatives = NegativeSampling.get(kwargs.pop("negatives", None))
        if self._negatives is not None and self._sharding != "replicated":
            raise NotImplementedError("negatives: the row- and column-sharded step loops (entity_sharding='rows' / 'columns') build "
                                      "their own corruption overrides and do not take a negative sampler; use replicated tables")
        if optimizer_mode == "sparse":   # needs a sampler that owns its step and draws finite lists (trainer.refuse_sparse has the reasons)
            refuse_sparse(self._negatives)
        if getattr(self._negatives, "shared", False):   # SharedNegatives: what it cannot be combined with
            self._negatives.check_model(self, optimizer_mode)
        from .relation_prediction import RelationPrediction

        self._relation_prediction = RelationPrediction.get(kwargs.pop("relation_prediction", None))
        if self._relation_prediction is not None:   # what the term cannot be combined with
            self._relation_prediction.check_model(self, optimizer_mode)
        self.optimizer = optimizers.get(optimizer)
        if optimizer_mode == "lazy":
            # DEVIATION from the reference (its optimizer is dense, optimizers.py:136-168): only rows that received a
            # gradient this step are updated and regularised -- TF-Addons LazyAdam semantics (amdkge_opt.lazy)
            self.optimizer.lazy = True
        if optimizer_mode == "sparse":
            # the same DEVIATION with the same result (an entity row moves iff its gradient row is not all zero), at a cost that does
            # not depend on the table: the sweep visits the rows the sampler names (include/ext/amdkge_sparse.h)
            self.optimizer.sparse = True
        if loss is None:
            raise ValueError("compile(): a loss is required")
        self.loss = loss_functions.get(loss)
        # KvsAll and BCELoss exist only together (include/amdkge_shared_labels.h: the labels are the loss step's)
        if getattr(self._negatives, "kvsall", False) and not getattr(self.loss, "labelled", False):
            raise NotImplementedError("negatives: KvsAll labels every entity for a binary cross-entropy and takes loss=BCELoss(...) only; the softmax "
                                      "over every entity with the other known answers masked is SharedNegatives('all', mask_known=True) "
                                      "with loss='multiclass_nll', not {!r}".format(self.loss.name))
        if getattr(self.loss, "labelled", False) and not getattr(self._negatives, "kvsall", False):
            raise NotImplementedError("loss: BCELoss is the loss of KvsAll training: compile(negatives=KvsAll(...), loss=BCELoss(...))")
        ini = entity_relation_initializer
        self._initializers = list(ini) if isinstance(ini, (list, tuple)) else [ini, ini]
        if len(self._initializers) != 2:
            raise ValueError("entity_relation_initializer must be one value or a pair [entity, relation]")
        if self.scoring_type == "RotatE":  # :1312-1315
            r = self._initializers[1]
            assert isinstance(r, str) and r.lower() == "glorot_uniform", \
                "RotatE requires the relation embeddings to be initialised with GlorotUniform"
        reg = entity_relation_regularizer
        regs = list(reg) if isinstance(reg, (list, tuple)) else [reg, reg]
        if len(regs) != 2:   # EmbeddingLookupLayer.py:147-150
            raise AssertionError("Incorrect length for regularizer. Expected 2, got {}".format(len(regs)))
        # independent per table, either may be None, each a sum of at most two LP terms (EmbeddingLookupLayer.py:131-155)
        self._regularizers = [regularizers.get(r) for r in regs]
        if any(regularizers.is_batch(r) for r in self._regularizers):   # BatchLPRegularizer: what it cannot be combined with
            refuse_modes(*BATCH_REG, deterministic=self._deterministic, lazy=optimizer_mode == "lazy", sharding=self._sharding)
            for r, table in zip(self._regularizers, ("ent", "rel")):
                if regularizers.is_batch(r):
                    r.norm_for(self.scoring_type, table)   # ValueError: norm="modulus" on rows without complex units
        self.is_compiled = True

    def _assert_compile_was_called(self):
        if not self.is_compiled:
            raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`.")

    # ------------------------------------------------------------------------------------ engine
    EVAL_CHUNK_SHARDED = 4096   # test triples per sharded evaluation / prediction pass (2 scratch rows each)

    def _build(self, n_ents, n_rels, batch_size=None, tables=None):
        from .. import placement

        self.max_ent_size, self.max_rel_size = int(n_ents), int(n_rels)
        self._n_ents, self._n_rels = int(n_ents), int(n_rels)
        self._filter_cache = (None, None)   # a new id map invalidates cached filter indexes
        self._loop = None                   # the step loop is bound to the engine built below
        K = self.internal_k
        if tables is None:
            cost = stream_cost(self._initializers[0], (n_ents, K))
            if cost is not None:   # a rank can draw just ITS rows of the whole-table stream (initializers.RowSource)
                ent_rows = RowSource(self._initializers[0], (n_ents, K), self.seed, 0).rows
                rel = RowSource(self._initializers[1], (n_rels, K), self.seed, cost).rows(0, n_rels)
            else:
                rng = np.random.Generator(np.random.PCG64(self.seed))
                ent = initialise(self._initializers[0], (n_ents, K), rng)
                rel = initialise(self._initializers[1], (n_rels, K), rng)
                ent_rows = lambda lo, hi: ent[lo:hi]   # noqa: E731
        else:
            ent, rel = tables
            ent_rows = ent if callable(ent) else (lambda lo, hi: ent[lo:hi])
        d = self._dist()
        kind = placement.Replicated   # (what a single rank uses, whatever entity_sharding says)
        if d is not None and self._sharding != "replicated":
            kind = placement.Rows if self._sharding == "rows" else placement.Columns
        self._placement = kind(self, d, n_ents, n_rels, ent_rows, rel, batch_size)

    def _dist(self):
        if self._dist_override is not None:
            return self._dist_override if self._dist_override.get_world_size() > 1 else None
        import torch.distributed as dist

        return dist if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) else None

    def _make_loop(self):
        return self._placement.make_loop()

    # ------------------------------------------------------------------------------------ fit
    def fit(self, x=None, batch_size=1000, epochs=100, verbose=True, callbacks=None, validation_split=0.0,
            validation_data=None, shuffle=True, initial_epoch=0, validation_batch_size=10,
            validation_corrupt_side="s,o", validation_freq=10, validation_burn_in=0, validation_filter=False,
            validation_entities_subset=None, partitioning_k=1, focusE=False, focusE_params={}):
        """:544-883.  Batches are sequential, un-shuffled slices of `x` with a short last batch
        (graph_data_loader.py:472-523); `shuffle` is accepted and, like in the reference (:553), unused."""
        import torch

        self._assert_compile_was_called()
        if partitioning_k != 1:
            raise NotImplementedError("partitioning_k > 1: tables are HBM-resident on MI355X, graph partitioning "
                                      "with disk swapping is out of scope (SURVEY.md section 2, rows 15-16)")
        X = _load_triples(x)
        if validation_split:   # :719-728: carve the validation set out of x without creating unseen entities
            assert isinstance(x, np.ndarray), "Validation split supported for numpy arrays only!"
            from ..evaluation.protocol import train_test_split_no_unseen

            X, validation_data = train_test_split_no_unseen(X, test_size=validation_split, seed=self.seed,
                                                            allow_duplication=False)
        # FocusE (:714-790): active only when asked for AND the data carries numeric columns behind s, p, o
        self.use_focusE = bool(focusE) and X.shape[1] > 3
        focus_w = None
        if self.use_focusE:
            assert isinstance(focusE_params, dict), "focusE parameters need to be in a dict!"
            nl = focusE_params.get("non_linearity", "linear")
            if nl not in _ffi.FOCUS_NONLINEARITY:
                raise ValueError("Invalid focusE non-linearity")
            stop_epoch = focusE_params.get("stop_epoch", 251)
            assert stop_epoch >= 0, "Invalid value for focusE stop_epoch: expected a value >=0 but got {}".format(stop_epoch)
            structural_wt = focusE_params.get("structural_wt", 0.001)
            assert 0 <= structural_wt <= 1, "Invalid focusE 'structural_wt' passed! It has to belong to [0,1]."
            self.focusE_params = {"non_linearity": nl, "stop_epoch": stop_epoch, "structural_wt": structural_wt}
            focus_w = np.ascontiguousarray(X[:, 3:].astype(np.float32).mean(axis=1), dtype=np.float32)   # :360
        elif X.shape[1] > 3:
            print("Data shape is {}: not only triples were given, but focusE is not active!".format(X.shape[1]))
        if self.data_indexer is None or not self.is_fitted:
            self.data_indexer = DataIndexer(X)
            Xi = self.data_indexer.get_indexes(X[:, :3])
            self._build(self.data_indexer.get_entities_count(), self.data_indexer.get_relations_count(), batch_size)
        else:  # continue training (initial_epoch > 0): same id map, same tables
            Xi = self.data_indexer.get_indexes(X[:, :3])
            self._placement.ensure_capacity(batch_size)
        eng = self._engine
        if self._loop is None:
            self._loop = self._make_loop()
        loop = self._loop
        if any(regularizers.is_batch(r) for r in self._regularizers):
            refuse_modes(*BATCH_REG, **fit_modes(self))
        cbs = list(callbacks or [])
        self._placement.begin_fit(bool(cbs))
        # negatives are keyed by a step counter that continues where the optimizer's iteration count stands: a run resumed
        # from a checkpoint draws what the uninterrupted run would have drawn, and a second fit() draws fresh negatives
        rng_base = int(self.optimizer.iterations)
        if hasattr(loop, "configure_for_data"):
            loop.configure_for_data(Xi, batch_size)
        train = torch.as_tensor(np.ascontiguousarray(Xi, dtype=np.int32)).to(eng.device)
        n = int(train.shape[0])
        # the negative sampler is bound here, where the id map and the training tensor exist: filter index, the ranges of all n
        # rows, thresholds and pool are made once; a step slices them (negatives.BoundNegatives).  Only trainer.StepLoop has the
        # sampler attribute: ShardedStepLoop.negatives is that loop's own "local" | "global" setting and is never touched here
        # (compile() refuses a sampler on sharded tables)
        if type(loop) is StepLoop:
            loop.negatives = None if self._negatives is None else self._negatives.bind(self, eng, train)
            loop.relation = None if self._relation_prediction is None else self._relation_prediction.bind(self, eng, train)
        elif self._negatives is not None:
            raise NotImplementedError("negatives: only the replicated step loop takes a negative sampler")
        elif self._relation_prediction is not None:
            raise NotImplementedError("relation_prediction: only the replicated step loop takes the relation objective")
        focus_dev = None
        if focus_w is not None:
            if focus_w.shape[0] != n:
                raise ValueError("FocusE: rows with unknown entities/relations were dropped; weights no longer align")
            focus_dev = torch.as_tensor(focus_w).to(eng.device)
        batch_size = int(batch_size)
        steps = (n + batch_size - 1) // batch_size
        self.history = History()
        for cb in cbs:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
            if hasattr(cb, "on_train_begin"):
                cb.on_train_begin()
        self.stop_training = False
        if isinstance(validation_entities_subset, str) and validation_entities_subset == "all":
            validation_entities_subset = None
        for epoch in range(int(initial_epoch), int(epochs)):
            self.current_epoch = epoch
            loop.reset_loss()
            focus = None
            if focus_dev is not None:   # update_focusE_params (:536-542): linear decay of the structural weight
                fp = self.focusE_params
                if fp["stop_epoch"] > 0:
                    fp["structural_wt"] = max(1.0 - epoch / fp["stop_epoch"], 0.001)
            first = 0
            if (epoch == int(initial_epoch) and getattr(loop, "auto_tune", False) and getattr(loop, "world", 1) > 1
                    and focus_dev is None and steps >= 24):
                # AMDKGE_DP_MERGE=auto: the first steps of this epoch are run under each gradient-merge schedule and the
                # fastest is kept (StepLoop.tune_merge; every schedule computes the same update).  The epoch's reported
                # loss then covers the remaining steps only.
                base = rng_base
                first = loop.tune_merge(lambda s_: train[(s_ - base) * batch_size:(s_ - base + 1) * batch_size], base)
                loop.auto_tune = False
            for step in range(first, steps):
                b0 = step * batch_size
                if focus_dev is not None:
                    focus = (focus_dev[b0:b0 + batch_size], self.focusE_params["structural_wt"], self.focusE_params["non_linearity"])
                    loop.step(train[b0:b0 + batch_size], rng_base + (epoch - int(initial_epoch)) * steps + step, focus)
                else:
                    loop.step(train[b0:b0 + batch_size], rng_base + (epoch - int(initial_epoch)) * steps + step)
            logs = {"loss": loop.mean_batch_loss()}
            validate = (epoch >= (validation_burn_in - 1) and validation_data is not None
                        and (epoch + 1) % int(validation_freq) == 0)
            if validate:
                self.is_fitted = True
                self._placement.publish()
                ranks = self.evaluate(validation_data, batch_size=validation_batch_size or batch_size,
                                      use_filter=validation_filter, dataset_type="valid",
                                      corrupt_side=validation_corrupt_side,
                                      entities_subset=validation_entities_subset, verbose=False)
                logs.update({"val_mrr": mrr_score(ranks), "val_mr": mr_score(ranks),
                             "val_hits@1": hits_at_n_score(ranks, 1), "val_hits@10": hits_at_n_score(ranks, 10),
                             "val_hits@100": hits_at_n_score(ranks, 100)})  # :1857-1863
            self.history._log(epoch, logs)
            if verbose:
                print(f"Epoch {epoch + 1}/{epochs} - " + " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
            # callbacks read AND write the tables (EarlyStopping snapshots them, and restores the best ones just before it stops
            # the run): they see this epoch's, and nothing published after them overwrites what they restored
            self._placement.before_callbacks()
            for cb in cbs:
                if hasattr(cb, "on_epoch_end"):
                    cb.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        self._placement.publish()
        if hasattr(getattr(loop, "negatives", None), "stats"):
            self.negative_sampling_stats_ = loop.negatives.stats()   # {"redraws", "exhausted"} of this fit(): one read-back
        if getattr(loop, "relation", None) is not None:
            self.relation_prediction_stats_ = loop.relation.stats()   # {"masked", "unmaskable"} of this fit(): one read-back
        if hasattr(getattr(loop, "negatives", None), "relation_types"):
            self.relation_types_ = loop.negatives.relation_types     # TypedNegatives: the bound sets, evaluate_typed()'s default
        for cb in cbs:
            if hasattr(cb, "on_train_end"):
                cb.on_train_end()
        self.is_fitted = True
        return self.history

    # ------------------------------------------------------------------------------------ filters
    def _cached_index(self, cls, cache_attr, use_filter, Xi):
        """An index of class `cls` over the union of the given datasets (dict) or the evaluated data itself (True), all indexed
        with the training id map (graph_data_loader.py:184-190,652-653); None for no filter.  The id mapping is host work
        (labels), the index itself (sort + CSR) is built on the device (kge_filter.hip).  The last dict's index is kept in
        self.<cache_attr> = (content checksum key, index), so validation during fit() and repeated calls reuse it."""
        try:   # (content checksum of the filter arrays: xxh3 runs at ~10 GB/s, zlib's crc32 at ~2)
            from xxhash import xxh3_64_intdigest as _digest
        except Exception:   # pragma: no cover
            from zlib import crc32 as _digest

        if isinstance(use_filter, dict):
            arrays = [_load_triples(v)[:, :3] for v in use_filter.values()]
            key = []
            for a in arrays:
                a = np.ascontiguousarray(a)
                if a.dtype == object:
                    key = None
                    break
                key.append((a.shape, str(a.dtype), _digest(a.view(np.uint8).reshape(-1))))
            key = None if key is None else ("dict", tuple(key), self._n_ents, self._n_rels)
            if key is not None and getattr(self, cache_attr, (None, None))[0] == key:
                return getattr(self, cache_attr)[1]
            fi = cls([self.data_indexer.get_indexes(a) for a in arrays], self._n_ents, self._n_rels, engine=self._engine)
            if key is not None:
                setattr(self, cache_attr, (key, fi))
            return fi
        if use_filter:
            return cls([Xi], self._n_ents, self._n_rels, engine=self._engine)
        return None

    def _filter_index(self, use_filter, Xi):
        """FilterIndex for evaluate() (amdkge_filter_build), cached in _filter_cache."""
        return self._cached_index(FilterIndex, "_filter_cache", use_filter, Xi)

    def _pair_filter_index(self, use_filter, Xi):
        """PairFilterIndex for evaluate_relations() / query_topn_relations(): the (s, o) pair as the key, the SET of relations known
        between the two (amdkge_pair_filter_build), in a cache of its own (_pair_filter_cache)."""
        return self._cached_index(PairFilterIndex, "_pair_filter_cache", use_filter, Xi)

    # ------------------------------------------------------------------------------------ predict
    def _index_test(self, x):
        assert self.is_fitted, "Model is not fit on the data yet!"
        X = _load_triples(x)
        return np.ascontiguousarray(self.data_indexer.get_indexes(X[:, :3]), dtype=np.int32)

    def predict(self, x, batch_size=32, verbose=0, callbacks=None):
        """:1736-1823: float32 (n,) scores in input order (rows with unknown keys dropped)."""
        import torch

        Xi = self._index_test(x)
        if Xi.shape[0] == 0:
            return np.zeros(0, dtype=np.float32)
        return self._placement.score(torch.as_tensor(Xi).to(self._engine.device)).cpu().numpy()

    # ------------------------------------------------------------------------------------ evaluate
    def evaluate(self, x=None, batch_size=10, verbose=True, use_filter=False, corrupt_side="s,o",
                 entities_subset=None, ranking_strategy="worst", callbacks=None, dataset_type="test"):
        """:1516-1692: int32 ranks (n, 1|2), 1-based, reference tie/filter semantics.  `batch_size` (the reference's default, 10,
        :1519) only chunked the TF graph in the reference; results do not depend on it and it is ignored here."""
        assert corrupt_side in ["s", "o", "s,o", "s+o"], "Invalid value for corrupt_side"
        assert ranking_strategy in ["best", "middle", "worst"], "Invalid value for ranking_strategy"
        Xi = self._index_test(x)
        n = Xi.shape[0]
        sides = [sd for sd in ("s", "o") if sd in corrupt_side]
        if n == 0:
            return np.zeros((0, 1 if corrupt_side in ("s", "o", "s+o") else 2), dtype=np.int32)
        # filters (graph_data_loader.py:184-190,652-653): True -> the evaluated data filters itself;
        # dict -> union of the given datasets, all indexed with the training id map
        fi = self._filter_index(use_filter, Xi)
        subset = None
        if entities_subset is not None and len(entities_subset) > 0:
            subset = np.asarray(self.data_indexer.get_indexes(np.asarray(entities_subset), "e"))
        r = self._placement.rank(Xi, sides, fi, subset, ranking_strategy).cpu().numpy()
        if corrupt_side == "s+o":  # :1459-1463 sums the two 0-based sides, then +1 (:1684)
            r = (r.sum(1, keepdims=True) - 1).astype(np.int32)
        return r

    def evaluate_relations(self, x, use_filter=False, relations_subset=None, ranking_strategy="worst", verbose=False):
        """Relation prediction's evaluate() (the reference has none): int32 ranks (n, 1), 1-based, of each triple's relation among
        the candidate relations for its (s, o) pair -- every relation, or `relations_subset` with entities_subset's semantics (the
        true relation's score is compared with the subset's, whether or not it is in it).  Ties and filters as in evaluate():
        `ranking_strategy` worst / best / middle over the quantised scores; `use_filter` False, True (the evaluated data filters
        itself) or a dict of datasets -- a relation KNOWN between s and o in them is not a competitor.  Unfiltered, a triple's own
        relation is a candidate and counts as its own competitor, as an entity does in evaluate().  Rows with unseen labels
        are dropped.  The result feeds mrr_score / hits_at_n_score as is.  One 1-vs-all pass over the relation table per chunk
        of queries (amdkge_relation_scores); works on every placement."""
        if ranking_strategy not in ("best", "middle", "worst"):
            raise ValueError("`ranking_strategy` must be 'worst', 'best' or 'middle', got {!r}.".format(ranking_strategy))
        if not self.is_fitted:
            raise ValueError("Model is not fitted.")
        if use_filter is None:
            use_filter = False
        if not isinstance(use_filter, (bool, dict)):
            raise ValueError("`use_filter` must be False, True or a dict of datasets.")
        Xi = self._index_test(x)
        if Xi.shape[0] == 0:
            return np.zeros((0, 1), dtype=np.int32)
        subset = None
        if relations_subset is not None and len(relations_subset) > 0:
            subset = np.asarray(self.data_indexer.get_indexes(np.asarray(relations_subset), "r"))
        fi = self._pair_filter_index(use_filter, Xi)
        return self._placement.rank_relations(Xi, fi, subset, ranking_strategy).cpu().numpy().reshape(-1, 1)

    def evaluate_candidates(self, x, candidates_s=None, candidates_o=None, use_filter=False, ranking_strategy="worst", verbose=False):
        """evaluate() against PER-TRIPLE candidate lists (the reference has none): int32 ranks (n, number of sides given), 1-based,
        columns in the order s, o -- sampled negatives (ogbl-wikikg2's 500 heads and 500 tails per test triple), re-ranking the
        output of a first stage, type-constrained evaluation.  They feed mrr_score / hits_at_n_score as they are.

        candidates_s / candidates_o: the entities that replace the subject / the object, as a 2-D array [n, C] of entity labels or
        a sequence of n 1-D label arrays (ragged; a list may be empty); at least one side must be given.  Row i of `x` is
        ranked against list i alone, with entities_subset's semantics: the true triple's score is compared with its
        candidates', whether or not its own entity is listed (listed, it competes with itself as in evaluate()).  Ties and filters
        as in evaluate(): `ranking_strategy` worst / best / middle over the quantised scores; `use_filter` False, True (the
        evaluated data filters itself) or a dict of datasets -- a candidate that is a KNOWN positive of the triple's (p, o) /
        (s, p) is not a competitor.  On duplicate-free lists the rank is evaluate(x[i:i+1], entities_subset=list_i, ...)'s.
        DUPLICATES: every occurrence of an entity in a list is a candidate of its own, so a repeated entity is counted each
        time (the reference's subset is a set), and a repeated known positive is likewise filtered each time.

        Lists and rows must stay aligned, so nothing is dropped silently: an unknown candidate label, or a row of `x` with an
        unseen label, raises ValueError.  One gather of the listed rows per side (amdkge_rank_lists): the cost is the
        candidates', not the entity table's.  Needs the whole table on one GPU: row- / column-sharded models raise
        NotImplementedError."""
        from ..evaluation.candidates import csr_of, list_lengths

        if ranking_strategy not in ("best", "middle", "worst"):
            raise ValueError("`ranking_strategy` must be 'worst', 'best' or 'middle', got {!r}.".format(ranking_strategy))
        if not self.is_fitted:
            raise ValueError("Model is not fitted.")
        if use_filter is None:
            use_filter = False
        if not isinstance(use_filter, (bool, dict)):
            raise ValueError("`use_filter` must be False, True or a dict of datasets.")
        given = [(sd, c) for sd, c in (("s", candidates_s), ("o", candidates_o)) if c is not None]
        if not given:
            raise ValueError("evaluate_candidates needs `candidates_s`, `candidates_o` or both.")
        X = _load_triples(x)
        Xi = self._index_test(X)
        if Xi.shape[0] != X.shape[0]:
            raise ValueError("{} of the {} rows of `x` have unseen labels: candidate lists and rows must stay aligned, remove "
                             "them (and their lists) first.".format(X.shape[0] - Xi.shape[0], X.shape[0]))
        n = Xi.shape[0]
        sides = []
        for sd, c in given:
            lens, labels = list_lengths(c if isinstance(c, np.ndarray) else list(c), n)
            ids = np.asarray(self.data_indexer.get_indexes(labels, "e")) if labels.shape[0] else np.zeros(0, dtype=np.int32)
            if ids.shape[0] != labels.shape[0]:
                raise ValueError("candidates_{}: {} of the {} candidate labels are unknown to the model.".format(
                    sd, labels.shape[0] - ids.shape[0], labels.shape[0]))
            sides.append((sd, csr_of(lens, ids)))
        if n == 0:
            return np.zeros((0, len(sides)), dtype=np.int32)
        fi = self._filter_index(use_filter, Xi)
        return self._placement.rank_candidates(Xi, sides, fi, ranking_strategy).cpu().numpy()

    def evaluate_typed(self, x, types=None, use_filter=False, corrupt_side="s,o", ranking_strategy="worst", min_size=1, verbose=False):
        """TYPE-CONSTRAINED evaluate() (the reference has none; PyKEEN's / LibKGE's / Krompass et al.'s protocol): int32 ranks,
        1-based, shaped like evaluate()'s ("s+o" included), of row i's subject among the DOMAIN set of its relation and of its
        object among the RANGE set, with entities_subset's semantics -- the true entity's score is compared with the set's,
        whether or not it is listed.

        types: a datasets.types.RelationTypes (observed in given datasets, or explicit), an already bound one, or None = the sets
        the last fit() with TypedNegatives left in model.relation_types_ (ValueError when there are none; observed() without
        datasets is valid in training only and raises ValueError here).  A relation that is unconstrained on a side, or whose
        set has fewer than `min_size` ids, is ranked against ALL entities: then the rank is evaluate()'s.  Ties and filters as
        in evaluate().  Rows with unseen labels are dropped, as evaluate() drops them.

        Nothing per triple is built on the host: a triple's candidates are a [lo, hi) range into the sets' one id array, looked up
        on the device (amdkge_relation_sets_ranges), and each side is one amdkge_rank_lists pass per chunk of 65 536 triples.  The
        cost is the sets', not the entity table's -- see DESIGN.md for where per-relation evaluate(entities_subset=) calls win.
        Needs the whole table on one GPU: row- / column-sharded models raise NotImplementedError."""
        from ..datasets.types import BoundRelationTypes, RelationTypes

        if corrupt_side not in ("s", "o", "s,o", "s+o"):
            raise ValueError("Invalid value for corrupt_side")
        if ranking_strategy not in ("best", "middle", "worst"):
            raise ValueError("`ranking_strategy` must be 'worst', 'best' or 'middle', got {!r}.".format(ranking_strategy))
        if not self.is_fitted:
            raise ValueError("Model is not fitted.")
        if use_filter is None:
            use_filter = False
        if not isinstance(use_filter, (bool, dict)):
            raise ValueError("`use_filter` must be False, True or a dict of datasets.")
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or int(min_size) < 0:
            raise ValueError("`min_size` must be a non-negative integer.")
        if not self._placement.lists_supported:
            self._placement.rank_typed(None, None, None, None, None, None)   # raises NotImplementedError before any device work
        if types is None:
            types = getattr(self, "relation_types_", None)
            if types is None:
                raise ValueError("evaluate_typed: no `types` given and the model has no relation_types_ (fit() with TypedNegatives binds them).")
        if isinstance(types, RelationTypes):
            types = types.bind(self, self._engine)
        if not isinstance(types, BoundRelationTypes):
            raise ValueError("`types` must be None, a RelationTypes or a bound one.")
        if (types.n_ents, types.n_rels) != (self._n_ents, self._n_rels) or types.engine.device != self._engine.device:
            raise ValueError("evaluate_typed: the bound relation types belong to another model.")
        Xi = self._index_test(x)
        sides = [sd for sd in ("s", "o") if sd in corrupt_side]
        if Xi.shape[0] == 0:
            return np.zeros((0, 1 if corrupt_side in ("s", "o", "s+o") else 2), dtype=np.int32)
        fi = self._filter_index(use_filter, Xi)
        r = self._placement.rank_typed(Xi, sides, types, fi, ranking_strategy, int(min_size)).cpu().numpy()
        if corrupt_side == "s+o":
            r = (r.sum(1, keepdims=True) - 1).astype(np.int32)
        return r

    # ------------------------------------------------------------------------------------ accessors
    def is_fit(self):
        return self.is_fitted

    def get_indexes(self, X, type_of="t", order="raw2ind"):
        return self.data_indexer.get_indexes(X, type_of, order)

    def get_count(self, concept_type="e"):
        assert self.is_fitted, "Model is not fit on the data yet!"
        if concept_type == "e":
            return self.data_indexer.get_entities_count()
        if concept_type == "r":
            return self.data_indexer.get_relations_count()
        raise ValueError("Invalid Concept Type (expected 'e' or 'r')")

    def get_train_embedding_matrix_size(self):
        assert self.is_fitted, "Model is not fit on the data yet!"
        return {"e": (self._n_ents, self.internal_k), "r": (self._n_rels, self.internal_k)}

    def get_embeddings(self, entities, embedding_type="e"):
        """:2214-2277."""
        if embedding_type not in ("e", "r"):
            raise ValueError("Invalid entity type: {}".format(embedding_type))
        assert self.is_fitted, "Model is not fit on the data yet!"
        idx = np.asarray(self.data_indexer.get_indexes(np.asarray(entities), embedding_type), dtype=np.int64)
        import torch

        tab = self._placement.entity_table() if embedding_type == "e" else self._engine.rel
        return self._engine.unpack(tab[torch.as_tensor(idx).to(tab.device)]).cpu().numpy()

    # ------------------------------------------------------------------------------------ calibration
    def calibrate(self, X_pos, X_neg=None, positive_base_rate=None, batch_size=32, epochs=50, verbose=0):
        """:1922-2122 -- Platt scaling of the scores (CalibrationLayer, layers/calibration/calibrate.py:11-129): two
        scalars (w, b) fitted with Adam (Keras defaults) on sigmoid cross-entropy, one update per batch of positives.
        With X_neg the negatives are iterated in lock step (their batch size adjusted so that both have the same
        number of batches, :2033-2052); without, one corruption per positive is generated per step
        (corruption_layer(inputs, num_ents, 1), :1886) -- here from the Philox stream keyed by (seed, step).
        Scores, corruptions and the objective/gradient reduction are libamdkge kernels; the scalar Adam runs on host."""
        import math

        import torch

        assert self.is_fitted, "Model is not fit on the data yet!"
        self.is_calibrated = False
        eng = self._engine
        Xp = self._index_test(X_pos)
        pos_size = int(Xp.shape[0])
        neg_size = pos_size
        batch_size = int(batch_size)
        Xn = None
        if X_neg is None:
            assert positive_base_rate is not None, "Please provide the negatives or positive base rate!"
        else:
            Xn = self._index_test(X_neg)
            neg_size = int(Xn.shape[0])
            if positive_base_rate is None:
                positive_base_rate = pos_size / (pos_size + neg_size)
        if positive_base_rate is not None and (positive_base_rate <= 0 or positive_base_rate >= 1):
            raise ValueError("positive_base_rate must be a value between 0 and 1.")
        n_batches = max(1, -(-pos_size // batch_size))
        bs_neg = batch_size
        if Xn is not None and -(-neg_size // batch_size) != n_batches:
            bs_neg = -(-neg_size // n_batches)
        # CalibrationLayer.__init__ / call constants
        w, b = 0.0, float(np.float32(math.log((neg_size + 1.0) / (pos_size + 1.0))))
        label_pos, label_neg = (pos_size + 1.0) / (pos_size + 2.0), 1.0 / (neg_size + 2.0)
        weight_neg = (1.0 - positive_base_rate) / positive_base_rate
        dev = eng.device
        Xpd = torch.as_tensor(Xp).to(dev)
        # row-sharded tables: the same code, the placement's scores are the same on every rank
        sp_all = self._placement.score(Xpd) if pos_size else None    # the embeddings are frozen: score once
        sn_all = self._placement.score(torch.as_tensor(Xn).to(dev)) if Xn is not None and neg_size else None
        slots = [(0.0, 0.0), (0.0, 0.0)]
        t = 0
        for epoch in range(int(epochs)):
            for bi in range(n_batches):
                sp = sp_all[bi * batch_size:(bi + 1) * batch_size]
                if sn_all is not None:
                    sn = sn_all[bi * bs_neg:(bi + 1) * bs_neg]
                else:
                    neg = eng.sample_corruptions(Xpd[bi * batch_size:(bi + 1) * batch_size], 1, self.seed, t,
                                                 sample_range=self._n_ents)
                    sn = self._placement.score(neg)
                if sp.shape[0] == 0:
                    continue
                t += 1
                loss, gw, gb = eng.platt_step(sp, sn, w, b, label_pos, label_neg, sn.shape[0] / sp.shape[0], weight_neg)
                alpha = 0.001 * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)   # tf.keras.optimizers.Adam() defaults
                upd = []
                for i, (p_, g_) in enumerate(((w, gw), (b, gb))):
                    m, v = slots[i]
                    m += (g_ - m) * (1.0 - 0.9)
                    v += (g_ * g_ - v) * (1.0 - 0.999)
                    slots[i] = (m, v)
                    upd.append(p_ - m * alpha / (math.sqrt(v) + 1e-7))
                w, b = upd
            if verbose:
                print(f"calibration epoch {epoch + 1}/{epochs} - loss: {loss:.6f}")
        self.calibration_parameters = {"calib_w": float(w), "calib_b": float(b), "pos_size": pos_size,
                                       "neg_size": neg_size, "positive_base_rate": float(positive_base_rate)}
        self.is_calibrated = True

    def predict_proba(self, x, batch_size=32, verbose=0, callbacks=None):
        """:2124-2212: sigmoid(-(w * score + b)) of the calibrated model (CalibrationLayer.call(training=0))."""
        if not self.is_calibrated:
            raise RuntimeError("Model has not been calibrated. Please call `model.calibrate(...)` before predicting probabilities.")
        s = self.predict(x, batch_size=batch_size).astype(np.float32)
        w = np.float32(self.calibration_parameters["calib_w"])
        b = np.float32(self.calibration_parameters["calib_b"])
        return (1.0 / (1.0 + np.exp((w * s + b).astype(np.float64)))).astype(np.float32)

    # ------------------------------------------------------------------------------------ persistence
    def save_weights(self, filepath):
        """Own flat format (the reference writes a TF checkpoint, :1046-1071): <filepath>.npz holds tables,
        optimizer slots and id maps; <filepath>.json the hyper-parameters.  Collective under torch.distributed: call on
        every rank; rank 0 writes these files.

        Row-sharded mode: rank r also writes ITS rows of the entity table and of the optimizer slots to
        <filepath>.shardRRR-of-WWW.npz, and <filepath>.npz holds the replicated part (relation table + slots, id maps,
        `shard_world`).  Nothing is gathered, so it works at C5 scale; load_weights() re-slices, so a checkpoint can be resumed
        on a different number of GPUs (or on one)."""
        assert self.is_fitted, "Model is not fit on the data yet!"
        arrays = self._placement.save(filepath, self._loop)
        if arrays is not None:   # (the writing rank)
            st = self.data_indexer.state()
            arrays["ent_raw"], arrays["rel_raw"] = st["ent_raw"], st["rel_raw"]
            # written under a temporary name and renamed: a reader never sees a torn archive
            with open(filepath + ".npz.tmp", "wb") as f:
                np.savez(f, **arrays)
            os.replace(filepath + ".npz.tmp", filepath + ".npz")
            meta = {"eta": self.eta, "k": self.k, "scoring_type": self.scoring_type, "seed": self.seed,
                    "optimizer": self.optimizer.get_config() if self.is_compiled else None,
                    "iterations": self.optimizer.iterations if self.is_compiled else 0,
                    "loss": {"name": self.loss.name, "params": self.loss._loss_parameters} if self.is_compiled else None,
                    "calibration": self.calibration_parameters if self.is_calibrated else None,
                    "regularizer": [regularizers.to_config(r) for r in self._regularizers] if self.is_compiled else None}
            with open(filepath + ".json.tmp", "w") as f:
                json.dump(meta, f)
            os.replace(filepath + ".json.tmp", filepath + ".json")
        if self._placement.dist is not None:
            self._placement.dist.barrier()   # every rank returns once the files are complete

    def load_weights(self, filepath):
        """Whole-table or row-sharded checkpoint -> this model, whatever its own sharding (rows are re-sliced)."""
        from ..placement import shard_file
        from ..sharded import ShardSpec

        z = np.load(filepath + ".npz", allow_pickle=False)
        self.data_indexer = DataIndexer.from_state({"ent_raw": z["ent_raw"], "rel_raw": z["rel_raw"]})
        if not self.is_compiled:
            self._initializers = ["zeros", "zeros"]
        saved_world = int(z["shard_world"]) if "shard_world" in z.files else 0
        n_ents = int(z["n_ents"]) if saved_world else int(z["ent"].shape[0])

        def rows_of(key):
            if not saved_world:
                arr = z[key]
                return lambda lo, hi: arr[lo:hi]
            shards = {}

            def rows(lo, hi):
                out = []
                for r in range(saved_world):
                    s = ShardSpec(n_ents, saved_world, r)
                    if s.hi <= lo or s.lo >= hi or s.n_local == 0:
                        continue
                    if r not in shards:
                        shards.clear()   # one shard file in memory at a time
                        shards[r] = np.load(shard_file(filepath, r, saved_world), allow_pickle=False)[key]
                    out.append(shards[r][max(lo, s.lo) - s.lo:min(hi, s.hi) - s.lo])
                return np.concatenate(out) if out else np.zeros((0, self.internal_k), np.float32)
            return rows

        self._build(n_ents, z["rel"].shape[0], tables=(rows_of("ent"), z["rel"]))
        slot_keys = [k[5:] for k in z.files if k.startswith("slot_")]
        if saved_world:
            s0 = np.load(shard_file(filepath, 0, saved_world), allow_pickle=False)
            slot_keys += [k[5:] for k in s0.files if k.startswith("slot_")]
        if slot_keys and self.is_compiled:
            self._loop = self._make_loop()
            eng = self._engine
            for kname in slot_keys:
                if kname not in eng.slots:
                    continue   # checkpoint of another optimizer
                if kname.endswith("_e"):   # (this rank's rows of them)
                    self._placement.upload_rows(eng.slots[kname], rows_of("slot_" + kname))
                else:
                    eng.pack(z["slot_" + kname], out=eng.slots[kname])
            if os.path.exists(filepath + ".json"):
                self.optimizer.iterations = int(json.load(open(filepath + ".json")).get("iterations", 0))
        if os.path.exists(filepath + ".json"):
            cal = json.load(open(filepath + ".json")).get("calibration")
            if cal:
                self.calibration_parameters, self.is_calibrated = cal, True
        self.is_fitted = True
