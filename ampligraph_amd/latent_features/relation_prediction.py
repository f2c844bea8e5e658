"""The relation-prediction training objective (Chen et al. 2021, "Relation Prediction as an Auxiliary Training Objective"): next to
the step's own loss over corrupted entities, every positive (s, p, o) is scored against EVERY relation and `loss` -- the softmax
cross-entropy multiclass_nll by default -- asks for p among them, times `weight` (the paper's lambda).  The step is
engine.train_relation_fwdbwd (include/amdkge_relation_objective.h; kge_train_relpred.hip: three exact-fp32 matrix products over the
relation table), which trainer.StepLoop.step runs between the main backward call and the optimizer sweep.  DistMult, ComplEx and
HolE, whose score is linear in the relation row; one GPU, replicated tables; no deterministic, lazy or FocusE mode.

    model.compile(..., relation_prediction=RelationPrediction(weight=0.25))
    model.compile(..., relation_prediction={"weight": 0.25, "loss": "multiclass_nll", "known": True})
"""
import math

import numpy as np

from ..datasets.filters import PairFilterIndex
from ..trainer import RELATION_TERM, fit_modes, refuse_modes
from . import loss_functions
from .negatives import check_datasets, known_index


class RelationPrediction:
    """weight: finite, >= 0 (0: the term is compiled and bound, and does nothing).
    loss: a name of loss_functions.LOSS_REGISTRY or a Loss object with an amdkge_loss descriptor (not BCELoss); `loss_params` its
    hyper-parameters when a name is given.
    known: which other relations of a positive's (s, o) pair are NOT competitors -- their scores are -inf before the loss:
      True   the relations the training set holds for the pair, the row's own among them (the loss compares the row's score with the
             relations NOT known for the pair; a pair for which every relation is known keeps its whole row),
      dict   the training set and these datasets (name -> triples, the form evaluate_relations(use_filter=...) takes),
      False  the row's own relation only.
    model.relation_prediction_stats_ = {"masked", "unmaskable"} after fit()."""

    def __init__(self, weight=1.0, loss="multiclass_nll", known=True, loss_params=None):
        if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not math.isfinite(float(weight)) \
                or float(weight) < 0.0:
            raise ValueError("relation_prediction: `weight` must be a finite number >= 0, got {!r}".format(weight))
        self.weight = float(weight)
        if not isinstance(loss, (str, loss_functions.Loss)):
            raise ValueError("relation_prediction: `loss` must be a loss name or a Loss object, got {!r}".format(loss))
        if isinstance(loss, str) and loss not in loss_functions.LOSS_REGISTRY:
            raise ValueError("relation_prediction: unknown loss {!r}; one of {}".format(loss, ", ".join(sorted(loss_functions.LOSS_REGISTRY))))
        self.loss = loss_functions.get(loss, loss_params)
        if getattr(self.loss, "labelled", False):
            raise ValueError("relation_prediction: BCELoss is the loss of KvsAll training over entities; a binary cross-entropy over "
                             "relations was not built")
        self.known = check_datasets(known, "known", who="relation_prediction")

    @classmethod
    def get(cls, spec):
        """None | RelationPrediction | its dict form {"weight", "loss", "loss_params", "known"} -> None | RelationPrediction"""
        if spec is None or isinstance(spec, cls):
            return spec
        if isinstance(spec, dict):
            unknown = set(spec) - {"weight", "loss", "loss_params", "known"}
            if unknown:
                raise ValueError("relation_prediction: unknown keys {}".format(sorted(unknown)))
            return cls(spec.get("weight", 1.0), spec.get("loss", "multiclass_nll"), spec.get("known", True), spec.get("loss_params"))
        raise ValueError("relation_prediction: expected None, a RelationPrediction or its dict form, got {!r}".format(spec))

    def get_config(self):
        """The dict form compile(relation_prediction=...) takes (datasets as given)."""
        return {"weight": self.weight, "loss": self.loss.name, "loss_params": dict(self.loss._loss_parameters), "known": self.known}

    def check_model(self, model, optimizer_mode="dense"):
        """compile()'s refusals: everything that is known before a GPU is touched."""
        if model.scoring_type not in ("DistMult", "ComplEx", "HolE"):
            raise NotImplementedError("relation_prediction: the term needs a score that is linear in the relation row (DistMult, ComplEx, "
                                      "HolE); {} scores a distance".format(model.scoring_type))
        refuse_modes(*RELATION_TERM, multi=model._dist() is not None, deterministic=model._deterministic, lazy=optimizer_mode == "lazy",
                     sharding=model._sharding)

    def bind(self, model, engine, train):
        refuse_modes(*RELATION_TERM, **fit_modes(model))
        index = known_index(model, engine, train, self.known, PairFilterIndex) if self.known is not False else None
        return BoundRelationPrediction(engine, self.weight, self.loss.to_ffi(), index)


class BoundRelationPrediction:
    """A RelationPrediction bound to one fit(): the PairFilterIndex over the training set (and `known`'s datasets), built on the device
    once; trainer.StepLoop.step calls step(batch), which looks the batch's pairs up (amdkge_pair_filter_ranges) and runs the term."""

    def __init__(self, engine, weight, loss_ffi, index):
        import torch

        self.engine, self.weight, self.loss_ffi, self.index = engine, float(weight), loss_ffi, index
        self.stats_dev = torch.zeros(2, dtype=torch.int64, device=engine.device)
        self._rows = None

    def ranges(self, batch):
        """(lo, hi, ids) of the batch's rows: the known relations of each pair, or -- known=False -- the row's own relation alone"""
        if self.index is not None:
            return self.index.device_filter(self.engine, batch)
        import torch

        B = int(batch.shape[0])
        if self._rows is None or int(self._rows.numel()) < B + 1:
            self._rows = torch.arange(B + 1, dtype=torch.int64, device=batch.device)
        return self._rows[:B], self._rows[1:B + 1], batch[:, 1].contiguous()

    def step(self, batch):
        if int(batch.shape[0]) == 0 or self.weight == 0.0:
            return
        self.engine.train_relation_fwdbwd(batch, self.loss_ffi, self.weight, flt=self.ranges(batch), stats=self.stats_dev)

    def stats(self):
        """{"masked", "unmaskable"} since the bind: one device read (synchronises the stream)."""
        mk, un = (int(v) for v in self.stats_dev.tolist())
        return {"masked": mk, "unmaskable": un}
