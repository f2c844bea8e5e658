"""Regulariser surface (/root/reference/ampligraph/latent_features/regularizers.py:14-73): LP with
keys `p` and `lambda` (defaults 2, 1e-5), the alias 'l3', and what tf.keras.regularizers.get accepts by name, which the
reference hands through (regularizers.py:59-73, EmbeddingLookupLayer.py:131-155): 'l1' / 'l2' (factor 0.01) and 'l1_l2'
(0.01 each) or its config dict {"class_name": "L1L2", "config": {"l1": ..., "l2": ...}}.  Every one of these is a sum of at
most two LP terms lambda * sum |x|^p over the WHOLE table; penalty and dense gradient are fused into the HIP optimizer sweep
(amdkge_opt.reg_p / reg_lambda / reg2_p / reg2_lambda).  The entity and the relation table take independent regularisers
(a [entity, relation] pair; either may be None).

BatchLPRegularizer is this engine's own addition: lambda * sum n^p over the rows of a step's POSITIVES, once per occurrence
(include/amdkge_batch_reg.h) -- the nuclear 3-norm N3 of Lacroix et al. 2018 with p = 3 on complex moduli, LibKGE's "weighted" Lp
on separate floats.  Identifiers 'N3' and 'batch_LP'; each member of the [entity, relation] pair is independently None, an
LPRegularizer (whole table, in the optimizer sweep) or a BatchLPRegularizer (amdkge_batch_reg_fwdbwd, between the backward
call and the sweep)."""


class LPRegularizer:
    """lambda * sum |x|^p  (+ a second term lambda2 * sum |x|^p2 for Keras' l1_l2)."""

    def __init__(self, p=2, lam=1e-5, p2=None, lam2=0.0):
        if int(p) < 1 or (p2 is not None and int(p2) < 1):
            raise ValueError("LP regularizer needs p >= 1")
        self.p, self.lam = int(p), float(lam)
        self.p2, self.lam2 = (int(p2) if p2 is not None else int(p)), float(lam2)

    @property
    def terms(self):
        """[(p, lambda), ...] with zero-weight terms dropped."""
        return [(p, lam) for p, lam in ((self.p, self.lam), (self.p2, self.lam2)) if lam != 0.0]

    def __call__(self, x):
        """The penalty of a table (numpy), as the Keras regulariser object would return it."""
        import numpy as np

        ax = np.abs(np.asarray(x, dtype=np.float64))
        return float(sum(lam * (ax ** p).sum() for p, lam in self.terms))


class BatchLPRegularizer:
    """lambda * sum_u n(row, u)^p over the entity / relation rows of a batch's positives, a row counted once per occurrence.
    p: 2 or 3.  norm: "float" (every float a unit, n = |x|), "modulus" (n = sqrt(re^2 + im^2) over the [re || im] halves:
    ComplEx / HolE rows, RotatE entity rows) or "auto": modulus where the model and the table allow it, float otherwise."""

    batch = True
    MODULUS_TABLES = {"ComplEx": ("ent", "rel"), "HolE": ("ent", "rel"), "RotatE": ("ent",)}

    def __init__(self, p=3, lam=1e-5, norm="auto"):
        if int(p) != p or int(p) not in (2, 3):
            raise ValueError("batch LP regularizer needs p = 2 or p = 3")
        if norm not in ("auto", "float", "modulus"):
            raise ValueError("batch LP regularizer: norm must be 'auto', 'float' or 'modulus'")
        if not float(lam) >= 0.0 or float(lam) == float("inf"):
            raise ValueError("batch LP regularizer needs a finite lambda >= 0")
        self.p, self.lam, self.norm = int(p), float(lam), norm

    def norm_for(self, scoring_type, table):
        """The norm mode ("float" | "modulus") this regulariser takes on `table` ("ent" | "rel") of a model; ValueError where
        "modulus" was asked for and the rows there hold no complex units."""
        ok = table in self.MODULUS_TABLES.get(scoring_type, ())
        if self.norm == "auto":
            return "modulus" if ok else "float"
        if self.norm == "modulus" and not ok:
            raise ValueError("batch LP regularizer: norm='modulus' is not offered for the {} table of {} ({})".format(
                {"ent": "entity", "rel": "relation"}[table], scoring_type,
                "a relation row holds phases, its modulus is 1" if scoring_type == "RotatE" else "its rows hold real units"))
        return self.norm

    def get_config(self):
        return {"kind": "batch", "p": self.p, "lambda": self.lam, "norm": self.norm}

    def __eq__(self, other):
        return isinstance(other, BatchLPRegularizer) and self.get_config() == other.get_config()

    __hash__ = None

    def __repr__(self):
        return "BatchLPRegularizer(p={}, lam={}, norm={!r})".format(self.p, self.lam, self.norm)


def is_batch(reg):
    return isinstance(reg, BatchLPRegularizer)


def to_config(reg):
    """A regulariser object (or None) -> the JSON form checkpoints carry; from_config reads it back.  The whole-table form has no
    "kind" field: what checkpoints held before the batch regularisers existed."""
    if reg is None:
        return None
    if is_batch(reg):
        return reg.get_config()
    return {"p": reg.p, "lambda": reg.lam, "p2": reg.p2, "lambda2": reg.lam2}


def from_config(cfg):
    if cfg is None:
        return None
    if cfg.get("kind", "table") == "batch":
        return BatchLPRegularizer(cfg.get("p", 3), cfg.get("lambda", 1e-5), cfg.get("norm", "auto"))
    return LPRegularizer(cfg.get("p", 2), cfg.get("lambda", 1e-5), cfg.get("p2"), cfg.get("lambda2", 0.0))


def _l1l2(l1, l2):
    l1, l2 = float(l1 or 0.0), float(l2 or 0.0)
    if l1 == 0.0 and l2 == 0.0:
        return None
    if l1 == 0.0:
        return LPRegularizer(2, l2)
    return LPRegularizer(1, l1, 2, l2)


def get(identifier, hyperparams=None):
    hyperparams = dict(hyperparams or {})
    if identifier is None:
        return None
    if isinstance(identifier, (LPRegularizer, BatchLPRegularizer)):
        return identifier
    if isinstance(identifier, dict):   # a Keras regulariser config
        name = str(identifier.get("class_name", "")).lower()
        cfg = dict(identifier.get("config", {}))
        if name in ("l1l2", "l1_l2"):
            return _l1l2(cfg.get("l1", 0.0), cfg.get("l2", 0.0))
        if name == "l1":
            return _l1l2(cfg.get("l1", 0.01), 0.0)
        if name == "l2":
            return _l1l2(0.0, cfg.get("l2", 0.01))
    if isinstance(identifier, str):
        if identifier == "l3":
            return LPRegularizer(3, hyperparams.get("lambda", 1e-5))
        if identifier == "N3":
            return BatchLPRegularizer(3, hyperparams.get("lambda", 1e-5), hyperparams.get("norm", "auto"))
        if identifier == "batch_LP":
            return BatchLPRegularizer(hyperparams.get("p", 3), hyperparams.get("lambda", 1e-5), hyperparams.get("norm", "auto"))
        if identifier == "LP":
            return LPRegularizer(hyperparams.get("p", 2), hyperparams.get("lambda", 1e-5))
        if identifier.lower() == "l1":
            return LPRegularizer(1, 0.01)   # tf.keras.regularizers.L1 default
        if identifier.lower() == "l2":
            return LPRegularizer(2, 0.01)   # tf.keras.regularizers.L2 default
        if identifier.lower() == "l1_l2":
            return _l1l2(0.01, 0.01)        # tf.keras.regularizers.l1_l2 defaults
    raise ValueError(f"Could not interpret regularizer identifier: {identifier!r}")
