"""What trainer.StepLoop.step calls, for every kind of negative setting with and without the relation term and a batch regulariser,
and what each of the three features that own part of the step (shared negatives, batch regulariser, relation term) refuses at compile,
bind / fit and step time.  No GPU and no built library: a recording engine answers the bind-time lookups from host-built indexes
(tests/test_host_data.py has the precedent) and writes every call of a step down; the samplers and the term are the real objects,
made the public way: X.get(spec).bind(model, engine, train).

12 training rows, batches of 6 (the second one does not start at row 0 of the training tensor: a wrong slice shows), groups of 4
(the last one partial), 5 entities, 2 relations."""
import numpy as np
import pytest
import torch

from ampligraph_amd import _ffi
from ampligraph_amd.datasets.filters import FilterIndex, PairFilterIndex
from ampligraph_amd.datasets.types import sets_csr
from ampligraph_amd.latent_features import BCELoss, KvsAll, ScoringBasedEmbeddingModel
from ampligraph_amd.latent_features.negatives import NegativeSampling, TypedNegatives
from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer, LPRegularizer
from ampligraph_amd.latent_features.relation_prediction import RelationPrediction
from ampligraph_amd.trainer import StepLoop

N, R, B, G, ETA, SEED = 5, 2, 6, 4, 2, 5
TRAIN = np.array([[0, 0, 1], [1, 0, 2], [2, 1, 3], [3, 1, 4], [4, 0, 0], [0, 1, 2], [1, 1, 3], [2, 0, 4], [3, 0, 0], [4, 1, 1], [0, 0, 3], [1, 1, 4]],
                 dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the recording engine
def _ranges(keys, start, q):
    k, s = keys.numpy(), start.numpy()
    pos = np.minimum(np.searchsorted(k, q), max(0, k.size - 1))
    hit = (k[pos] == q) if k.size else np.zeros(len(q), bool)
    return torch.as_tensor(np.where(hit, s[pos], 0)), torch.as_tensor(np.where(hit, s[np.minimum(pos + 1, s.size - 1)], 0))


class RecordingEngine:
    """The surface the samplers, the relation term and StepLoop use on one rank.  Every call is written down as (method, arguments,
    keywords) with the arguments described by `show`: a tensor the engine knows by name -- the training tensor, what it returned at
    bind time or in this step -- as "name" or "name[r0:r1]" (its rows), any other tensor as (dtype, shape), a descriptor by its
    class, scalars as they are."""
    device = torch.device("cpu")

    def __init__(self, scoring_type):
        self.scoring_type, self.k = scoring_type, 8
        self.calls, self._names, self._alive = [], {}, []

    def name(self, obj, name):
        """`obj` (a tensor: its storage; anything else: the object) is shown as `name` from now on"""
        self._alive.append(obj)
        self._names[obj.untyped_storage().data_ptr() if isinstance(obj, torch.Tensor) else id(obj)] = (name, obj)
        return obj

    def show(self, a):
        if isinstance(a, torch.Tensor):
            known = self._names.get(a.untyped_storage().data_ptr()) if a.numel() else None
            if known is None:
                return (str(a.dtype).replace("torch.", ""), tuple(a.shape))
            name, whole = known
            row = max(1, int(np.prod(whole.shape[1:])))
            r0 = a.storage_offset() // row
            return name if tuple(a.shape) == tuple(whole.shape) else "{}[{}:{}]".format(name, r0, r0 + int(a.shape[0]))
        if isinstance(a, (tuple, list)):
            return tuple(self.show(v) for v in a)
        if id(a) in self._names:
            return self._names[id(a)][0]
        if isinstance(a, _ffi.Opt):
            return ("Opt", int(a.iteration))
        if isinstance(a, (BatchLPRegularizer, LPRegularizer, _ffi.Loss)):
            return type(a).__name__
        assert a is None or isinstance(a, (bool, int, float, str)), a
        return a

    def _record(self, method, *args, **kw):
        self.calls.append((method, tuple(self.show(a) for a in args), {k: self.show(v) for k, v in kw.items()}))

    # ---- bind-time lookups, answered on the host
    def prepare_training(self, name):
        pass

    def filter_build(self, X, form, n_ents, n_rels):
        fi = FilterIndex([X.numpy()], n_ents, n_rels)
        keys, start, ids = (torch.as_tensor(getattr(fi, nm)) for nm in FilterIndex._FORMS[form])
        return keys, start, self.name(ids, form + ".ids")

    def filter_ranges(self, keys, start, triples, side, n_ents, n_rels):
        t = triples.numpy().astype(np.int64)
        lo, hi = _ranges(keys, start, t[:, 1] * n_ents + t[:, 2] if side == 1 else t[:, 0] * n_rels + t[:, 1])
        sd = "s" if side == 1 else "o"
        return self.name(lo, sd + ".lo"), self.name(hi, sd + ".hi")

    def pair_filter_build(self, X, n_ents, n_rels):
        fi = PairFilterIndex([X.numpy()], n_ents, n_rels)
        keys, start, ids = (torch.as_tensor(getattr(fi, nm)) for nm in PairFilterIndex._FORMS["pair"])
        return self.name(keys, "pair.keys"), self.name(start, "pair.start"), self.name(ids, "pair.ids")

    def pair_filter_ranges(self, keys, start, triples, n_ents):
        self._record("pair_filter_ranges", keys, start, triples, n_ents)
        t = triples.numpy().astype(np.int64)
        lo, hi = _ranges(keys, start, t[:, 0] * n_ents + t[:, 2])
        return self.name(lo, "pair.lo"), self.name(hi, "pair.hi")

    def relation_sets_build(self, X, side, n_ents, n_rels):
        keys, start, ids = (torch.as_tensor(a) for a in sets_csr(X.numpy(), side))
        return self.name(keys, side + ".sets"), start, ids

    def relation_sets_ranges(self, keys, start, triples, min_size=0, fallback=(0, 0)):
        sd = self.show(keys)[0]
        n = int(triples.shape[0])
        return self.name(torch.zeros(n, dtype=torch.int64), sd + ".cand.lo"), self.name(torch.ones(n, dtype=torch.int64), sd + ".cand.hi")

    def negatives_side_thresholds(self, po_keys, sp_keys, n_ents=None, n_rels=None):
        return self.name(torch.zeros(int(n_rels), dtype=torch.int32), "thr")

    # ---- the calls of a step
    def tiled_supported(self, B, eta):
        self._record("tiled_supported", B, eta)
        return True

    def sample_shared(self, triples, group_size, num_negs, seed, step, **kw):
        self._record("sample_shared", triples, group_size, num_negs, seed, step, **kw)
        n = int(triples.shape[0])
        return (self.name(torch.zeros(-(-n // min(group_size, n)), num_negs, dtype=torch.int32), "ids"),
                self.name(torch.zeros(n, dtype=torch.int32), "side"))

    def sample_negatives(self, triples, eta, seed, step, **kw):
        self._record("sample_negatives", triples, eta, seed, step, **kw)
        return self.name(torch.zeros(int(triples.shape[0]) * eta, 3, dtype=torch.int32), "neg")

    def sample_negatives_typed(self, triples, eta, seed, step, **kw):
        self._record("sample_negatives_typed", triples, eta, seed, step, **kw)
        return self.name(torch.zeros(int(triples.shape[0]) * eta, 3, dtype=torch.int32), "neg")

    def __getattr__(self, method):
        if method not in ("train_fwdbwd", "train_step_tiled", "train_shared_fwdbwd", "train_shared_masked_fwdbwd", "train_shared_dist_fwdbwd",
                          "train_shared_labels_fwdbwd", "train_shared_dist_labels_fwdbwd", "train_relation_fwdbwd", "batch_reg_fwdbwd", "opt_step"):
            raise AttributeError(method)
        return lambda *args, **kw: self._record(method, *args, **kw)


def _setup(scoring, loss, negatives, relation, n3, monkeypatch, path="atomic", **opt_kw):
    """compile() the settings on a real model (so only what compile accepts is run), bind them the way fit() does -> loop, engine, train"""
    monkeypatch.setenv("AMDKGE_TRAIN_PATH", path)
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    monkeypatch.delenv("AMDKGE_FORCE_DIST", raising=False)
    m = ScoringBasedEmbeddingModel(eta=ETA, k=4, scoring_type=scoring, seed=SEED)
    m.compile(optimizer="sgd", loss=loss, negatives=negatives, relation_prediction=RelationPrediction(0.25) if relation else None,
              entity_relation_regularizer=BatchLPRegularizer(3, 0.25) if n3 else None)
    m.optimizer.lazy = bool(opt_kw.get("lazy", False))
    m._n_ents, m._n_rels = N, R
    eng = RecordingEngine(scoring)
    loop = StepLoop(eng, m.eta, m.loss, m.optimizer, m._regularizers[0], m.seed, None)
    loop.reg_rel = m._regularizers[1]
    train = eng.name(torch.as_tensor(TRAIN), "train")
    loop.negatives = None if m._negatives is None else m._negatives.bind(m, eng, train)
    loop.relation = None if m._relation_prediction is None else m._relation_prediction.bind(m, eng, train)
    if loop.loss_ffi is not None:
        eng.name(loop.loss_ffi, "loss")
    if loop.relation is not None:
        eng.name(loop.relation.loss_ffi, "relation loss")
    del eng.calls[:]
    return loop, eng, train


# ------------------------------------------------------------------------------------------------ 1. the calls of a step
# Every row: (name, model, loss, compile(negatives=...), AMDKGE_TRAIN_PATH, main), main(a, b, step, it, dense) being the literal
# calls of the backward stage for the batch train[a:b] drawn at `step` in optimizer iteration `it`; dense: the relation term or a
# batch regulariser is on (the per-corruption step then leaves the owner-computes path).  ROWS / STATS name bound tensors the engine
# did not hand out.
def _filters(a, b):
    return dict(s_filter=(f"s.lo[{a}:{b}]", f"s.hi[{a}:{b}]", "s.ids"), o_filter=(f"o.lo[{a}:{b}]", f"o.hi[{a}:{b}]", "o.ids"))


STATS2, STATS3, ALL_IDS = ("int64", (2,)), ("int64", (3,)), ("int32", (2, N))


def _atomic(a, b, step, it, dense, **override):
    return [("train_fwdbwd", (f"train[{a}:{b}]", ETA, "loss", SEED, step), dict(row_offset=0, b_global=B, **override))]


def _tiled(a, b, step, it, dense, **override):
    if dense:
        return _atomic(a, b, step, it, dense, **override)
    return [("tiled_supported", (B, ETA), {}),
            ("train_step_tiled", (f"train[{a}:{b}]", ETA, "loss", ("Opt", it), SEED, step),
             dict(reg_e=None, reg_r=None, row_offset=0, b_global=B, grad_only=False, pos_atomic=False, **override))]


def _filtered(a, b, step, it, dense):
    draw = ("sample_negatives", (f"train[{a}:{b}]", ETA, SEED, step),
            dict(row_offset=0, b_global=B, side="uniform", side_thr=None, pool=None, max_tries=8, stats=STATS2, **_filters(a, b)))
    if dense:
        return [draw] + _atomic(a, b, step, it, dense, neg_override="neg")
    return [("tiled_supported", (B, ETA), {}), draw] + _tiled(a, b, step, it, dense, neg_override="neg")[1:]


def _typed(a, b, step, it, dense):
    return [("sample_negatives_typed", (f"train[{a}:{b}]", ETA, SEED, step),
             dict(s_cand=(f"s.cand.lo[{a}:{b}]", f"s.cand.hi[{a}:{b}]", ("int32", (10 + N,))), o_cand=(f"o.cand.lo[{a}:{b}]", f"o.cand.hi[{a}:{b}]", ("int32", (9 + N,))),
                  row_offset=0, b_global=B, side="uniform", side_thr=None, pool=None, s_filter=None, o_filter=None, max_tries=8, stats=STATS3))
            ] + _atomic(a, b, step, it, dense, neg_override="neg")


def _draw(a, b, step, M=6, **kw):
    return ("sample_shared", (f"train[{a}:{b}]", G, M, SEED, step), dict(dict(side="uniform", side_thr=None, pool=None), **kw))


def _draw_sides(a, b, step):   # the all-entities list: only the sides are drawn (one id per group, dropped)
    return ("sample_shared", (f"train[{a}:{b}]", G, 1, SEED, step), dict(side="uniform", side_thr=None))


def _shared(a, b, step, it, dense):
    return [_draw(a, b, step), ("train_shared_fwdbwd", (f"train[{a}:{b}]", G, 6, "ids", "side", "loss"), {})]


def _shared_bernoulli(a, b, step, it, dense):
    return [_draw(a, b, step, side="bernoulli", side_thr="thr"), ("train_shared_fwdbwd", (f"train[{a}:{b}]", G, 6, "ids", "side", "loss"), {})]


def _masked(a, b, step, it, dense):
    return [_draw(a, b, step), ("train_shared_masked_fwdbwd", (f"train[{a}:{b}]", G, 6, "ids", "side", "loss"), dict(_filters(a, b), identity=False, stats=STATS2))]


def _masked_all(a, b, step, it, dense):
    return [_draw_sides(a, b, step),
            ("train_shared_masked_fwdbwd", (f"train[{a}:{b}]", G, N, ALL_IDS, "side", "loss"), dict(_filters(a, b), identity=True, stats=STATS2))]


def _dist(a, b, step, it, dense):
    return [_draw(a, b, step), ("train_shared_dist_fwdbwd", (f"train[{a}:{b}]", G, 6, "ids", "side", "loss"), {})]


def _dist_masked_all(a, b, step, it, dense):
    return [_draw_sides(a, b, step),
            ("train_shared_dist_fwdbwd", (f"train[{a}:{b}]", G, N, ALL_IDS, "side", "loss"), dict(_filters(a, b), identity=True, stats=STATS2))]


def _kvsall(a, b, step, it, dense):
    f = _filters(a, b)
    return [_draw_sides(a, b, step),
            ("train_shared_labels_fwdbwd", (f"train[{a}:{b}]", G, N, ALL_IDS, "side", f["s_filter"], f["o_filter"]),
             dict(label_smoothing=0.1, reduction="mean", weights=None, identity=True, stats=STATS2))]


def _kvsall_query(a, b, step, it, dense):
    f = _filters(a, b)
    return [_draw_sides(a, b, step),
            ("train_shared_dist_labels_fwdbwd", (f"train[{a}:{b}]", G, N, ALL_IDS, "side", f["s_filter"], f["o_filter"]),
             dict(label_smoothing=0.1, reduction="mean", weights=(("float32", (b - a,)), ("float32", (b - a,))), identity=True, stats=STATS2))]


BCE = {"label_smoothing": 0.1, "reduction": "mean"}
ROWS = [
    ("no sampler, atomic", "ComplEx", "nll", None, "atomic", _atomic),
    ("no sampler, tiled", "ComplEx", "nll", None, "tiled", _tiled),
    ("filtered", "ComplEx", "nll", lambda: NegativeSampling(filter=True), "tiled", _filtered),
    ("typed", "ComplEx", "nll", lambda: TypedNegatives("observed"), "atomic", _typed),
    ("shared", "ComplEx", "nll", lambda: {"shared": 6, "group_size": G}, "tiled", _shared),
    ("shared bernoulli", "ComplEx", "nll", lambda: {"shared": 6, "group_size": G, "side": "bernoulli"}, "tiled", _shared_bernoulli),
    ("shared masked", "ComplEx", "nll", lambda: {"shared": 6, "group_size": G, "mask_known": True}, "tiled", _masked),
    ("shared masked identity", "ComplEx", "nll", lambda: {"shared": "all", "group_size": G, "mask_known": True}, "tiled", _masked_all),
    ("distance", "TransE", "nll", lambda: {"shared_distance": 6, "group_size": G}, "tiled", _dist),
    ("distance masked identity", "TransE", "nll", lambda: {"shared_distance": "all", "group_size": G, "mask_known": True}, "tiled", _dist_masked_all),
    ("KvsAll", "ComplEx", lambda: BCELoss(BCE), lambda: KvsAll(group_size=G), "tiled", _kvsall),
    ("KvsAll query", "TransE", lambda: BCELoss(BCE), lambda: KvsAll(weight="query", group_size=G), "tiled", _kvsall_query),
]


def _extras(a, b, relation, n3, it):
    """the dense extras between the backward call and the sweep, then the sweep: the batch regulariser is not the sweep's"""
    out = []
    if relation:
        out += [("pair_filter_ranges", ("pair.keys", "pair.start", f"train[{a}:{b}]", N), {}),
                ("train_relation_fwdbwd", (f"train[{a}:{b}]", "relation loss", 0.25), dict(flt=("pair.lo", "pair.hi", "pair.ids"), stats=STATS2))]
    if n3:
        out += [("batch_reg_fwdbwd", (f"train[{a}:{b}]", "BatchLPRegularizer", "BatchLPRegularizer"), {})]
    return out


@pytest.mark.parametrize("n3", [False, True], ids=["", "N3"])
@pytest.mark.parametrize("relation", [False, True], ids=["", "relation"])
@pytest.mark.parametrize("name,scoring,loss,negatives,path,main", ROWS, ids=[r[0] for r in ROWS])
def test_the_calls_of_a_step(monkeypatch, name, scoring, loss, negatives, path, main, relation, n3):
    if relation and scoring == "TransE":
        with pytest.raises(NotImplementedError, match="linear in the relation row"):   # compile does not accept the combination
            _setup(scoring, loss if isinstance(loss, str) else loss(), negatives and negatives(), relation, n3, monkeypatch, path)
        return
    loop, eng, train = _setup(scoring, loss if isinstance(loss, str) else loss(), negatives and negatives(), relation, n3, monkeypatch, path)
    hooks = []
    loop.kernel_hook = lambda i: hooks.append((i, len(eng.calls)))
    for it, (a, b, step) in enumerate(((0, 6, 7), (6, 12, 8)), start=1):
        del eng.calls[:], hooks[:]
        loop.step(train[a:b], step)
        dense = relation or n3
        want = main(a, b, step, it, dense) + _extras(a, b, relation, n3, it)
        whole_step = main is _tiled and not dense or main is _filtered and not dense   # the owner-computes call is the complete step
        if not whole_step:
            want += [("opt_step", (("Opt", it), None, None), {})]
        assert eng.calls == want
        # hook 0 after the path is chosen and before the first draw, hook 1 before the sweep, hook 2 after it
        first = 1 if want[0][0] == "tiled_supported" else 0
        assert hooks == [(0, first), (1, len(want) - (0 if whole_step else 1)), (2, len(want))]
        assert loop.n_steps == it and loop.optimizer.iterations == it


def test_an_empty_batch_still_sweeps(monkeypatch):
    for row in (ROWS[0], ROWS[4]):
        loop, eng, train = _setup(row[1], row[2], row[3] and row[3](), True, True, monkeypatch, row[4])
        loop.step(train[0:0], 3)
        assert eng.calls == [("opt_step", (("Opt", 1), None, None), {})] and loop.n_steps == 1


# ------------------------------------------------------------------------------------------------ 2. the refusals
# feature -> stage -> mode -> refused?  A refusal is a NotImplementedError whose head (the text before the first colon) names the
# feature and whose text holds the mode's keyword; a mode a stage cannot see has no cell.
KEYWORD = {"FocusE": ("FocusE",), "ranks": ("one rank",), "deterministic": ("deterministic",), "lazy": ("lazy",),
           "rows": ("sharded", "entity_sharding"), "columns": ("sharded", "entity_sharding")}
REFUSED = {
    "negatives": {"compile": dict(ranks=False, deterministic=True, lazy=True, rows=True, columns=True),
                  "bind": dict(FocusE=True, ranks=True, deterministic=True),
                  "step": dict(FocusE=True, ranks=True, deterministic=True, lazy=False)},
    "batch regularizer": {"compile": dict(ranks=False, deterministic=True, lazy=True, rows=True, columns=True),
                          "bind": dict(FocusE=True, ranks=True, deterministic=True),
                          "step": dict(FocusE=True, ranks=True, deterministic=True, lazy=True)},
    "relation_prediction": {"compile": dict(ranks=True, deterministic=True, lazy=True, rows=True, columns=True),
                            "bind": dict(FocusE=True, ranks=True, deterministic=True),
                            "step": dict(FocusE=True, ranks=True, deterministic=True, lazy=True)},
}
SETTING = {"negatives": dict(negatives={"shared": 6, "group_size": G}), "batch regularizer": dict(entity_relation_regularizer="N3"),
           "relation_prediction": dict(relation_prediction={"weight": 0.25})}
CELLS = [(f, stage, mode, refused) for f, stages in REFUSED.items() for stage, modes in stages.items() for mode, refused in modes.items()]


class _TwoRanks:
    def get_world_size(self):
        return 2

    def get_rank(self):
        return 0


class _Reached(Exception):
    """fit() got past its refusals"""


def _compile(feature, mode):
    m = ScoringBasedEmbeddingModel(eta=ETA, k=4, scoring_type="ComplEx", seed=SEED)
    if mode == "ranks":
        m._dist_override = _TwoRanks()
    kw = {"deterministic": dict(deterministic=True), "lazy": dict(optimizer_mode="lazy"), "rows": dict(entity_sharding="rows"),
          "columns": dict(entity_sharding="columns")}.get(mode, {})
    m.compile(optimizer="sgd", loss="nll", **SETTING[feature], **kw)
    return m


def _bind(feature, mode):
    """the stage at which fit() has a loop and knows whether FocusE is on: bind() for the sampler and the term, fit() itself for the
    batch regulariser (run here up to the first call past its refusals, on a placement that hands out the loop below)"""
    class Loop:
        multi, deterministic = mode == "ranks", mode == "deterministic"

    m = _compile(feature, None)
    if feature == "batch regularizer":
        class Placement:
            engine = None

            def make_loop(self):
                return Loop()

            def begin_fit(self, has_callbacks):
                raise _Reached

        m._build = lambda *a, **kw: setattr(m, "_placement", Placement())
        X = np.concatenate([TRAIN.astype(str).astype(object), np.ones((12, 1), dtype=object)], 1)
        with pytest.raises(_Reached):
            m.fit(X if mode == "FocusE" else X[:, :3], batch_size=B, epochs=1, focusE=mode == "FocusE")
        return
    m._n_ents, m._n_rels, m._loop, m.use_focusE = N, R, Loop(), mode == "FocusE"
    eng = RecordingEngine("ComplEx")
    (m._negatives if feature == "negatives" else m._relation_prediction).bind(m, eng, torch.as_tensor(TRAIN))


def _step(feature, mode, monkeypatch):
    """-> loop, engine, run: run() is one step under `mode`, with the FocusE fields of the loss descriptor set to marks beforehand"""
    s = SETTING[feature]
    loop, eng, train = _setup("ComplEx", "nll", s.get("negatives"), "relation_prediction" in s, "entity_relation_regularizer" in s, monkeypatch,
                              lazy=mode == "lazy")
    loop.multi, loop.deterministic = mode == "ranks", mode == "deterministic"
    loop.loss_ffi.focus_nonlinearity, loop.loss_ffi.d_focus_w = 2, 4096
    return loop, eng, lambda: loop.step(train[0:6], 7, focus=(torch.ones(6), 0.5, "linear") if mode == "FocusE" else None)


@pytest.mark.parametrize("feature,stage,mode,refused", CELLS, ids=["{}-{}-{}".format(*c[:3]) for c in CELLS])
def test_refusal_table(monkeypatch, feature, stage, mode, refused):
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    run = {"compile": lambda: _compile(feature, mode), "bind": lambda: _bind(feature, mode), "step": lambda: _step(feature, mode, monkeypatch)[2]()}[stage]
    if not refused:
        run()
        return
    with pytest.raises(NotImplementedError) as e:
        run()
    text = str(e.value)
    assert text.split(":")[0].endswith(feature) and any(word in text for word in KEYWORD[mode]), text


@pytest.mark.parametrize("feature,mode", [(f, m) for f, stage, m, refused in CELLS if stage == "step" and refused])
def test_a_refused_step_touches_nothing(monkeypatch, feature, mode):
    """the optimizer's clock (and with it the RNG base of the next fit()), the loop's step count, the FocusE fields of the loss
    descriptor and the engine are what they were"""
    loop, eng, run = _step(feature, mode, monkeypatch)
    with pytest.raises(NotImplementedError):
        run()
    assert (loop.optimizer.iterations, loop.n_steps, loop.loss_ffi.focus_nonlinearity, loop.loss_ffi.d_focus_w, eng.calls) == (0, 0, 2, 4096, [])
