"""optimizer_mode="sparse" without a GPU: what compile() accepts and refuses, what bind and step refuse, the config and save round
trip, the literal calls of a step on the recording engine of tests/test_step_calls_host.py (the sampler's step, the relation term,
the batch regulariser, then opt_step_rows on the sampler's candidate rows -- and no opt_step), and the numpy restatement
tests/sparse_ref.py against the oracle's whole-table lazy sweep."""
import json

import numpy as np
import pytest
import torch

import sparse_ref as SR
import test_step_calls_host as S
from ampligraph_amd.latent_features import BCELoss, KvsAll, ScoringBasedEmbeddingModel, optimizers
from ampligraph_amd.latent_features.negatives import BoundSharedNegatives, NegativeSampling, SharedDistanceNegatives, SharedNegatives
from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer
from ampligraph_amd.latent_features.relation_prediction import RelationPrediction
from ampligraph_amd.trainer import StepLoop
from oracle import kge_oracle as O

N, R, B, G, ETA, SEED, TRAIN = S.N, S.R, S.B, S.G, S.ETA, S.SEED, S.TRAIN


def _model(scoring="ComplEx", loss="nll", **kw):
    m = ScoringBasedEmbeddingModel(eta=ETA, k=4, scoring_type=scoring, seed=SEED)
    m.compile(optimizer=kw.pop("optimizer", "adam"), loss=loss, **kw)
    return m


# ------------------------------------------------------------------------------------------------ 1. compile
FORMS = [("ComplEx", lambda **kw: SharedNegatives(8, **kw)), ("ComplEx", lambda **kw: SharedNegatives(8, mask_known=True, **kw)),
         ("TransE", lambda **kw: SharedDistanceNegatives(8, **kw)), ("RotatE", lambda **kw: SharedDistanceNegatives(8, mask_known=True, **kw))]


@pytest.mark.parametrize("pool", [None, ["a", "b", "c"]], ids=["", "pool"])
@pytest.mark.parametrize("scoring,make", FORMS, ids=["shared", "masked", "distance", "distance masked"])
def test_compile_accepts_the_samplers_that_draw_finite_lists(scoring, make, pool):
    m = _model(scoring, negatives=make(entities=pool), optimizer_mode="sparse")
    assert m.optimizer.sparse is True and m.optimizer.lazy is False and m.optimizer.to_ffi(1).lazy == 0
    if pool is not None:   # the list that is the pool
        cls = type(make())
        m = _model(scoring, negatives=cls("all", entities=pool, mask_known=make().mask_known), optimizer_mode="sparse")
        assert m.optimizer.sparse is True
    # the dict form, and the mode is per compile(): the next one is dense again
    key = "shared_distance" if scoring in ("TransE", "RotatE") else "shared"
    assert _model(scoring, negatives={key: 8, "entities": pool}, optimizer_mode="sparse").optimizer.sparse is True
    m.compile(optimizer="adam", loss="nll", negatives=make(entities=pool))
    assert m.optimizer.sparse is False


def test_other_modes_are_what_they_were():
    assert _model().optimizer.sparse is False and _model(optimizer_mode="lazy").optimizer.sparse is False
    with pytest.raises(ValueError, match="optimizer_mode"):
        _model(optimizer_mode="sparser")
    for neg in ({"shared": 8}, {"shared": 8, "mask_known": True}):   # the touched-rows mode stays refused with a sampler that owns its step
        with pytest.raises(NotImplementedError, match="lazy"):
            _model(negatives=neg, optimizer_mode="lazy")
    with pytest.raises(NotImplementedError, match="lazy"):
        _model("TransE", negatives={"shared_distance": 8}, optimizer_mode="lazy")


# feature -> what compile(optimizer_mode="sparse", ...) is given -> the keywords of its refusal (None: accepted)
COMPILE = [
    ("no sampler", dict(), ("sparse", "names no rows", "optimizer_mode='lazy'")),
    ("override sampler", dict(negatives=NegativeSampling(filter=True)), ("sparse", "names no rows", "optimizer_mode='lazy'")),
    ("typed sampler", dict(negatives={"types": "observed"}), ("sparse", "names no rows")),
    ("identity list", dict(negatives={"shared": "all"}), ("sparse", "every row is a candidate")),
    ("identity list masked", dict(negatives={"shared": "all", "mask_known": True}), ("sparse", "every row is a candidate")),
    ("KvsAll", dict(negatives=KvsAll(), loss=BCELoss()), ("sparse", "every row is a candidate")),
    ("deterministic", dict(negatives={"shared": 8}, deterministic=True), ("negatives", "deterministic")),
    ("rows", dict(negatives={"shared": 8}, entity_sharding="rows"), ("negatives", "entity_sharding")),
    ("columns", dict(negatives={"shared": 8}, entity_sharding="columns"), ("negatives", "entity_sharding")),
    ("no sampler, rows", dict(entity_sharding="rows"), ("sparse", "names no rows")),
    ("relation term", dict(negatives={"shared": 8}, relation_prediction={"weight": 0.25}), None),
    ("N3", dict(negatives={"shared": 8}, entity_relation_regularizer="N3"), None),
    ("LP", dict(negatives={"shared": 8}, entity_relation_regularizer="l2"), None),
]


@pytest.mark.parametrize("name,kw,words", COMPILE, ids=[c[0] for c in COMPILE])
def test_compile_refusals(name, kw, words):
    kw = dict(kw)
    if words is None:
        assert _model(optimizer_mode="sparse", **kw).optimizer.sparse is True
        return
    with pytest.raises(NotImplementedError) as e:
        _model(optimizer_mode="sparse", **kw)
    assert all(w in str(e.value) for w in words), str(e.value)


# ------------------------------------------------------------------------------------------------ 2. the calls of a step
class Engine(S.RecordingEngine):
    """the recording engine with the two calls of the mode"""

    def step_rows(self, triples, ids):
        self._record("step_rows", triples, ids)
        cap = min(2 * int(triples.shape[0]) + (0 if ids is None else int(ids.numel())), N)
        return self.name(torch.zeros(max(cap, 1), dtype=torch.int32)[:cap], "rows"), self.name(torch.zeros(1, dtype=torch.int64), "n_rows")

    def opt_step_rows(self, *args, **kw):
        self._record("opt_step_rows", *args, **kw)


def _setup(scoring, negatives, relation, n3, monkeypatch, sparse=True):
    """S._setup with optimizer_mode="sparse" and the engine above"""
    monkeypatch.setenv("AMDKGE_TRAIN_PATH", "tiled")
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    monkeypatch.delenv("AMDKGE_FORCE_DIST", raising=False)
    m = ScoringBasedEmbeddingModel(eta=ETA, k=4, scoring_type=scoring, seed=SEED)
    m.compile(optimizer="sgd", loss="nll", negatives=negatives, relation_prediction=RelationPrediction(0.25) if relation else None,
              entity_relation_regularizer=BatchLPRegularizer(3, 0.25) if n3 else None, **({"optimizer_mode": "sparse"} if sparse else {}))
    m._n_ents, m._n_rels = N, R
    eng = Engine(scoring)
    loop = StepLoop(eng, m.eta, m.loss, m.optimizer, m._regularizers[0], m.seed, None)
    loop.reg_rel = m._regularizers[1]
    train = eng.name(torch.as_tensor(TRAIN), "train")
    loop.negatives = None if m._negatives is None else m._negatives.bind(m, eng, train)
    loop.relation = None if m._relation_prediction is None else m._relation_prediction.bind(m, eng, train)
    eng.name(loop.loss_ffi, "loss")
    if loop.relation is not None:
        eng.name(loop.relation.loss_ffi, "relation loss")
    del eng.calls[:]
    return loop, eng, train


SAMPLERS = [("shared", "ComplEx", {"shared": 6, "group_size": G}, S._shared), ("masked", "ComplEx", {"shared": 6, "group_size": G, "mask_known": True}, S._masked),
            ("distance", "TransE", {"shared_distance": 6, "group_size": G}, S._dist)]


@pytest.mark.parametrize("extra", ["", "relation", "N3"])
@pytest.mark.parametrize("name,scoring,negatives,main", SAMPLERS, ids=[r[0] for r in SAMPLERS])
def test_the_calls_of_a_sparse_step(monkeypatch, name, scoring, negatives, main, extra):
    relation, n3 = extra == "relation", extra == "N3"
    if relation and scoring == "TransE":
        with pytest.raises(NotImplementedError, match="linear in the relation row"):   # compile does not accept the combination in any mode
            _setup(scoring, negatives, relation, n3, monkeypatch)
        return
    loop, eng, train = _setup(scoring, negatives, relation, n3, monkeypatch)
    hooks = []
    loop.kernel_hook = lambda i: hooks.append((i, len(eng.calls)))
    for it, (a, b, step) in enumerate(((0, 6, 7), (6, 12, 8)), start=1):
        del eng.calls[:], hooks[:]
        loop.step(train[a:b], step)
        want = main(a, b, step, it, relation or n3) + S._extras(a, b, relation, n3, it)
        want += [("step_rows", (f"train[{a}:{b}]", "ids"), {}), ("opt_step_rows", (("Opt", it), None, None, "rows", "n_rows", N), {})]
        assert eng.calls == want and not [c for c in eng.calls if c[0] == "opt_step"]
        assert hooks == [(0, 0), (1, len(want) - 2), (2, len(want))]
        assert loop.n_steps == it and loop.optimizer.iterations == it
    # the same loop in dense mode ends in opt_step and never asks for rows
    loop, eng, train = _setup(scoring, negatives, relation, n3, monkeypatch, sparse=False)
    loop.step(train[0:6], 7)
    assert eng.calls[-1] == ("opt_step", (("Opt", 1), None, None), {}) and not [c for c in eng.calls if c[0] in ("step_rows", "opt_step_rows")]


def test_an_empty_batch_sweeps_no_rows(monkeypatch):
    loop, eng, train = _setup("ComplEx", {"shared": 6, "group_size": G}, True, True, monkeypatch)
    loop.step(train[0:6], 3)
    del eng.calls[:]
    loop.step(train[0:0], 4)      # no draw, no backward call: the ids of the step before are not candidates of this one
    assert eng.calls == [("step_rows", (("int32", (0, 3)), None), {}), ("opt_step_rows", (("Opt", 2), None, None, ("int32", (0,)), "n_rows", 0), {})]


class _Draws:
    """what BoundSharedNegatives asks of an engine, recorded"""
    device = torch.device("cpu")

    def __init__(self):
        self.asked = []

    def sample_shared(self, triples, group_size, num_negs, seed, step, **kw):
        n = int(triples.shape[0])
        self.ids = torch.arange(-(-n // min(group_size, n)) * num_negs, dtype=torch.int32).reshape(-1, num_negs)
        return self.ids, torch.zeros(n, dtype=torch.int32)

    def step_rows(self, triples, ids):
        self.asked.append((triples, ids))
        return "rows", "n"

    def train_shared_fwdbwd(self, *a, **kw):
        pass


def test_candidate_rows_are_the_rows_of_the_step_just_run():
    X = torch.as_tensor(TRAIN)
    eng = _Draws()
    drawn = BoundSharedNegatives(eng, 6, G, "uniform", None, None)
    assert drawn.names_rows
    drawn.step(X[:6], None, SEED, 1)
    assert drawn.candidate_rows(X[:6]) == ("rows", "n") and eng.asked[-1][1] is eng.ids          # the ids drawn, not drawn twice
    # a list every group shares (num_negs="all" over a pool): one copy of it, not the [n_groups, M] tensor
    pool = torch.tensor([4, 1, 3], dtype=torch.int32)
    shared = BoundSharedNegatives(eng, 3, G, "uniform", None, pool, all_list=pool)
    assert shared.names_rows
    ids, _ = shared.draw(X[:6], SEED, 1)
    assert tuple(ids.shape) == (2, 3)
    shared.candidate_rows(X[:6])
    assert eng.asked[-1][1] is pool
    # the list of every entity names no rows
    every = BoundSharedNegatives(eng, N, G, "uniform", None, None, all_list=torch.arange(N, dtype=torch.int32))
    assert not every.names_rows
    with pytest.raises(NotImplementedError, match="every row is a candidate"):
        every.candidate_rows(X[:6])
    assert KvsAll.names_rows is False and not SharedNegatives("all").names_rows and SharedNegatives("all", entities=["a"]).names_rows


# ------------------------------------------------------------------------------------------------ 3. bind and step refusals
@pytest.mark.parametrize("mode", ["FocusE", "ranks", "deterministic"])
def test_bind_refuses_what_the_shared_step_refuses(mode):
    class Loop:
        multi, deterministic = mode == "ranks", mode == "deterministic"

    m = _model(negatives={"shared": 6, "group_size": G}, optimizer_mode="sparse")
    m._n_ents, m._n_rels, m._loop, m.use_focusE = N, R, Loop(), mode == "FocusE"
    with pytest.raises(NotImplementedError) as e:
        m._negatives.bind(m, Engine("ComplEx"), torch.as_tensor(TRAIN))
    assert str(e.value).startswith("negatives:") and any(w in str(e.value) for w in S.KEYWORD[mode])


@pytest.mark.parametrize("mode", ["FocusE", "ranks", "deterministic", "no sampler", "override sampler", "identity list"])
def test_a_refused_sparse_step_touches_nothing(monkeypatch, mode):
    """as test_step_calls_host.test_a_refused_step_touches_nothing demands of the others: the optimizer's clock, the loop's step
    count, the FocusE fields of the loss descriptor and the engine are what they were"""
    negatives = {"shared": 6, "group_size": G}
    loop, eng, train = _setup("ComplEx", negatives, False, False, monkeypatch)
    if mode == "no sampler":
        loop.negatives = None
    elif mode == "override sampler":
        loop.negatives = lambda *a, **kw: pytest.fail("a refused step draws nothing")
    elif mode == "identity list":
        loop.negatives = BoundSharedNegatives(eng, N, G, "uniform", None, None, all_list=torch.arange(N, dtype=torch.int32))
    loop.multi, loop.deterministic = mode == "ranks", mode == "deterministic"
    loop.loss_ffi.focus_nonlinearity, loop.loss_ffi.d_focus_w = 2, 4096
    with pytest.raises(NotImplementedError) as e:
        loop.step(train[0:6], 7, focus=(torch.ones(6), 0.5, "linear") if mode == "FocusE" else None)
    words = {"no sampler": ("names no rows",), "override sampler": ("names no rows",), "identity list": ("every row is a candidate",)}.get(mode) or S.KEYWORD[mode]
    assert any(w in str(e.value) for w in words), str(e.value)
    assert (loop.optimizer.iterations, loop.n_steps, loop.loss_ffi.focus_nonlinearity, loop.loss_ffi.d_focus_w, eng.calls) == (0, 0, 2, 4096, [])


# ------------------------------------------------------------------------------------------------ 4. config and save round trip
def test_the_config_carries_the_mode_and_its_sampler():
    m = _model(negatives={"shared": 6, "group_size": G, "entities": ["a", "b"]}, optimizer_mode="sparse")
    oc = m.optimizer.get_config()
    assert oc["sparse"] is True and oc["lazy"] is False
    back = dict(json.loads(json.dumps(oc)))
    assert optimizers.get(back.pop("name"), back).sparse is True
    old = {k: v for k, v in oc.items() if k != "sparse"}      # a checkpoint written before the mode existed
    assert optimizers.get(old.pop("name"), old).sparse is False
    cfg = json.loads(json.dumps(m.get_config(), default=lambda o: o.tolist()))
    assert cfg["negatives"] == {"shared": 6, "group_size": G, "side": "uniform", "entities": ["a", "b"]}
    twin = ScoringBasedEmbeddingModel.from_config(cfg)
    assert isinstance(twin._negatives, SharedNegatives) and twin._negatives.num_negs == 6 and list(twin._negatives.entities) == ["a", "b"]
    # a dense model's config is what it was
    assert "negatives" not in _model(negatives={"shared": 6}).get_config() and _model().optimizer.get_config()["sparse"] is False


def test_restore_model_compiles_the_mode_again(tmp_path, monkeypatch):
    """save_model's two files written by hand around the parts that need no engine; load_weights is the engine's and is stubbed"""
    from ampligraph_amd.latent_features import regularizers
    from ampligraph_amd.utils.model_utils import restore_model

    m = _model("TransE", negatives=SharedDistanceNegatives(6, mask_known=True), optimizer_mode="sparse", entity_relation_regularizer="l2")
    d = tmp_path / "saved"
    d.mkdir()
    meta = {"config": m.get_config(), "optimizer": m.optimizer.get_config(), "loss": {"name": m.loss.name, "params": m.loss._loss_parameters},
            "regularizer": [regularizers.to_config(r) for r in m._regularizers]}
    (d / "model.json").write_text(json.dumps(meta, default=lambda o: o.tolist()))
    (d / "model.npz").write_bytes(b"")
    monkeypatch.setattr(ScoringBasedEmbeddingModel, "load_weights", lambda self, base: None)
    r = restore_model(str(d))
    assert r.optimizer.sparse is True and type(r._negatives) is SharedDistanceNegatives and r._negatives.mask_known is True
    assert r.get_config() == m.get_config()
    # without the key (an older checkpoint of a shared-negative model): dense, as before
    meta["optimizer"].pop("sparse")
    meta["config"].pop("negatives")
    (d / "model.json").write_text(json.dumps(meta))
    r = restore_model(str(d))
    assert r.optimizer.sparse is False and r._negatives is None


# ------------------------------------------------------------------------------------------------ 5. the numpy restatement
def test_candidate_rows_are_numpys_unique():
    X = np.array([[5, 0, 2], [2, 1, 5], [9, 0, 0]])
    assert SR.candidate_rows(X, np.array([[7, 2], [0, 11]])).tolist() == [0, 2, 5, 7, 9, 11]
    assert SR.candidate_rows(X).tolist() == [0, 2, 5, 9] and SR.candidate_rows(X).dtype == np.int32
    assert SR.candidate_rows(np.zeros((0, 3), int), np.array([3, 3])).tolist() == [3] and SR.candidate_rows(np.zeros((0, 3), int)).size == 0


@pytest.mark.parametrize("reg", [None, dict(p=2, lam_e=1e-2, lam_r=1e-3), dict(terms_e=[(3, 1e-3), (1, 1e-4)], terms_r=[(2, 1e-2)])], ids=["", "l2", "l3+l1"])
@pytest.mark.parametrize("kind", sorted(O.OPT_SLOTS))
def test_sweep_rows_is_the_lazy_sweep_where_the_list_covers_the_nonzero_rows(kind, reg):
    rng = np.random.default_rng(3)
    n, r, K = 40, 5, 8
    ent, rel = rng.normal(size=(n, K)).astype(np.float32), rng.normal(size=(r, K)).astype(np.float32)
    Ge, Gr = np.zeros((n, K), np.float32), rng.normal(size=(r, K)).astype(np.float32)
    hot = rng.choice(n, 11, replace=False)
    Ge[hot] = rng.normal(size=(11, K)).astype(np.float32)
    Gr[2] = 0
    listed = np.union1d(hot, rng.choice(n, 9, replace=False))       # a strict superset: listed all-zero rows stay
    assert listed.size > hot.size

    def run(sweep):
        st = O.TrainState(ent, rel, kind, 1e-2)
        for _ in range(2):   # the second sweep meets slots that moved
            out = sweep(st)
        return st, out

    a, la = run(lambda st: O.apply_optimizer_lazy(st, Ge, Gr, reg, ent_mask=None))
    b, (lb, left) = run(lambda st: SR.sweep_rows(st, Ge, Gr, listed, reg))
    assert np.array_equal(a.ent, b.ent) and np.array_equal(a.rel, b.rel) and la == lb and not left.any()
    assert all(np.array_equal(a.slots[k], b.slots[k]) for k in a.slots)
    assert np.array_equal(a.ent[np.setdiff1d(np.arange(n), hot)], ent[np.setdiff1d(np.arange(n), hot)])
    # a row with a gradient that is NOT listed keeps everything, its gradient included
    c, (_, left) = run(lambda st: SR.sweep_rows(st, Ge, Gr, listed[listed != hot[0]], reg))
    assert np.array_equal(c.ent[hot[0]], ent[hot[0]]) and np.array_equal(left[hot[0]], Ge[hot[0]]) and not np.array_equal(a.ent[hot[0]], ent[hot[0]])
    others = np.arange(n) != hot[0]
    assert np.array_equal(c.ent[others], a.ent[others]) and not left[others].any()
