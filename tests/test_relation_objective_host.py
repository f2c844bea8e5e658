"""The relation-prediction training objective without a GPU: the numpy restatement (tests/relation_objective_ref.py) against torch
autograd of the matrix form with the softmax cross-entropy; the object, dict and config forms of RelationPrediction; every refusal;
the argument checks of the two entry points that return before a launch; the signature table against the header's text; and the
order of the calls trainer.StepLoop.step makes, on a recording double of the engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_decl
import relation_objective_ref as RR
from bound_samplers import bound
from ampligraph_amd.latent_features import RelationPrediction, ScoringBasedEmbeddingModel, loss_functions, optimizers
from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer, LPRegularizer
from oracle import kge_oracle as O

MODELS = ("DistMult", "ComplEx", "HolE")


def _case(model, k=7, N=12, R=9, B=23, seed=1):
    rng = np.random.default_rng(seed)
    K = O.internal_k(model, k)
    ent, rel = (rng.normal(size=(N, K)) * 0.6).astype(np.float32), (rng.normal(size=(R, K)) * 0.6).astype(np.float32)
    pool = rng.choice(N, 4, replace=False)
    D = np.stack([pool[rng.integers(0, 4, 3 * B)], rng.integers(0, R, 3 * B), pool[rng.integers(0, 4, 3 * B)]], 1).astype(np.int32)
    X = D[rng.integers(0, len(D), B)]
    return ent, rel, X, RR.known_relations(X, [D])


def _torch_scores(model, k, ent, rel, X):
    """the matrix form in fp64 with autograd: S [B, R] = scale * Q Rel^T, and the positives' scores"""
    e = torch.tensor(ent.astype(np.float64), requires_grad=True)
    r = torch.tensor(rel.astype(np.float64), requires_grad=True)
    s, o = e[torch.as_tensor(X[:, 0].astype(np.int64))], e[torch.as_tensor(X[:, 2].astype(np.int64))]
    if model == "DistMult":
        Q = s * o
    else:
        s0, s1, o0, o1 = s[:, :k], s[:, k:], o[:, :k], o[:, k:]
        Q = torch.cat([s0 * o0 + s1 * o1, s0 * o1 - s1 * o0], 1)
    scale = 2.0 / k if model == "HolE" else 1.0
    S = scale * Q @ r.T
    return e, r, S, S[torch.arange(len(X)), torch.as_tensor(X[:, 1].astype(np.int64))]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("model", MODELS)
def test_restatement_equals_autograd_of_the_matrix_form(model):
    """multiclass_nll, nothing masked: L_i = -s_pos + log(exp(s_pos) + sum_j exp(s_ij)) -- the reference's softmax with the positive as
    a class of its own next to all R relation scores (its own relation among them)"""
    k, w = 7, 0.25
    ent, rel, X, _ = _case(model, k)
    B, R = len(X), len(rel)
    L, Ge, Gr, sp, sn = RR.relation_step(model, ent, rel, X, np.zeros((B, R), dtype=bool), "multiclass_nll", "sum", w)
    e, r, S, pos = _torch_scores(model, k, ent, rel, X)
    assert np.allclose(S.detach().numpy().T.reshape(-1), sn, rtol=1e-5, atol=1e-6) and np.allclose(pos.detach().numpy(), sp, rtol=1e-5, atol=1e-6)
    loss = w * (torch.logsumexp(torch.cat([pos[:, None], S], 1), 1) - pos).sum()
    loss.backward()
    assert abs(L - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
    for G, T in ((Ge, e.grad.numpy()), (Gr, r.grad.numpy())):
        assert np.abs(G - T).max() <= 2e-6 * np.abs(T).max(), np.abs(G - T).max()


@pytest.mark.parametrize("model", MODELS)
def test_known_true_is_the_cross_entropy_over_the_unmasked_columns(model):
    """with the training set's relations of the pair masked (the row's own among them), a row's loss is cross_entropy with the
    positive as the target over [positive | the relations NOT known for the pair]: the masked entries add e^-75 terms only"""
    k = 7
    ent, rel, X, known = _case(model, k)
    B, R = len(X), len(rel)
    mask, masked, unmaskable = RR.mask_matrix(B, R, known)
    assert unmaskable == 0 and masked > B and mask[np.arange(B), X[:, 1]].all()
    _, _, S, pos = _torch_scores(model, k, ent, rel, X)
    for i in range(B):
        Li = RR.relation_step(model, ent, rel, X[i:i + 1], mask[i:i + 1], "multiclass_nll", "sum", 1.0)[0]
        logits = torch.cat([pos[i:i + 1], S[i][torch.as_tensor(~mask[i])]]).detach()
        want = float(torch.nn.functional.cross_entropy(logits[None, :], torch.zeros(1, dtype=torch.int64)))
        assert abs(Li - want) <= 1e-6 * max(1.0, abs(want)), (i, Li, want)


def test_fully_known_row_keeps_its_scores():
    mask, masked, unmaskable = RR.mask_matrix(3, 2, [np.array([0, 1]), np.array([1]), np.zeros(0, np.int32)])
    assert mask.tolist() == [[False, False], [False, True], [False, False]] and (masked, unmaskable) == (1, 1)
    assert RR.mask_matrix(2, 3, None)[1:] == (0, 0)
    assert RR.override_rows(np.array([[4, 1, 5], [6, 0, 7]]), 2).tolist() == [[4, 0, 5], [6, 0, 7], [4, 1, 5], [6, 1, 7]]


# ------------------------------------------------------------------------------------------------ forms
def test_object_dict_and_config_forms():
    rp = RelationPrediction()
    assert (rp.weight, rp.loss.name, rp.known) == (1.0, "multiclass_nll", True)
    rp = RelationPrediction.get({"weight": 0.25, "loss": "self_adversarial", "loss_params": {"margin": 2.0, "alpha": 0.25}, "known": False})
    assert (rp.weight, rp.loss.name, rp.known) == (0.25, "self_adversarial", False) and rp.loss._loss_parameters["margin"] == 2.0
    assert RelationPrediction.get(None) is None and RelationPrediction.get(rp) is rp
    back = RelationPrediction.get(rp.get_config())
    assert back.get_config() == rp.get_config()
    assert RelationPrediction(0.5, loss_functions.get("nll", {"reduction": "mean"})).get_config()["loss_params"] == {"reduction": "mean"}
    datasets = {"valid": np.array([["a", "r", "b"]])}
    assert RelationPrediction(known=datasets).known is datasets and RelationPrediction(weight=0).weight == 0.0
    for bad in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight="1"), dict(weight=True), dict(loss="no such loss"),
                dict(loss=3), dict(loss=loss_functions.BCELoss()), dict(known={}), dict(known="yes")):
        with pytest.raises(ValueError):
            RelationPrediction(**bad)
    with pytest.raises(ValueError, match="unknown keys"):
        RelationPrediction.get({"weigth": 1.0})
    with pytest.raises(ValueError):
        RelationPrediction.get(0.5)


def _compiled(scoring_type="ComplEx", **kw):
    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=scoring_type, seed=3)
    m.compile(optimizer="adam", loss="multiclass_nll", **kw)
    return m


def test_model_config_round_trip():
    plain = {"eta": 2, "k": 4, "scoring_type": "ComplEx", "seed": 3, "max_ent_size": None, "max_rel_size": None}
    for kw in ({}, {"relation_prediction": None}):
        m = _compiled(**kw)
        assert m.get_config() == plain and m._relation_prediction is None
    m = _compiled(relation_prediction={"weight": 0.25, "known": False})
    cfg = m.get_config()
    assert cfg == dict(plain, relation_prediction={"weight": 0.25, "loss": "multiclass_nll", "loss_params": {"reduction": "sum"}, "known": False})
    back = ScoringBasedEmbeddingModel.from_config(cfg)
    assert back._relation_prediction.get_config() == cfg["relation_prediction"] and back.get_config() == cfg
    m.compile(optimizer="adam", loss="nll")   # a second compile() without the keyword drops the term
    assert m._relation_prediction is None and m.get_config() == plain


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw,reason", [(dict(deterministic=True), "atomics"), (dict(optimizer_mode="lazy"), "lazy"),
                                       (dict(entity_sharding="rows"), "entity_sharding"), (dict(entity_sharding="columns"), "entity_sharding")])
def test_compile_refusals_name_their_reason(kw, reason):
    with pytest.raises(NotImplementedError, match=reason):
        _compiled(relation_prediction=RelationPrediction(0.5), **kw)
    _compiled(**kw)   # without the term every mode compiles


@pytest.mark.parametrize("model", ["TransE", "RotatE"])
def test_compile_refuses_the_distance_models(model):
    with pytest.raises(NotImplementedError, match="linear in the relation row"):
        _compiled(model, relation_prediction={"weight": 0.5})
    _compiled(model)


def test_compile_refuses_more_than_one_rank():
    class _Dist:
        def get_world_size(self):
            return 2

        def get_rank(self):
            return 0

    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="ComplEx", seed=3)
    m._dist_override = _Dist()
    with pytest.raises(NotImplementedError, match="one rank"):
        m.compile(optimizer="adam", loss="multiclass_nll", relation_prediction={"weight": 0.5})
    m.compile(optimizer="adam", loss="multiclass_nll")


def test_compile_passes_bad_values_on_as_value_errors():
    for bad in ({"weight": -0.5}, {"loss": "softmax"}, {"weight": float("nan")}):
        with pytest.raises(ValueError):
            _compiled(relation_prediction=bad)


def test_bind_refuses_focuse():
    class _M:
        use_focusE, _loop = True, None

    with pytest.raises(NotImplementedError, match="FocusE"):
        RelationPrediction(0.5).bind(_M(), None, None)


# ------------------------------------------------------------------------------------------------ what the step loop calls
class _RecordingEngine:
    """the surface trainer.StepLoop uses on one rank, recording the order of the calls"""
    scoring_type, k, device = "ComplEx", 8, "cpu"

    def __init__(self):
        self.calls = []

    def prepare_training(self, name):
        pass

    def tiled_supported(self, B, eta):
        return True

    def train_step_tiled(self, triples, eta, loss, opt, seed, step, reg_e=None, reg_r=None, **kw):
        self.calls.append(("train_step_tiled",))

    def train_fwdbwd(self, triples, eta, loss, seed, step, **kw):
        self.calls.append(("train_fwdbwd",))

    def train_shared_fwdbwd(self, triples, G, M, ids, side, loss):
        self.calls.append(("train_shared_fwdbwd",))

    def train_shared_masked_fwdbwd(self, triples, G, M, ids, side, loss, **kw):
        self.calls.append(("train_shared_masked_fwdbwd",))

    def train_shared_dist_fwdbwd(self, triples, G, M, ids, side, loss, **kw):
        self.calls.append(("train_shared_dist_fwdbwd",))

    def train_shared_labels_fwdbwd(self, triples, G, M, ids, side, sf, of, **kw):
        self.calls.append(("train_shared_labels_fwdbwd",))

    def train_relation_fwdbwd(self, triples, loss, weight, flt=None, stats=None, **kw):
        self.calls.append(("train_relation_fwdbwd", int(triples.shape[0]), float(weight), flt is not None))

    def batch_reg_fwdbwd(self, triples, reg_e, reg_r):
        self.calls.append(("batch_reg_fwdbwd",))

    def opt_step(self, opt, reg_e, reg_r):
        self.calls.append(("opt_step",))


class _Term:
    """BoundRelationPrediction without a device: step(batch) -> engine.train_relation_fwdbwd"""

    def __init__(self, engine, weight=0.25):
        self.engine, self.weight = engine, weight

    def step(self, batch):
        self.engine.train_relation_fwdbwd(batch, None, self.weight, flt=("lo", "hi", "ids"))


def _loop(reg=None, negatives=None, term=True, loss="nll", **opt_kw):
    """negatives: None or the arguments of bound() (tests/bound_samplers.py) behind the engine"""
    from ampligraph_amd.trainer import StepLoop

    eng = _RecordingEngine()
    loop = StepLoop(eng, 2, loss_functions.get(loss), optimizers.get("sgd", opt_kw), reg, seed=0, dist=None)
    loop.negatives = None if negatives is None else bound(eng, **negatives)
    assert loop.relation is None
    if term:
        loop.relation = _Term(eng)
    return loop, eng, torch.zeros(6, 3, dtype=torch.int32)


REL = ("train_relation_fwdbwd", 6, 0.25, True)


@pytest.mark.parametrize("name,negatives,loss,main", [
    ("shared", lambda: dict(kind="shared"), "nll", "train_shared_fwdbwd"),
    ("masked", lambda: dict(kind="masked"), "nll", "train_shared_masked_fwdbwd"),
    ("distance", lambda: dict(kind="shared", distance=True), "nll", "train_shared_dist_fwdbwd"),
    ("kvsall", lambda: dict(kind="kvsall"), loss_functions.BCELoss(), "train_shared_labels_fwdbwd"),
    ("per-corruption", lambda: None, "nll", "train_fwdbwd")])
def test_step_order(monkeypatch, name, negatives, loss, main):
    """main step -> relation term -> batch regulariser (if any) -> opt_step, on every branch; the per-corruption branch takes the
    dense-gradient step, never the owner-computes one"""
    monkeypatch.delenv("AMDKGE_TRAIN_PATH", raising=False)
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    loop, eng, X = _loop(None, negatives(), loss=loss)
    loop.step(X, 0)
    assert eng.calls == [(main,), REL, ("opt_step",)]
    loop, eng, X = _loop(BatchLPRegularizer(3, 0.25), negatives(), loss=loss)
    loop.step(X, 0)
    assert eng.calls == [(main,), REL, ("batch_reg_fwdbwd",), ("opt_step",)]
    loop, eng, X = _loop(LPRegularizer(2, 0.5), negatives(), term=False, loss=loss)   # without the term: today's calls
    loop.step(X, 0)
    assert eng.calls == ([("train_step_tiled",)] if name == "per-corruption" else [(main,), ("opt_step",)])


def test_step_refusals(monkeypatch):
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    loop, eng, X = _loop()
    loop.deterministic = True
    with pytest.raises(NotImplementedError, match="atomics"):
        loop.step(X, 0)
    loop, eng, X = _loop()
    with pytest.raises(NotImplementedError, match="FocusE"):
        loop.step(X, 0, focus=(torch.ones(6), 0.5, "linear"))
    loop, eng, X = _loop(lazy=True)
    with pytest.raises(NotImplementedError, match="lazy"):
        loop.step(X, 0)
    loop, eng, X = _loop()
    loop.multi = True
    with pytest.raises(NotImplementedError, match="one rank"):
        loop.step(X, 0)
    assert eng.calls == []


# ------------------------------------------------------------------------------------------------ the built library
def test_signature_table_matches_the_header_text():
    """names, types against the header text, binding and amdkge.h's silence: tests/test_abi_host.py; here what is this header's own"""
    assert "#include \"amdkge.h\"" in abi_decl.text("amdkge_relation_objective.h")


def test_argument_checks_return_before_a_launch():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    EINVAL, EUNSUPPORTED = _ffi.EINVAL, _ffi.EUNSUPPORTED
    m = _ffi.Model(_ffi.SCORING_TYPES["ComplEx"], 8, 5, 3, 3, 0, 0, 0)
    loss = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
    one = C.c_void_p(8)   # a non-NULL pointer no check dereferences

    def call(model=m, ls=loss, w=1.0, ent=one, rel=one, tri=one, B=4, lo=None, hi=None, known=None, ge=one, gr=one, acc=one, work=one):
        return lib.amdkge_train_relation_fwdbwd(C.byref(model) if model is not None else None, C.byref(ls) if ls is not None else None, w, ent, rel, tri, B, lo, hi, known,
                                                ge, gr, acc, None, None, work, None, None)

    for model in ("TransE", "RotatE"):
        assert call(model=_ffi.Model(_ffi.SCORING_TYPES[model], 8, 5, 3, 3, 0, 0, 0)) == EUNSUPPORTED
        assert lib.amdkge_train_relation_workspace_bytes(C.byref(_ffi.Model(_ffi.SCORING_TYPES[model], 8, 5, 3, 3, 0, 0, 0)), 4) == 0
    assert b"TransE and RotatE" in lib.amdkge_last_error()
    focus = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0, 1, 0.5, None)
    assert call(ls=focus) == EUNSUPPORTED and b"FocusE" in lib.amdkge_last_error()
    for kw in (dict(model=None), dict(ls=None), dict(ls=_ffi.Loss(9, 0, 0.0, 0.0)), dict(w=-1.0), dict(w=float("nan")), dict(w=float("inf")), dict(B=-1),
               dict(ent=None), dict(rel=None), dict(ge=None), dict(gr=None), dict(acc=None), dict(tri=None), dict(work=None),
               dict(lo=one), dict(lo=one, hi=one), dict(hi=one, known=one), dict(known=one)):
        assert call(**kw) == EINVAL, kw
    assert b"range arrays" in lib.amdkge_last_error()
    assert call(B=0) == 0 and call(B=0, tri=None, work=None) == 0            # an empty batch is a no-op
    assert call(w=0.0) == 0 and call(w=0.0, tri=None, work=None) == 0        # and so is a weight of zero
    assert call(w=0.0, lo=one) == EINVAL and call(B=0, w=-1.0) == EINVAL     # ... whose other arguments are still checked
    # the workspace: 0 for what the path does not take, else 2 B (K + 1) floats, B int32, a double and one chunk of scores
    ws = lib.amdkge_train_relation_workspace_bytes
    assert ws(None, 4) == 0 and ws(C.byref(m), 0) == 0 and ws(C.byref(m), -3) == 0
    assert ws(C.byref(m), 4) >= 4 * (2 * 4 * 17 + 4 + 4 * 3) + 8
    big = _ffi.Model(_ffi.SCORING_TYPES["DistMult"], 8, 5, 240, 240, 0, 0, 0)
    assert ws(C.byref(big), 70000) < 4 * (2 * 70000 * 9 + 70000) + 4 * (1 << 24) + 4096   # the score buffer is one chunk, not B * R
