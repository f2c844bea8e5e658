"""KvsAll training (include/amdkge_shared_labels.h) without a GPU: the numpy restatement (tests/shared_labels_ref.py) against torch
autograd of binary_cross_entropy_with_logits, the weight="query" identity, the surface of KvsAll / BCELoss (forms, refusals, config
round trip), the argument checks of the three entry points, and what one StepLoop.step calls."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import shared_labels_ref as LR
import shared_mask_ref as MR
import shared_ref as SR
from bound_samplers import bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ampligraph_amd", "lib", "libamdkge.so")


def tables(model, N, R, k, seed=0, scale=0.6):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(N, k)) * scale).astype(np.float32), (rng.normal(size=(R, k)) * scale).astype(np.float32)


def graph(seed, n, N, R):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the definition is the standard one
def torch_step(model, ent, rel, X, G, ids, side, labels, eps, reduction, w):
    """the step in torch fp64: the scores restated (DistMult: <s * p, o>; TransE: -|s + p - o|_1), F.binary_cross_entropy_with_logits
    with the smoothed targets and the row weights -> (loss, dL/d ent, dL/d rel)"""
    E = torch.tensor(ent.astype(np.float64), requires_grad=True)
    Rl = torch.tensor(rel.astype(np.float64), requires_grad=True)
    Xt = torch.as_tensor(np.asarray(X, dtype=np.int64))
    B, M = X.shape[0], ids.shape[1]
    lists = torch.as_tensor(np.asarray(ids, dtype=np.int64)[np.arange(B) // min(G, B)])
    subj = torch.as_tensor(np.asarray(side) != 0)[:, None]
    s, p, o = E[Xt[:, 0]], Rl[Xt[:, 1]], E[Xt[:, 2]]
    cand = E[lists]                                                             # [B, M, k]
    if model == "DistMult":
        q = torch.where(subj, p * o, s * p)
        S = (q[:, None, :] * cand).sum(-1)
    else:
        q = torch.where(subj, o - p, s + p)
        S = -(q[:, None, :] - cand).abs().sum(-1)
    t = torch.as_tensor(LR.targets(labels, float(np.float32(eps))))
    wr = torch.as_tensor(LR.row_weights(side, w) / (M if reduction == "mean" else 1.0))[:, None]
    loss = (wr * torch.nn.functional.binary_cross_entropy_with_logits(S, t, reduction="none")).sum()
    loss.backward()
    return float(loss.detach()), E.grad.numpy(), Rl.grad.numpy()


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("model", ["DistMult", "TransE"])
def test_labelled_step_equals_autograd_of_bce_with_logits(model, eps, reduction, weights):
    """The restatement rounds its scores to fp32 (the oracle's, and the header's distance arithmetic) where autograd keeps fp64: a
    relative 6e-8 per score, which the loss and a coefficient sig(x) - t (slope <= 1/4) carry on.  Bars: 1e-6 on the loss, 1e-5 of
    the largest entry on a gradient (sums of M such coefficients times O(1) rows)."""
    N, R, k, B, G, M = 30, 2, 6, 23, 8, 17
    ent, rel = tables(model, N, R, k)
    D = graph(1, 5 * N, N, R)
    X = D[np.random.default_rng(2).integers(0, len(D), B)]
    ids, side = SR.sample_shared(X, G, M, 3, 4, sample_range=N)
    ks, ko = MR.known_lists(X, [D], N, R)
    labels, n_lab, n_none = LR.label_matrix(X, G, ids, side, ks, ko)
    assert 0 < n_lab < B * M and 0 < side.sum() < B
    rng = np.random.default_rng(5)
    w = (rng.uniform(0.2, 1.0, B).astype(np.float32), rng.uniform(0.2, 1.0, B).astype(np.float32)) if weights else None
    L, Ge, Gr, sp, sn = LR.labelled_step(model, ent, rel, X, G, ids, side, labels, eps, reduction, w, R)
    Lt, Te, Tr = torch_step(model, ent, rel, X, G, ids, side, labels, eps, reduction, w)
    print(f"{model} eps={eps} {reduction} weights={weights}: loss {L:.12g} / {Lt:.12g}, gap ent {np.abs(Ge - Te).max() / np.abs(Te).max():.3g} "
          f"rel {np.abs(Gr - Tr).max() / np.abs(Tr).max():.3g}")
    assert abs(L - Lt) <= 1e-6 * abs(Lt)
    assert np.abs(Ge - Te).max() <= 1e-5 * np.abs(Te).max() and np.abs(Gr - Tr).max() <= 1e-5 * np.abs(Tr).max()


def test_bce32_is_bce64_on_finite_scores_and_follows_ieee_on_the_others():
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(5, 9)) * 4).astype(np.float32)
    labels = rng.random((5, 9)) < 0.3
    w = rng.uniform(0.5, 1.5, 5)
    for eps in (0.0, 0.1):
        per, c = LR.bce64(x.astype(np.float64), labels, eps, "mean", w)
        ell, c32, wr = LR.bce32(x, labels, eps, "mean", w)
        assert np.allclose((wr[:, None].astype(np.float64) * ell).sum(1), per, rtol=1e-5) and np.allclose(c32, c, rtol=0, atol=1e-6 * w.max() / 9)
    x[0, 0], x[1, 1], x[2, 2] = np.nan, np.inf, -np.inf
    labels[2, 2], labels[3, 3] = True, False
    x[3, 3] = -np.inf
    ell, c, _ = LR.bce32(x, labels, 0.0, "sum", np.ones(5))
    assert np.isnan(ell[0, 0]) and np.isnan(c[0, 0])                            # NaN in, NaN out (fmaxf(x, 0) alone would give a number)
    assert np.isnan(ell[1, 1]) and c[1, 1] == (0.0 if labels[1, 1] else 1.0)    # +inf: inf - inf (or inf - 0 * inf); sig = 1
    assert np.isposinf(ell[2, 2]) and c[2, 2] == -1.0                           # -inf, t = 1: +inf; sig = 0
    assert np.isnan(ell[3, 3]) and c[3, 3] == 0.0                               # -inf, t = 0: 0 * inf
    assert np.isfinite(np.delete(ell.reshape(-1), [0, 10, 20, 30])).all()


# ------------------------------------------------------------------------------------------------ 2. weight="query"
def test_query_weights_give_the_loss_over_the_unique_queries():
    """side "o": the rows sharing (s, p) have one list of labels and one row of scores, so with w = 1 / their number the weighted sum
    over ALL training rows is the unweighted sum over the unique (s, p) -- loss and gradients"""
    from ampligraph_amd.latent_features.negatives import KvsAll

    N, R, k, G = 12, 2, 5, 8
    X = graph(7, 60, N, R)
    X = np.concatenate([X, X[:3]])                                              # a duplicated triple (three of them)
    ws, wo = KvsAll.query_weights(X)
    sp_keys, first, counts = np.unique(X[:, :2], axis=0, return_index=True, return_counts=True)
    assert counts.max() > 2 and len(first) < len(X) and np.allclose(wo, 1.0 / counts[np.unique(X[:, :2], axis=0, return_inverse=True)[1].reshape(-1)])
    po_counts = {tuple(r): c for r, c in zip(*np.unique(X[:, 1:], axis=0, return_counts=True))}
    assert np.allclose(ws, [1.0 / po_counts[tuple(r)] for r in X[:, 1:]]) and ws.dtype == wo.dtype == np.float32
    ent, rel = tables("DistMult", N, R, k)
    ids = np.tile(np.arange(N, dtype=np.int32), (SR.n_groups(len(X), G), 1))

    def step(rows, w):
        Xr = X[rows]
        side = np.zeros(len(Xr), np.int32)
        ks, ko = MR.known_lists(Xr, [X], N, R)
        labels = LR.label_matrix(Xr, G, ids[:SR.n_groups(len(Xr), G)], side, ks, ko)[0]
        return LR.labelled_step("DistMult", ent, rel, Xr, G, ids[:SR.n_groups(len(Xr), G)], side, labels, 0.1, "sum", w, R)

    La, Ea, Ra, _, _ = step(np.arange(len(X)), (ws, wo))
    Lu, Eu, Ru, _, _ = step(np.sort(first), None)
    L1 = step(np.arange(len(X)), None)[0]
    print(f"weighted over {len(X)} rows {La:.12g}, unweighted over {len(first)} unique queries {Lu:.12g}, unweighted over all rows {L1:.12g}")
    assert abs(La - Lu) <= 1e-6 * abs(Lu) and abs(L1 - Lu) > 0.1 * abs(Lu)      # (float32 weights: 6e-8 each)
    assert np.allclose(Ea, Eu, rtol=1e-6, atol=1e-6 * np.abs(Eu).max()) and np.allclose(Ra, Ru, rtol=1e-6, atol=1e-6 * np.abs(Ru).max())


# ------------------------------------------------------------------------------------------------ 3. the surface
def _model(scoring="ComplEx", **kw):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    m = ScoringBasedEmbeddingModel(eta=2, k=8, scoring_type=scoring, seed=1)
    m.compile(optimizer="adam", **kw)
    return m


def test_forms_of_kvsall_and_bceloss():
    from ampligraph_amd.latent_features import BCELoss, KvsAll, loss_functions
    from ampligraph_amd.latent_features.negatives import NegativeSampling, SharedNegatives

    assert set(loss_functions.LOSS_REGISTRY) == {"pairwise", "nll", "absolute_margin", "self_adversarial", "multiclass_nll"}
    b = BCELoss()
    assert b._loss_parameters == {"reduction": "sum", "label_smoothing": 0.0} and b.name == "bce" and b.labelled
    b = loss_functions.get("bce", {"reduction": "mean", "label_smoothing": 0.1})
    assert isinstance(b, BCELoss) and b._loss_parameters == {"reduction": "mean", "label_smoothing": 0.1} and loss_functions.get(b) is b
    with pytest.raises(NotImplementedError, match="amdkge_loss"):
        b.to_ffi()
    for bad in (1.0, -0.1, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="label_smoothing"):
            BCELoss({"label_smoothing": bad})
    with pytest.raises(AssertionError):
        BCELoss({"reduction": "max"})
    s = KvsAll()
    assert (s.side, s.weight, s.known, s.group_size, s.shared, s.kvsall) == ("uniform", "triple", True, SharedNegatives.ALL_GROUP_SIZE, True, True)
    d = {"kvsall": "all", "side": "o", "weight": "query", "known": {"valid": np.zeros((1, 3), np.int64)}, "group_size": 64}
    s = NegativeSampling.get(d)
    assert isinstance(s, KvsAll) and s.get_config() == d and NegativeSampling.get(s) is s
    assert NegativeSampling.get({"kvsall": "all"}).get_config() == KvsAll().get_config()
    for bad, match in (({"kvsall": 5}, "kvsall"), ({"kvsall": "all", "entities": ["a"]}, "unknown keys"), ({"kvsall": "all", "side": "x"}, "side"),
                       ({"kvsall": "all", "weight": "row"}, "weight"), ({"kvsall": "all", "known": False}, "known"), ({"kvsall": "all", "known": {}}, "known"),
                       ({"kvsall": "all", "group_size": 0}, "group_size")):
        with pytest.raises(ValueError, match=match):
            NegativeSampling.get(bad)


def test_compile_refusals():
    from ampligraph_amd.latent_features import BCELoss, KvsAll

    for scoring in ("TransE", "DistMult", "ComplEx", "HolE", "RotatE"):         # all five models
        m = _model(scoring, loss=BCELoss({"label_smoothing": 0.1}), negatives=KvsAll())
        assert m.is_compiled and m._negatives.kvsall and m.loss.labelled
    with pytest.raises(NotImplementedError, match="SharedNegatives\\('all', mask_known=True\\)"):
        _model(loss="multiclass_nll", negatives=KvsAll())
    for negatives in (None, {"shared": "all", "mask_known": True}, {"filter": True}):
        with pytest.raises(NotImplementedError, match="KvsAll"):
            _model(loss=BCELoss(), negatives=negatives)
    with pytest.raises(NotImplementedError, match="deterministic"):
        _model(loss=BCELoss(), negatives=KvsAll(), deterministic=True)
    with pytest.raises(NotImplementedError, match="lazy"):
        _model(loss=BCELoss(), negatives=KvsAll(), optimizer_mode="lazy")
    for sharding in ("rows", "columns"):
        with pytest.raises(NotImplementedError, match="sharded"):
            _model(loss=BCELoss(), negatives=KvsAll(), entity_sharding=sharding)


def test_bind_refusals():
    from ampligraph_amd.latent_features.negatives import KvsAll

    class M:
        use_focusE, _loop, _n_ents, _n_rels = True, None, 5, 2

    with pytest.raises(NotImplementedError, match="FocusE"):
        KvsAll().bind(M(), None, None)

    class L:
        multi, deterministic = True, False

    M.use_focusE, M._loop = False, L()
    with pytest.raises(NotImplementedError, match="one rank"):
        KvsAll().bind(M(), None, None)
    L.multi, L.deterministic = False, True
    with pytest.raises(NotImplementedError, match="deterministic"):
        KvsAll().bind(M(), None, None)


def test_config_round_trip():
    from ampligraph_amd.latent_features import BCELoss, KvsAll, ScoringBasedEmbeddingModel

    m = _model(loss=BCELoss({"label_smoothing": 0.1, "reduction": "mean"}), negatives=KvsAll(side="o", weight="query", group_size=32))
    cfg = m.get_config()
    assert cfg["negatives"] == {"kvsall": "all", "side": "o", "weight": "query", "known": True, "group_size": 32}
    m2 = ScoringBasedEmbeddingModel.from_config(cfg)
    assert m2._negatives.get_config() == cfg["negatives"] and m2.get_config() == cfg
    assert "negatives" not in _model(loss="nll").get_config() and "negatives" not in _model(loss="nll", negatives={"shared": 4}).get_config()


# ------------------------------------------------------------------------------------------------ 4. the built library
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return LIB


def test_symbols_are_exported_and_bound(built):
    from ampligraph_amd import _ffi

    labels = _ffi.ABI["amdkge_shared_labels.h"]   # names, types against the header and binding: tests/test_abi_host.py
    assert len(labels["amdkge_shared_label_loss"][1]) == 22
    # the step entry points: the masked ones' arguments, the amdkge_loss* replaced by (float, int32), two weight pointers added
    masked = _ffi.ABI["amdkge_shared_mask.h"]["amdkge_train_shared_masked_fwdbwd"][1]
    want = [masked[0], C.c_float, _ffi.I32] + masked[2:-2] + [_ffi.P, _ffi.P] + masked[-2:]
    assert labels["amdkge_train_shared_labels_fwdbwd"][1] == want
    assert labels["amdkge_train_shared_dist_labels_fwdbwd"][1] == want


def test_argument_checks_return_before_touching_a_device(built):
    """every call below ends in AMDKGE_EINVAL / AMDKGE_EUNSUPPORTED: the pointers are host bytes that nothing reads"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    buf = C.create_string_buffer(256)
    p = C.addressof(buf)
    six = [p] * 6

    def kernel(scores=p, row0=0, rows=4, G=2, M=3, ids=p, side=p, ranges=six, mode=0, eps=0.1, mean=0, scale=1.0, ws=None, wo=None, loss=p):
        return lib.amdkge_shared_label_loss(scores, row0, rows, G, M, ids, side, *ranges, mode, eps, mean, scale, ws, wo, loss, None, None)

    def err():
        return lib.amdkge_last_error().decode()

    for kw, word in ((dict(eps=1.0), "label_smoothing"), (dict(eps=-0.01), "label_smoothing"), (dict(eps=float("nan")), "label_smoothing"),
                     (dict(ranges=[p, p, p, None, p, p]), "six range arrays"), (dict(ranges=[None] * 6), "six range arrays"),
                     (dict(ws=p), "d_w_s and d_w_o"), (dict(wo=p), "d_w_s and d_w_o"), (dict(mode=2), "list_mode"), (dict(ids=None), "d_neg_ids"),
                     (dict(scores=None), "NULL"), (dict(side=None), "NULL"), (dict(loss=None), "NULL"), (dict(row0=-1), "bad sizes"), (dict(rows=-1), "bad sizes"),
                     (dict(G=0), "bad sizes"), (dict(M=0), "bad sizes"), (dict(M=1 << 24), "bad sizes"), (dict(scale=0.0), "scale"), (dict(scale=float("inf")), "scale")):
        assert kernel(**kw) == -1 and word in err(), (kw, err())
    assert kernel(rows=0) == 0 and kernel(rows=0, ids=None, mode=1) == 0           # nothing to do; IDENTITY needs no ids

    for name, model_ok, model_bad in (("amdkge_train_shared_labels_fwdbwd", 2, 0), ("amdkge_train_shared_dist_labels_fwdbwd", 0, 2)):
        fn = getattr(lib, name)

        def step(model=model_ok, eps=0.1, B=4, G=2, M=3, ids=p, ranges=six, mode=0, ws=None, wo=None, tables=p, fn=fn):
            m = _ffi.Model(model, 8, 5, 2, 2, 0)
            return fn(C.byref(m), eps, 0, tables, tables, p, B, G, M, ids, p, p, p, p, None, None, p, *ranges, mode, ws, wo, None, None)

        for kw, word in ((dict(eps=1.0), "label_smoothing"), (dict(eps=float("nan")), "label_smoothing"), (dict(ranges=[None] * 6), "six range arrays"),
                         (dict(ranges=[p, None, p, p, p, p]), "six range arrays"), (dict(ws=p), "d_w_s and d_w_o"), (dict(wo=p), "d_w_s and d_w_o"),
                         (dict(mode=7), "list_mode"), (dict(ids=None), "d_neg_ids"), (dict(M=0), "bad sizes"), (dict(G=0), "bad sizes"), (dict(B=-1), "bad sizes"),
                         (dict(tables=None), "NULL"), (dict(model=9), "scoring_type")):
            assert step(**kw) == -1 and word in err(), (name, kw, err())
        assert step(model=model_bad) == -5 and "score a" in err()                  # AMDKGE_EUNSUPPORTED: the other family's models
        assert step(B=0) == 0


# ------------------------------------------------------------------------------------------------ 5. what the step loop calls
class _RecordingEngine:
    """the surface trainer.StepLoop uses on one rank in the shared branch, recording the calls"""
    scoring_type, k, device = "ComplEx", 8, "cpu"

    def __init__(self):
        self.calls = []

    def prepare_training(self, name):
        pass

    def train_shared_labels_fwdbwd(self, triples, G, M, ids, side, s_filter, o_filter, **kw):
        self.calls.append(("train_shared_labels_fwdbwd", G, M, s_filter, o_filter, kw))

    def train_shared_dist_labels_fwdbwd(self, triples, G, M, ids, side, s_filter, o_filter, **kw):
        self.calls.append(("train_shared_dist_labels_fwdbwd", G, M, s_filter, o_filter, kw))

    def train_shared_masked_fwdbwd(self, *a, **kw):
        self.calls.append(("train_shared_masked_fwdbwd",))

    def batch_reg_fwdbwd(self, triples, reg_e, reg_r):
        self.calls.append(("batch_reg_fwdbwd", int(triples.shape[0]), reg_e, reg_r))

    def opt_step(self, opt, reg_e, reg_r):
        self.calls.append(("opt_step", reg_e, reg_r))


def _loop(loss, reg=None, negatives=False, **bound_kw):
    """negatives: whether the loop gets a BoundKvsAll (tests/bound_samplers.py; bound_kw: its weights / distance)"""
    from ampligraph_amd.latent_features import optimizers
    from ampligraph_amd.trainer import StepLoop

    eng = _RecordingEngine()
    loop = StepLoop(eng, 2, loss, optimizers.get("sgd"), reg, seed=0, dist=None)
    loop.negatives = bound(eng, "kvsall", num_negs=9, **bound_kw) if negatives else None
    return loop, eng, torch.zeros(6, 3, dtype=torch.int32)


def test_the_calls_of_one_step(monkeypatch):
    from ampligraph_amd.latent_features import BCELoss, loss_functions
    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer

    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    bce = BCELoss({"label_smoothing": 0.1, "reduction": "mean"})
    kw = dict(label_smoothing=0.1, reduction="mean", weights=None, identity=True, stats="stats")
    loop, eng, X = _loop(bce, negatives=True)
    assert loop.loss_ffi is None and loop.label_loss is bce
    loop.step(X, 0)
    assert eng.calls == [("train_shared_labels_fwdbwd", 4, 9, "sf", "of", kw), ("opt_step", None, None)]
    # the distance models; the row weights; N3 between the backward call and the sweep
    n3 = BatchLPRegularizer(3, 0.25)
    loop, eng, X = _loop(bce, reg=n3, negatives=True, weights=("ws", "wo"), distance=True)
    loop.step(X, 0)
    assert eng.calls == [("train_shared_dist_labels_fwdbwd", 4, 9, "sf", "of", dict(kw, weights=("ws", "wo"))), ("batch_reg_fwdbwd", 6, n3, n3),
                         ("opt_step", None, None)]
    # the two halves exist only together
    loop, eng, X = _loop(bce)
    with pytest.raises(NotImplementedError, match="KvsAll"):
        loop.step(X, 0)
    loop, eng, X = _loop(loss_functions.get("nll"), negatives=True)
    with pytest.raises(NotImplementedError, match="BCELoss"):
        loop.step(X, 0)
    loop, eng, X = _loop(bce, negatives=True)
    with pytest.raises(NotImplementedError, match="FocusE"):
        loop.step(X, 0, focus=(torch.ones(6), 0.5, "linear"))
    assert eng.calls == []
