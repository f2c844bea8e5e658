"""Shared negatives for the distance models without a GPU: what is the extension header's own (include/amdkge_shared_dist.h;
names and types: tests/test_abi_host.py), the argument validation of both entry points (returned before any device
work), SharedDistanceNegatives and compile(), the step loop's choice of call, and the numpy restatement of the header's arithmetic
(tests/shared_dist_ref.py) against the oracle on the override rows."""
import ctypes as C

import numpy as np
import pytest

import shared_dist_ref as DR
import shared_ref as SR
from ampligraph_amd._ffi import EINVAL, EUNSUPPORTED
from bound_samplers import bound
from oracle import kge_oracle as O

CONTRACTION, DISTANCE = ("DistMult", "ComplEx", "HolE"), ("TransE", "RotatE")


# ------------------------------------------------------------------------------------------------------------ header and binding table
def test_extension_header_and_its_signature_table():
    from ampligraph_amd import _ffi

    dist = _ffi.ABI["amdkge_shared_dist.h"]
    # exactly the argument lists of the entry points they stand next to
    assert dist["amdkge_train_shared_dist_fwdbwd"] == _ffi.ABI["amdkge_shared_mask.h"]["amdkge_train_shared_masked_fwdbwd"]
    assert dist["amdkge_train_shared_dist_workspace_bytes"] == _ffi.ABI["amdkge_shared.h"]["amdkge_train_shared_workspace_bytes"]


def _model(_ffi, name, k=8, N=50, R=4):
    return _ffi.Model(_ffi.SCORING_TYPES[name], k, N, R, R, 0, 0, 0)


def test_workspace_bytes_without_gpu():
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    for name in DISTANCE:
        m = _model(_ffi, name)
        K = 16 if name == "RotatE" else 8
        need = lib.amdkge_train_shared_dist_workspace_bytes(C.byref(m), 37, 5, 33)
        assert need >= 4 * (2 * 37 * K + 2 * 37 + 37 * 33) and need % 256 == 0
        assert lib.amdkge_train_shared_dist_workspace_bytes(C.byref(m), 37, 500, 33) == need   # G is clamped to B: one chunk holds every row either way
        assert lib.amdkge_train_shared_workspace_bytes(C.byref(m), 37, 5, 33) == 0             # the matrix-product step still refuses them
        for bad in ((0, 5, 33), (-1, 5, 33), (37, 0, 33), (37, -2, 33), (37, 5, 0), (37, 5, -1), (37, 5, 1 << 24)):
            assert lib.amdkge_train_shared_dist_workspace_bytes(C.byref(m), *bad) == 0, bad
    for name in CONTRACTION:
        m = _model(_ffi, name)
        assert lib.amdkge_train_shared_dist_workspace_bytes(C.byref(m), 37, 5, 33) == 0
        assert lib.amdkge_train_shared_workspace_bytes(C.byref(m), 37, 5, 33) > 0
    assert lib.amdkge_train_shared_dist_workspace_bytes(None, 37, 5, 33) == 0
    bad = _model(_ffi, "TransE", k=0)
    assert lib.amdkge_train_shared_dist_workspace_bytes(C.byref(bad), 37, 5, 33) == 0


def test_argument_validation_without_gpu():
    """Every error below is returned before any device work: the pointers that are set are never dereferenced."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)
    six = ("s_lo", "s_hi", "s_ids", "o_lo", "o_hi", "o_ids")
    ls = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)

    def step(model="TransE", loss=ls, ent=X, rel=X, tri=X, B=5, G=2, M=3, ids=X, side=X, ge=X, gr=X, acc=X, work=X, mode=0, stats=X, **rg):
        r = {k: X for k in six}
        r.update(rg)
        m = _model(_ffi, model)
        return lib.amdkge_train_shared_dist_fwdbwd(C.byref(m), C.byref(loss) if loss is not None else None, ent, rel, tri, B, G, M, ids, side, ge, gr, acc, None,
                                                   None, work, *(r[k] for k in six), mode, stats, None)

    none = {k: None for k in six}
    for rg in ({}, none):                                                       # masked and unmasked
        for model in CONTRACTION:
            assert step(model=model, **rg) == EUNSUPPORTED and b"amdkge_train_shared_fwdbwd" in lib.amdkge_last_error()
        for model in DISTANCE:
            for bad in (dict(B=-1), dict(G=0), dict(G=-3), dict(M=0), dict(M=-1), dict(M=1 << 24), dict(loss=None), dict(ent=None), dict(rel=None), dict(ge=None),
                        dict(gr=None), dict(acc=None), dict(tri=None), dict(ids=None), dict(side=None), dict(work=None)):
                assert step(model=model, **bad, **rg) == EINVAL, bad
            assert step(model=model, loss=_ffi.Loss(9, 0, 0.0, 0.0), **rg) == EINVAL
            focus = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)
            focus.focus_nonlinearity, focus.d_focus_w = 1, 4096
            assert step(model=model, loss=focus, **rg) == EUNSUPPORTED and b"FocusE" in lib.amdkge_last_error()
            assert step(model=model, B=0, tri=None, side=None, work=None, **rg) == 0   # nothing to do
    bad_model = _ffi.Model(17, 8, 50, 4, 4, 0, 0, 0)
    assert lib.amdkge_train_shared_dist_fwdbwd(C.byref(bad_model), C.byref(ls), X, X, X, 5, 2, 3, X, X, X, X, X, None, None, X, *([None] * 6), 0, None, None) == EINVAL
    # the range arrays given only in part, the list mode
    for k in six:
        assert step(**{k: None}) == EINVAL and b"together" in lib.amdkge_last_error(), k
        assert step(**dict(none, **{k: X})) == EINVAL, k
    for mode in (-1, 2, 9):
        assert step(mode=mode) == EINVAL and b"list_mode" in lib.amdkge_last_error()
        assert step(mode=mode, **none) == EINVAL
    assert step(ids=None, mode=0) == EINVAL and b"d_neg_ids" in lib.amdkge_last_error()
    assert step(ids=None, mode=1) == EINVAL                                 # (the tiles gather by the ids whatever the mask reads)


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_class_dict_and_config_round_trip():
    from ampligraph_amd.latent_features.negatives import NegativeSampling, SharedDistanceNegatives, SharedNegatives

    d = SharedDistanceNegatives(64)
    assert isinstance(d, SharedNegatives) and d.shared is True
    assert d.get_config() == {"shared_distance": 64, "group_size": 64, "side": "uniform", "entities": None}
    got = NegativeSampling.get({"shared_distance": "all", "mask_known": True, "side": "bernoulli", "group_size": 100})
    assert type(got) is SharedDistanceNegatives and (got.num_negs, got.mask_known, got.side, got.group_size) == ("all", True, "bernoulli", 100)
    cfg = got.get_config()
    assert cfg == {"shared_distance": "all", "group_size": 100, "side": "bernoulli", "entities": None, "mask_known": True}
    again = NegativeSampling.get(cfg)
    assert type(again) is SharedDistanceNegatives and again.get_config() == cfg
    assert SharedDistanceNegatives("all").group_size == SharedNegatives.ALL_GROUP_SIZE
    ents = np.array(["a", "b"])
    assert NegativeSampling.get({"shared_distance": 4, "entities": ents}).get_config()["entities"].tolist() == ["a", "b"]
    # the plain class and its dict are what they were
    plain = NegativeSampling.get({"shared": 16})
    assert type(plain) is SharedNegatives and plain.get_config() == {"shared": 16, "group_size": 16, "side": "uniform", "entities": None}
    assert not hasattr(plain, "distance")
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"shared_distance": 16, "max_tries": 3})
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"shared_distance": 16, "shared_negs": 3})
    with pytest.raises(ValueError, match="breaks the sharing"):
        NegativeSampling.get({"shared_distance": 16, "filter": True})
    with pytest.raises(ValueError, match="num_negs"):
        NegativeSampling.get({"shared_distance": "every"})
    with pytest.raises(ValueError, match="mask_known"):
        SharedDistanceNegatives(8, mask_known="yes")


def test_compile_accepts_the_distance_models_and_keeps_the_refusals():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import SharedDistanceNegatives, SharedNegatives

    for model in DISTANCE:
        for spec in ({"shared_distance": 32, "mask_known": True}, SharedDistanceNegatives(1024, side="bernoulli", mask_known=True)):
            m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=model)
            m.compile(optimizer="adam", loss="self_adversarial", negatives=spec)
            assert type(m._negatives) is SharedDistanceNegatives and m._negatives.mask_known is True
        with pytest.raises(NotImplementedError, match="deterministic"):
            m.compile(optimizer="adam", loss="nll", negatives={"shared_distance": 8}, deterministic=True)
        with pytest.raises(NotImplementedError, match="lazy"):
            m.compile(optimizer="adam", loss="nll", negatives={"shared_distance": 8}, optimizer_mode="lazy")
        for sharding in ("rows", "columns"):
            with pytest.raises(NotImplementedError, match="entity_sharding"):
                m.compile(optimizer="adam", loss="nll", negatives={"shared_distance": 8}, entity_sharding=sharding)
        with pytest.raises(ValueError, match="breaks the sharing"):
            m.compile(optimizer="adam", loss="nll", negatives={"shared_distance": 8, "filter": True})
        # SharedNegatives on a distance model still raises; its message names the new class
        with pytest.raises(NotImplementedError, match="scores a distance.*SharedDistanceNegatives"):
            m.compile(optimizer="adam", loss="nll", negatives=SharedNegatives(8))
    for model in CONTRACTION:
        m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=model)
        for spec in ({"shared_distance": 8}, SharedDistanceNegatives(8)):
            with pytest.raises(NotImplementedError, match="SharedNegatives"):
                m.compile(optimizer="adam", loss="nll", negatives=spec)
        m.compile(optimizer="adam", loss="nll", negatives={"shared": 8})


def test_bind_marks_the_bound_sampler_and_keeps_its_refusals():
    from ampligraph_amd.latent_features.negatives import SharedDistanceNegatives

    class Model:
        _n_ents, _n_rels, use_focusE, _loop = 10, 2, True, None

    with pytest.raises(NotImplementedError, match="FocusE"):
        SharedDistanceNegatives(4).bind(Model(), None, None)

    class Loop:
        multi, deterministic = True, False

    Model.use_focusE, Model._loop = False, Loop()
    with pytest.raises(NotImplementedError, match="one rank"):
        SharedDistanceNegatives(4).bind(Model(), None, None)
    Loop.multi, Loop.deterministic = False, True
    with pytest.raises(NotImplementedError, match="deterministic"):
        SharedDistanceNegatives(4).bind(Model(), None, None)
    Loop.deterministic = False

    class Engine:
        device = "cpu"

    b = SharedDistanceNegatives(4, group_size=3, side="o").bind(Model(), Engine(), None)
    assert b.distance is True and b.shared is True and (b.num_negs, b.group_size, b.side) == (4, 3, "o") and not hasattr(b, "mask")
    a = SharedDistanceNegatives("all").bind(Model(), Engine(), None)
    assert a.distance is True and a.num_negs == 10 and a.all_list.tolist() == list(range(10))


def test_step_loop_takes_the_distance_call_only_for_a_distance_sampler():
    import torch

    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    calls = []

    class Eng:
        scoring_type, k, device = "TransE", 8, "cpu"

        def prepare_training(self, name):
            pass

        def train_shared_fwdbwd(self, triples, G, M, ids, side, loss):
            calls.append(("shared", tuple(triples.shape), G, M, ids, side))

        def train_shared_masked_fwdbwd(self, triples, G, M, ids, side, loss, s_filter=None, o_filter=None, identity=False, stats=None):
            calls.append(("masked", tuple(triples.shape), G, M, ids, side, s_filter, o_filter, identity, stats))

        def train_shared_dist_fwdbwd(self, triples, G, M, ids, side, loss, **kw):
            calls.append(("dist", tuple(triples.shape), G, M, ids, side, kw))

        def opt_step(self, *a):
            calls.append(("opt",))

    loop = StepLoop(Eng(), 3, loss_functions.get("nll"), optimizers.get("adam"), None, seed=5, dist=None)
    batch = torch.zeros(10, 3, dtype=torch.int32)
    loop.negatives = bound(loop.engine, "shared", calls, distance=True)
    loop.step(batch, 7)
    assert calls == [("draw", (10, 3), 5, 7), ("dist", (10, 3), 4, 6, "ids", "side", {}), ("opt",)]
    del calls[:]
    loop.negatives = bound(loop.engine, "masked", calls, distance=True)
    loop.step(batch, 8)
    assert calls == [("draw", (10, 3), 5, 8), ("mask", (10, 3)),
                     ("dist", (10, 3), 4, 6, "ids", "side", dict(s_filter="sf", o_filter="of", identity=True, stats="stats")), ("opt",)]
    del calls[:]
    loop.negatives = bound(loop.engine, "shared", calls)                                                   # a sampler without the attribute: exactly today's calls
    loop.step(batch, 9)
    assert calls == [("draw", (10, 3), 5, 9), ("shared", (10, 3), 4, 6, "ids", "side"), ("opt",)]
    del calls[:]
    loop.negatives = bound(loop.engine, "masked", calls)
    loop.step(batch, 10)
    assert calls == [("draw", (10, 3), 5, 10), ("mask", (10, 3)), ("masked", (10, 3), 4, 6, "ids", "side", "sf", "of", True, "stats"), ("opt",)] and loop.n_steps == 4
    loop.negatives = bound(loop.engine, "shared", calls, distance=True)
    with pytest.raises(NotImplementedError, match="FocusE"):
        loop.step(batch, 11, focus=(torch.zeros(10), 0.5, "linear"))
    loop.deterministic = True
    with pytest.raises(NotImplementedError, match="deterministic"):
        loop.step(batch, 11)
    loop.deterministic, loop.multi = False, True
    with pytest.raises(NotImplementedError, match="one rank"):
        loop.step(batch, 12)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _tables(model, k, N, R, seed, scale=0.6):
    rng = np.random.default_rng(seed)
    K = O.internal_k(model, k)
    return (rng.normal(size=(N, K)) * scale).astype(np.float32), (rng.normal(size=(R, K)) * scale).astype(np.float32)


def _row_gap(G, T):
    scale = np.maximum(np.abs(T).max(axis=1, keepdims=True), 1e-6 * max(np.abs(T).max(), 1e-30))
    return float((np.abs(G - T) / scale).max())


@pytest.mark.parametrize("model", DISTANCE)
@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_restatement_equals_the_oracle_on_the_override_rows(model, reduction):
    """The header's formulation (one query per positive, the conj form for RotatE's subject side, the chain through the query map)
    against O.dense_gradients on SR.override_rows: fp64 sums on both sides, so the gap is the fp32 rounding of q and of the residual
    (1e-7 relative) -- held to 1e-5 on the scores and the row-scaled 2e-5 of assert_grads_close on the gradients, under the
    precondition that no residual is within rounding of zero."""
    N, R, k, B, G, M = 60, 4, 12, 37, 8, 9
    ent, rel = _tables(model, k, N, R, seed=3)
    rng = np.random.default_rng(4)
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
    ids, side = SR.sample_shared(X, G, M, 9, 4, sample_range=N)
    ids[0, 0], ids[0, 1], ids[1, 0] = N - 1, 0, X[8, 2]
    assert 0 < side.sum() < B
    st = DR.DistStep(model, ent, rel, X, G, ids, side, R)
    assert st.min_modulus() > (1e-6 if model == "TransE" else 1e-3)
    negs = SR.override_rows(X, G, ids, side)
    for loss in O.LOSS_DEFAULTS:
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, M, loss, None, reduction, R)
        L, Ge, Gr, ps, ns = st.step(loss, reduction)
        assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max()) and np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L))
        assert _row_gap(Ge, Te) < 2e-5 and _row_gap(Gr, Tr) < 2e-5, (loss, _row_gap(Ge, Te), _row_gap(Gr, Tr))


def test_transe_query_is_the_reference_one_vs_all_order():
    """|e + (p - o)| == |(o - p) - e| bit for bit: the scores of the restatement are O.corruption_scores' on both sides."""
    N, R, k, B = 30, 3, 10, 12
    ent, rel = _tables("TransE", k, N, R, seed=5)
    rng = np.random.default_rng(6)
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
    ids = np.arange(N, dtype=np.int32)[None, :]
    s, p, o = O.lookup(ent, rel, X)
    for sd, name in ((1, "s"), (0, "o")):
        st = DR.DistStep("TransE", ent, rel, X, B, ids, np.full(B, sd, np.int32), R)
        want = O.corruption_scores("TransE", name, s, p, o, ent)
        assert np.array_equal(st.neg_matrix.astype(np.float32), want)


def test_masked_entries_send_no_gradient():
    import shared_mask_ref as MR

    N, R, k, B, G, M = 20, 2, 6, 9, 4, 7
    for model in DISTANCE:
        ent, rel = _tables(model, k, N, R, seed=7)
        rng = np.random.default_rng(8)
        X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
        ids, side = SR.sample_shared(X, G, M, 2, 1, sample_range=N)
        mask = np.zeros((B, M), dtype=bool)
        mask[:, 2] = mask[3, 5] = True
        st = DR.DistStep(model, ent, rel, X, G, ids, side, R)
        L, Ge, Gr, sp, sn = st.step("self_adversarial", "sum", mask=mask)
        # the same definition through the oracle's own rows (tests/shared_mask_ref.py)
        L2, Te, Tr, sp2, sn2 = MR.masked_step(model, ent, rel, X, G, ids, side, mask, "self_adversarial", "sum", R)
        assert np.array_equal(np.isneginf(sn), np.isneginf(sn2)) and np.isfinite(L) and abs(L - L2) <= 1e-5 * max(1.0, abs(L2))
        assert _row_gap(Ge, Te) < 2e-5 and _row_gap(Gr, Tr) < 2e-5
