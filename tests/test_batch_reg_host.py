"""Batch regularisers (include/amdkge_batch_reg.h) without a GPU: the numpy restatement (tests/batch_reg_ref.py) against autograd and
against the whole-table regulariser, the regulariser surface (regularizers.get, the [entity, relation] pair, configs, compile()'s
refusals), what trainer.StepLoop.step calls, and the built library (the symbol, the kernel's resources)."""
import json
import os

import numpy as np
import pytest

import batch_reg_ref as BR
from bound_samplers import bound
from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, loss_functions, optimizers, regularizers
from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer, LPRegularizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ampligraph_amd", "lib", "libamdkge.so")


# ------------------------------------------------------------------------------------------------ the restatement
def _edge_case(model, k=5, N=9, R=3, seed=1):
    """tables and a batch with a repeated entity, a positive with s == o, and units at exactly zero (a float-mode one, and for the
    complex layouts a whole complex unit) in rows the batch uses"""
    ent, rel = BR.tables(model, k, N, R, seed)
    X = np.array([[0, 0, 1], [2, 1, 2], [0, 2, 3], [4, 0, 0], [5, 1, 6], [1, 1, 0]], np.int32)
    ent[0, 1] = 0.0
    rel[1, 0] = 0.0
    if BR.nc_of(model) == 2:
        ent[2, 3] = ent[2, k + 3] = 0.0
        rel[0, 2] = rel[0, k + 2] = 0.0
    return ent, rel, X


@pytest.mark.parametrize("p_e,p_r", [(2, 2), (3, 3), (3, 2)])
@pytest.mark.parametrize("model", BR.MODELS)
def test_gradient_against_autograd(model, p_e, p_r):
    """The restatement's gradient (fp32 per-unit values, fp64 sums) against torch autograd, in float64, of the same penalty.  What
    separates them is the fp32 rounding of the per-unit chain -- at most five roundings (m2's two products and sum, the square root,
    c m, f x; c itself), 2^-24 each -- on every occurrence: 1e-6 of the row's largest magnitude bounds it with room."""
    import torch

    k = 5
    ent, rel, X = _edge_case(model, k)
    lam_e, lam_r = 0.05, 0.125
    for norm_e, norm_r in BR.norms_of(model):
        R, Ge, Gr = BR.batch_reg(model, k, ent, rel, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r)
        te = torch.tensor(ent.astype(np.float64), requires_grad=True)
        tr = torch.tensor(rel.astype(np.float64), requires_grad=True)
        Rt = BR.penalty_torch(model, k, te, tr, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r)
        Rt.backward()
        Rt = float(Rt.detach())
        assert abs(R - Rt) <= 1e-6 * abs(Rt)
        assert np.isfinite(te.grad.numpy()).all() and np.isfinite(tr.grad.numpy()).all()
        BR.assert_rows_close(Ge, te.grad.numpy(), 1e-6)
        BR.assert_rows_close(Gr, tr.grad.numpy(), 1e-6)
        # a unit at exactly zero gets exactly zero; rows outside the batch get nothing
        assert Ge[0, 1] == 0.0 and Gr[1, 0] == 0.0 and not Ge[7:].any()
        if BR.nc_of(model) == 2:
            assert Ge[2, 3] == 0.0 and Ge[2, k + 3] == 0.0 and Gr[0, 2] == 0.0 and Gr[0, k + 2] == 0.0
        # the repeated entity 0 (s of two positives, o of two) is counted per occurrence
        _, g1 = BR.row_terms(ent[0:1], k, BR.nc_of(model), p_e, lam_e, norm_e)
        occ0 = int((X[:, 0] == 0).sum() + (X[:, 2] == 0).sum())
        assert occ0 == 4 and np.allclose(Ge[0], occ0 * g1[0].astype(np.float64), rtol=1e-12, atol=0)
        _, g2 = BR.row_terms(ent[2:3], k, BR.nc_of(model), p_e, lam_e, norm_e)
        assert np.allclose(Ge[2], 2 * g2[0].astype(np.float64), rtol=1e-12, atol=0)   # s == o: two occurrences


def test_n3_is_not_the_float_norm():
    """the reason the modulus mode exists: |re|^3 + |im|^3 != (re^2 + im^2)^(3/2)"""
    ent, rel, X = _edge_case("ComplEx")
    Rm = BR.batch_reg("ComplEx", 5, ent, rel, X, 3, 0.1, BR.MODULUS, 3, 0.1, BR.MODULUS)[0]
    Rf = BR.batch_reg("ComplEx", 5, ent, rel, X, 3, 0.1, BR.FLOAT, 3, 0.1, BR.FLOAT)[0]
    assert Rm > Rf * 1.05


@pytest.mark.parametrize("model", BR.MODELS)
def test_identity_with_the_whole_table_regulariser(model):
    """float norm, p = 2, every table row exactly once: the batch penalty is LPRegularizer(2, lambda)(table) and the gradient is
    2 lambda x on every float.  Entity rows occur once as s or o only if the relation term's batch differs: two batches."""
    k, N, R = 6, 8, 4
    ent, rel = BR.tables(model, k, N, R, 3)
    lam = 0.03125   # (a power of two: fl(2 lambda) and lambda x are exact in fp32, the comparison is on the sums alone)
    Xe = np.stack([np.arange(0, N, 2), np.zeros(N // 2, int), np.arange(1, N, 2)], 1)    # every entity once, as an s or an o
    Re, Ge, _ = BR.batch_reg(model, k, ent, rel, Xe, 2, lam, BR.FLOAT, 2, 0.0, BR.FLOAT)
    assert abs(Re - LPRegularizer(2, lam)(ent)) <= 1e-6 * Re
    assert np.array_equal(Ge, 2 * lam * ent.astype(np.float64))
    Xr = np.stack([np.zeros(R, int), np.arange(R), np.ones(R, int)], 1)                   # every relation once
    Rr, _, Gr = BR.batch_reg(model, k, ent, rel, Xr, 2, 0.0, BR.FLOAT, 2, lam, BR.FLOAT)
    assert abs(Rr - LPRegularizer(2, lam)(rel)) <= 1e-6 * Rr
    assert np.array_equal(Gr, 2 * lam * rel.astype(np.float64))


# ------------------------------------------------------------------------------------------------ the regulariser surface
def _lp(r):
    return None if r is None else (type(r).__name__, r.p, r.lam, r.p2, r.lam2)


# identifier, hyper-parameters -> what regularizers.get returned before the batch regularisers existed
PARENT_FORMS = [
    (None, None, None),
    ("l3", None, ("LPRegularizer", 3, 1e-5, 3, 0.0)),
    ("l3", {"lambda": 0.5}, ("LPRegularizer", 3, 0.5, 3, 0.0)),
    ("LP", None, ("LPRegularizer", 2, 1e-5, 2, 0.0)),
    ("LP", {"p": 3, "lambda": 1e-3}, ("LPRegularizer", 3, 1e-3, 3, 0.0)),
    ("LP", {"p": 1}, ("LPRegularizer", 1, 1e-5, 1, 0.0)),
    ("l1", None, ("LPRegularizer", 1, 0.01, 1, 0.0)),
    ("L1", None, ("LPRegularizer", 1, 0.01, 1, 0.0)),
    ("l2", None, ("LPRegularizer", 2, 0.01, 2, 0.0)),
    ("L2", None, ("LPRegularizer", 2, 0.01, 2, 0.0)),
    ("l1_l2", None, ("LPRegularizer", 1, 0.01, 2, 0.01)),
    ({"class_name": "L1L2", "config": {"l1": 0.25, "l2": 0.5}}, None, ("LPRegularizer", 1, 0.25, 2, 0.5)),
    ({"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.5}}, None, ("LPRegularizer", 2, 0.5, 2, 0.0)),
    ({"class_name": "L1L2", "config": {}}, None, None),
    ({"class_name": "L1", "config": {"l1": 0.125}}, None, ("LPRegularizer", 1, 0.125, 2, 0.0)),
    ({"class_name": "L2", "config": {}}, None, ("LPRegularizer", 2, 0.01, 2, 0.0)),
]


@pytest.mark.parametrize("ident,hp,want", PARENT_FORMS, ids=[str(i) for i in range(len(PARENT_FORMS))])
def test_existing_identifiers_are_unchanged(ident, hp, want):
    assert _lp(regularizers.get(ident, hp)) == want


def test_existing_objects_and_errors_are_unchanged():
    r = LPRegularizer(3, 0.5)
    assert regularizers.get(r) is r and r.terms == [(3, 0.5)] and LPRegularizer(1, 0.1, 2, 0.2).terms == [(1, 0.1), (2, 0.2)]
    for bad in ("n3", "batch_lp", "nope", 7):
        with pytest.raises(ValueError, match="Could not interpret regularizer identifier"):
            regularizers.get(bad)


def test_batch_forms():
    n3 = regularizers.get("N3", {"lambda": 0.25})
    assert isinstance(n3, BatchLPRegularizer) and (n3.p, n3.lam, n3.norm) == (3, 0.25, "auto") and n3.batch
    assert regularizers.get("N3") == BatchLPRegularizer(3, 1e-5, "auto")
    b = regularizers.get("batch_LP", {"p": 2, "lambda": 0.5, "norm": "float"})
    assert b == BatchLPRegularizer(2, 0.5, "float") and b != n3 and regularizers.get(b) is b
    assert regularizers.get("batch_LP") == BatchLPRegularizer() == BatchLPRegularizer(p=3, lam=1e-5, norm="auto")
    assert regularizers.is_batch(b) and not regularizers.is_batch(LPRegularizer()) and not regularizers.is_batch(None)
    for kw in (dict(p=1), dict(p=4), dict(p=2.5), dict(norm="l2"), dict(lam=-1.0), dict(lam=float("inf")), dict(lam=float("nan"))):
        with pytest.raises(ValueError):
            BatchLPRegularizer(**kw)


def test_auto_norm_follows_the_model_and_the_table():
    auto, mod, flt = BatchLPRegularizer(norm="auto"), BatchLPRegularizer(norm="modulus"), BatchLPRegularizer(norm="float")
    for model in BR.MODELS:
        for table in ("ent", "rel"):
            ok = BR.modulus_allowed(model, table)
            assert auto.norm_for(model, table) == ("modulus" if ok else "float")
            assert flt.norm_for(model, table) == "float"
            if ok:
                assert mod.norm_for(model, table) == "modulus"
            else:
                with pytest.raises(ValueError, match="phases" if model == "RotatE" else "real units"):
                    mod.norm_for(model, table)


def test_config_forms_round_trip():
    for r in (None, LPRegularizer(3, 0.5), LPRegularizer(1, 0.1, 2, 0.2), BatchLPRegularizer(2, 0.5, "float"), BatchLPRegularizer()):
        cfg = json.loads(json.dumps(regularizers.to_config(r)))
        back = regularizers.from_config(cfg)
        assert type(back) is type(r)
        assert back == r if regularizers.is_batch(r) else _lp(back) == _lp(r)
    # the whole-table form is what checkpoints held before: no "kind" field; a config without one restores as before
    assert regularizers.to_config(LPRegularizer(3, 0.5)) == {"p": 3, "lambda": 0.5, "p2": 3, "lambda2": 0.0}
    assert regularizers.to_config(BatchLPRegularizer(3, 0.5))["kind"] == "batch"
    assert _lp(regularizers.from_config({"p": 3, "lambda": 0.5})) == ("LPRegularizer", 3, 0.5, 3, 0.0)


def _compiled(scoring_type="ComplEx", reg=None, **kw):
    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=scoring_type, seed=3)
    m.compile(optimizer="sgd", loss="multiclass_nll", entity_relation_regularizer=reg, **kw)
    return m


def test_pair_form_and_model_config():
    n3, lp = BatchLPRegularizer(3, 0.25), LPRegularizer(2, 0.5)
    assert _compiled(reg=n3)._regularizers == [n3, n3]
    for pair in ([n3, None], [None, n3], [n3, lp], [lp, n3], ["N3", "l3"]):
        m = _compiled(reg=pair)
        assert [type(r) for r in m._regularizers] == [type(regularizers.get(r)) for r in pair]
        cfg = json.loads(json.dumps(m.get_config()))
        assert cfg["entity_relation_regularizer"] == [regularizers.to_config(r) for r in m._regularizers]
        back = ScoringBasedEmbeddingModel.from_config(cfg)
        assert back.get_config() == m.get_config() and (back.eta, back.k, back.scoring_type, back.seed) == (2, 4, "ComplEx", 3)
    # without a batch member the model's config is the constructor arguments alone, as before
    for reg in (None, lp, [lp, None], "l3"):
        assert _compiled(reg=reg).get_config() == {"eta": 2, "k": 4, "scoring_type": "ComplEx", "seed": 3, "max_ent_size": None, "max_rel_size": None}


@pytest.mark.parametrize("kw,reason", [(dict(deterministic=True), "atomics"), (dict(optimizer_mode="lazy"), "lazy"),
                                       (dict(entity_sharding="rows"), "entity_sharding"), (dict(entity_sharding="columns"), "entity_sharding")])
def test_compile_refusals_name_their_reason(kw, reason):
    with pytest.raises(NotImplementedError, match=reason):
        _compiled(reg="N3", **kw)
    with pytest.raises(NotImplementedError, match=reason):
        _compiled(reg=[None, BatchLPRegularizer(2, 0.1)], **kw)
    _compiled(reg="l3", **kw)   # the whole-table regulariser keeps every mode


def test_compile_refuses_the_modulus_where_rows_hold_no_complex_units():
    for model, pair in (("TransE", ["N3", None]), ("DistMult", [None, "N3"]), ("RotatE", ["N3", "N3"])):
        _compiled(model, [regularizers.get(r) for r in pair])   # (auto: float where the modulus is not offered)
    mod = BatchLPRegularizer(3, 0.1, "modulus")
    _compiled("RotatE", [mod, None])
    for model, pair in (("TransE", [mod, None]), ("DistMult", [None, mod]), ("RotatE", [None, mod])):
        with pytest.raises(ValueError, match="modulus"):
            _compiled(model, pair)


# ------------------------------------------------------------------------------------------------ what the step loop calls
class _RecordingEngine:
    """the surface trainer.StepLoop uses on one rank, recording the order of the calls"""
    scoring_type, k = "ComplEx", 8

    def __init__(self):
        self.calls = []

    def prepare_training(self, name):
        pass

    def tiled_supported(self, B, eta):
        return True

    def train_step_tiled(self, triples, eta, loss, opt, seed, step, reg_e=None, reg_r=None, **kw):
        self.calls.append(("train_step_tiled", reg_e, reg_r))

    def train_fwdbwd(self, triples, eta, loss, seed, step, **kw):
        self.calls.append(("train_fwdbwd",))

    def train_shared_fwdbwd(self, triples, G, M, ids, side, loss):
        self.calls.append(("train_shared_fwdbwd",))

    def batch_reg_fwdbwd(self, triples, reg_e, reg_r):
        self.calls.append(("batch_reg_fwdbwd", int(triples.shape[0]), reg_e, reg_r))

    def opt_step(self, opt, reg_e, reg_r):
        self.calls.append(("opt_step", reg_e, reg_r))


def _loop(reg, reg_rel="same", shared=False, **opt_kw):
    """shared: whether the loop gets a BoundSharedNegatives (tests/bound_samplers.py)"""
    import torch

    from ampligraph_amd.trainer import StepLoop

    eng = _RecordingEngine()
    loop = StepLoop(eng, 2, loss_functions.get("nll"), optimizers.get("sgd", opt_kw), reg, seed=0, dist=None)
    loop.reg_rel = reg_rel
    loop.negatives = bound(eng, "shared") if shared else None
    return loop, eng, torch.zeros(6, 3, dtype=torch.int32)


def test_step_without_a_batch_member_makes_todays_calls(monkeypatch):
    monkeypatch.delenv("AMDKGE_TRAIN_PATH", raising=False)
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    lp = LPRegularizer(3, 0.5)
    loop, eng, X = _loop(lp)
    loop.step(X, 0)
    assert eng.calls == [("train_step_tiled", lp, lp)]
    loop, eng, X = _loop(lp, reg_rel=None, shared=True)
    loop.step(X, 0)
    assert eng.calls == [("train_shared_fwdbwd",), ("opt_step", lp, None)]


def test_step_with_a_batch_member(monkeypatch):
    monkeypatch.delenv("AMDKGE_TRAIN_PATH", raising=False)
    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    n3, lp = BatchLPRegularizer(3, 0.25), LPRegularizer(2, 0.5)
    # shared branch: forward / backward, the batch regulariser, the sweep -- which takes the whole-table member only
    loop, eng, X = _loop(n3, reg_rel=lp, shared=True)
    loop.step(X, 0)
    assert eng.calls == [("train_shared_fwdbwd",), ("batch_reg_fwdbwd", 6, n3, None), ("opt_step", None, lp)]
    # per-corruption branch: the dense-gradient form, never the owner-computes step
    loop, eng, X = _loop(lp, reg_rel=n3)
    assert loop.use_tiled
    loop.step(X, 0)
    assert eng.calls == [("train_fwdbwd",), ("batch_reg_fwdbwd", 6, None, n3), ("opt_step", lp, None)]
    loop, eng, X = _loop(n3)   # one regulariser for both tables
    loop.step(X, 0)
    assert eng.calls == [("train_fwdbwd",), ("batch_reg_fwdbwd", 6, n3, n3), ("opt_step", None, None)]


def test_step_refusals(monkeypatch):
    import torch

    monkeypatch.delenv("AMDKGE_DETERMINISTIC", raising=False)
    n3 = BatchLPRegularizer(3, 0.25)
    loop, eng, X = _loop(n3)
    loop.deterministic = True
    with pytest.raises(NotImplementedError, match="atomics"):
        loop.step(X, 0)
    loop, eng, X = _loop(n3)
    with pytest.raises(NotImplementedError, match="FocusE"):
        loop.step(X, 0, focus=(torch.ones(6), 0.5, "linear"))
    loop, eng, X = _loop(n3, lazy=True)
    with pytest.raises(NotImplementedError, match="lazy"):
        loop.step(X, 0)
    assert eng.calls == []


def test_the_sweep_does_not_take_a_batch_regulariser():
    from ampligraph_amd.engine import reg_fields

    with pytest.raises(NotImplementedError, match="batch_reg_fwdbwd"):
        reg_fields(BatchLPRegularizer(), 2)
    assert reg_fields(LPRegularizer(3, 0.5), 2) == (3, 0.5, 2, 0.0) and reg_fields(None, 2) == (2, 0.0, 2, 0.0)


# ------------------------------------------------------------------------------------------------ the built library
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return LIB


def test_symbol_is_exported_and_bound(built):
    import ctypes as C

    from ampligraph_amd import _ffi

    # export, types against the header, binding and the header's values of BATCH_REG_NORMS: tests/test_abi_host.py
    res, args = _ffi.ABI["amdkge_batch_reg.h"]["amdkge_batch_reg_fwdbwd"]
    assert res is C.c_int and len(args) == 15 and args[6] is C.c_float and args[9] is C.c_float


def test_kernel_has_no_scratch_and_no_spills(built):
    """read from the code object the way tests/test_kernel_resources.py reads it: four instantiations (real / two-half layout, one
    float / 16 bytes per lane), none with scratch, LDS only the four doubles of the workgroup's penalty, at least four waves per SIMD"""
    from ampligraph_amd.utils.codeobj import kernel_resources

    res = {n: r for n, r in kernel_resources(built).items() if "batch_reg_kernel" in n}
    assert sorted(res) == [f"_ZN3kge16batch_reg_kernelILb{c}ELi{v}EEEvNS_12BatchRegArgsE" for c in (0, 1) for v in (1, 4)]
    for name, r in res.items():
        assert r["scratch"] == 0 and r["lds"] == 32 and r["agpr"] == 0 and r["waves_per_simd"] >= 4, (name, r)
