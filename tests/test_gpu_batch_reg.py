"""amdkge_batch_reg_fwdbwd (include/amdkge_batch_reg.h) against its numpy restatement (tests/batch_reg_ref.py): every model, norm mode
and p, dense and padded rows, the one-float and the 16-byte path with one chunk of units and with two, batches of less than a
workgroup's four waves up to one past 64 workgroups' worth; a term switched off with a NULL gradient table, B = 0, the refusals,
NaN / inf, and the regulariser end to end through fit(), save_model and restore_model.

Bars: gradients 1e-5 of the row's largest magnitude (the project's bar for the default, unordered mode: the order of the atomic
adds is free), the penalty 1e-6 relative (fp32 lane sums of at most 2 * 5 values per lane and 64 lanes, then double)."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_reg_ref as BR
from ampligraph_amd._ffi import EINVAL, EUNSUPPORTED
from test_gpu_guard_bands import stored, unstored
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

PAD_MARK = 7.0   # what the padding floats of a gradient table hold on entry


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Case:
    """tables of one model in the stored layout on the device"""

    def __init__(self, model, k, N, R, pad, seed=0, scale=0.3):
        from ampligraph_amd import _ffi

        self.model, self.k, self.N, self.R = model, k, N, R
        self.nc = BR.nc_of(model)
        self.ks = (k + 3) // 4 * 4 if pad else k
        self.ent, self.rel = BR.tables(model, k, N, R, seed, scale)
        self.m = _ffi.Model(_ffi.SCORING_TYPES[model], k, N, R, R, self.ks, 0, 0)
        self.upload()

    def upload(self):
        self.d_ent, self.d_rel = dev(stored(self.ent, self.k, self.ks, self.nc)), dev(stored(self.rel, self.k, self.ks, self.nc))

    def grad_table(self, n):
        """zeros in the live floats, PAD_MARK in the padding floats"""
        g = np.full((n, self.nc * self.ks), PAD_MARK, np.float32)
        for h in range(self.nc):
            g[:, h * self.ks:h * self.ks + self.k] = 0.0
        return g

    def call(self, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r, null_e=False, null_r=False, B=None, args=None):
        """-> (rc, penalty, entity gradient stored [N, Ks] or None, relation gradient); args: overrides of the pointer arguments"""
        from ampligraph_amd import _ffi

        ge0, gr0 = self.grad_table(self.N), self.grad_table(self.R)
        ge, gr = (None if null_e else dev(ge0)), (None if null_r else dev(gr0))
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        tri = dev(np.ascontiguousarray(X, np.int32)) if X is not None and len(X) else None
        a = dict(ent=P(self.d_ent), rel=P(self.d_rel), tri=P(tri), ge=P(ge), gr=P(gr), acc=P(acc))
        a.update(args or {})
        rc = _ffi.lib().amdkge_batch_reg_fwdbwd(C.byref(self.m), a["ent"], a["rel"], a["tri"], (0 if X is None else len(X)) if B is None else B,
                                                p_e, lam_e, norm_e, p_r, lam_r, norm_r, a["ge"], a["gr"], a["acc"], None)
        torch.cuda.synchronize()
        return rc, float(acc.item()), (None if ge is None else ge.cpu().numpy()), (None if gr is None else gr.cpu().numpy())

    def padding_untouched(self, g):
        want = self.grad_table(g.shape[0])
        mask = want == PAD_MARK
        return np.array_equal(g[mask].view(np.uint32), want[mask].view(np.uint32))

    def check(self, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r, **kw):
        rc, R, ge, gr = self.call(X, p_e, lam_e, norm_e, p_r, lam_r, norm_r, **kw)
        assert rc == 0, rc
        wR, wGe, wGr = BR.batch_reg(self.model, self.k, self.ent, self.rel, X, p_e, lam_e, norm_e, p_r, lam_r, norm_r)
        assert abs(R - wR) <= 1e-6 * abs(wR), (R, wR)
        for g, w in ((ge, wGe), (gr, wGr)):
            if g is not None:
                assert self.padding_untouched(g)
                BR.assert_rows_close(unstored(g, self.k, self.ks, self.nc), w, 1e-5)
        return R, ge, gr


LAM_E, LAM_R = 0.05, 0.125


# k: 1 and 7 (one lane, one partial group), 33 (odd, padded to 36), 70 (two chunks of the one-float path), 200 (the product's width:
# 16-byte path with dense rows too), 300 (two chunks of the 16-byte path)
@pytest.mark.parametrize("pad", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("k", [1, 7, 33, 70, 200, 300])
@pytest.mark.parametrize("model", BR.MODELS)
def test_kernel_against_the_restatement(gpu_lib, model, k, pad):
    N, R = 50, 5
    cs = Case(model, k, N, R, pad, seed=k)
    rng = np.random.default_rng(100 + k)
    combos = [(pe, pr, ne, nr) for (ne, nr) in BR.norms_of(model) for pe, pr in ((3, 2), (2, 3))]
    for n, B in enumerate((1, 63, 65, 257)):
        X = BR.triples(rng, B, N, R)
        for pe, pr, ne, nr in (combos if B == 257 else [combos[n % len(combos)]]):
            cs.check(X, pe, LAM_E, ne, pr, LAM_R, nr)
    # one hub entity in every row, as subject and as object: 2 * 130 occurrences of one row
    X = np.stack([np.full(130, 17), rng.integers(0, R, 130), np.full(130, 17)], 1)
    pe, pr, ne, nr = combos[0]
    _, ge, _ = cs.check(X, pe, LAM_E, ne, pr, LAM_R, nr)
    assert not np.delete(unstored(ge, k, cs.ks, cs.nc), 17, axis=0).any()


@pytest.mark.parametrize("model,k,pad", [("ComplEx", 33, True), ("TransE", 7, False), ("RotatE", 200, True)])
def test_a_term_switched_off_and_an_empty_batch(gpu_lib, model, k, pad):
    N, R = 50, 5
    cs = Case(model, k, N, R, pad)
    X = BR.triples(np.random.default_rng(5), 65, N, R)
    ne = BR.MODULUS if BR.modulus_allowed(model, "ent") else BR.FLOAT
    # lambda == 0: the term's table is not touched and may be NULL
    R_e, ge, gr = cs.check(X, 3, LAM_E, ne, 2, 0.0, BR.FLOAT, null_r=True)
    assert gr is None and ge.any()
    R_r, ge, gr = cs.check(X, 3, 0.0, ne, 2, LAM_R, BR.FLOAT, null_e=True)
    assert ge is None and gr.any()
    R_er, _, _ = cs.check(X, 3, LAM_E, ne, 2, LAM_R, BR.FLOAT)
    assert abs(R_er - (R_e + R_r)) <= 1e-6 * R_er
    rc, R0, ge, gr = cs.call(X, 3, 0.0, ne, 2, 0.0, BR.FLOAT)                       # both off, tables given: untouched
    assert rc == 0 and R0 == 0.0 and np.array_equal(ge, cs.grad_table(N)) and np.array_equal(gr, cs.grad_table(R))
    assert cs.call(X, 3, 0.0, ne, 2, 0.0, BR.FLOAT, null_e=True, null_r=True)[:2] == (0, 0.0)
    # B == 0 does nothing, with or without a triples pointer
    for Xe in (None, np.zeros((0, 3), np.int32)):
        rc, R0, ge, gr = cs.call(Xe, 3, LAM_E, ne, 2, LAM_R, BR.FLOAT)
        assert rc == 0 and R0 == 0.0 and np.array_equal(ge, cs.grad_table(N)) and np.array_equal(gr, cs.grad_table(R))


def test_refusals_write_nothing(gpu_lib):
    from ampligraph_amd import _ffi

    N, R = 50, 5
    X = BR.triples(np.random.default_rng(6), 65, N, R)
    F, M = BR.FLOAT, BR.MODULUS

    def refused(cs, want, why, *terms, **kw):
        rc, R0, ge, gr = cs.call(X, *terms, **kw)
        assert rc == want, (why, rc)
        msg = _ffi.lib().amdkge_last_error().decode()
        assert "batch_reg" in msg or "model" in msg or "k " in msg, msg
        assert R0 == 0.0 and (ge is None or np.array_equal(ge, cs.grad_table(N))) and (gr is None or np.array_equal(gr, cs.grad_table(R))), why
        return msg

    cx = Case("ComplEx", 8, N, R, True)
    for p in (0, 1, 4, -3):
        assert "entity" in refused(cx, EINVAL, "p_ent", p, LAM_E, M, 3, LAM_R, M)
        assert "relation" in refused(cx, EINVAL, "p_rel", 3, LAM_E, M, p, LAM_R, M)
        refused(cx, EINVAL, "p of a term that is off", p, 0.0, M, 3, LAM_R, M)
    for norm in (-1, 2):
        refused(cx, EINVAL, "norm_ent", 3, LAM_E, norm, 3, LAM_R, M)
        refused(cx, EINVAL, "norm_rel", 3, LAM_E, M, 3, LAM_R, norm)
    for lam in (-0.5, float("nan"), float("inf")):
        refused(cx, EINVAL, "lambda_ent", 3, lam, M, 3, LAM_R, M)
        refused(cx, EINVAL, "lambda_rel", 3, LAM_E, M, 3, lam, M)
    refused(cx, EINVAL, "B < 0", 3, LAM_E, M, 3, LAM_R, M, B=-1)
    for name in ("ent", "rel", "acc", "tri"):
        refused(cx, EINVAL, "NULL " + name, 3, LAM_E, M, 3, LAM_R, M, args={name: None})
    refused(cx, EINVAL, "NULL g_ent, lambda_ent != 0", 3, LAM_E, M, 3, LAM_R, M, null_e=True)
    refused(cx, EINVAL, "NULL g_rel, lambda_rel != 0", 3, LAM_E, M, 3, LAM_R, M, null_r=True)
    for model in ("TransE", "DistMult"):
        cs = Case(model, 8, N, R, True)
        assert "real units" in refused(cs, EUNSUPPORTED, model + " entity modulus", 3, LAM_E, M, 3, LAM_R, F)
        assert "real units" in refused(cs, EUNSUPPORTED, model + " relation modulus", 3, LAM_E, F, 3, LAM_R, M)
        refused(cs, EUNSUPPORTED, model + " modulus of a term that is off", 3, 0.0, M, 3, LAM_R, F)
    cr = Case("RotatE", 8, N, R, True)
    assert "phases" in refused(cr, EUNSUPPORTED, "RotatE relation modulus", 3, LAM_E, M, 3, LAM_R, M)
    assert cr.call(X, 3, LAM_E, M, 3, LAM_R, F)[0] == 0
    bad = Case("ComplEx", 8, N, R, True)
    bad.m.k = 0
    refused(bad, EINVAL, "invalid model", 3, LAM_E, M, 3, LAM_R, M)


# ------------------------------------------------------------------------------------------------------------ NaN and inf
@pytest.mark.parametrize("pad", [False, True], ids=["one-float", "16-byte"])
@pytest.mark.parametrize("norm,p", [(BR.MODULUS, 3), (BR.MODULUS, 2), (BR.FLOAT, 3), (BR.FLOAT, 2)])
def test_nan_and_inf_reach_exactly_the_defined_floats(gpu_lib, norm, p, pad):
    """One NaN (re of unit 2) and one inf (im of unit 5) in entity row 3.  Every row of the batch occurs exactly ONCE in it, so every
    gradient float receives one add and the run without the plant is reproducible bit for bit: all other rows are compared bitwise."""
    model, k, N, R, B = "ComplEx", 7, 24, 12, 12
    cs = Case(model, k, N, R, pad)
    X = np.stack([np.arange(B), np.arange(B), B + np.arange(B)], 1)                  # s = i, p = i, o = 12 + i: all distinct
    terms = (p, LAM_E, norm, p, LAM_R, norm)
    rc, R0, ge0, gr0 = cs.call(X, *terms)
    assert rc == 0 and np.isfinite(R0) and np.isfinite(ge0).all()
    cs.ent[3, 2], cs.ent[3, k + 5] = np.nan, np.inf
    cs.upload()
    rc, R1, ge1, gr1 = cs.call(X, *terms)
    assert rc == 0 and not np.isfinite(R1)
    g = unstored(ge1, k, cs.ks, cs.nc)
    bad = np.zeros((N, 2 * k), bool)
    bad[3, 2] = bad[3, k + 5] = True                                                  # the floats themselves, always
    if norm == BR.MODULUS and p == 3:
        bad[3, k + 2] = bad[3, 5] = True                                              # f = c * m: both components of the unit
    assert np.array_equal(~np.isfinite(g), bad), np.argwhere(~np.isfinite(g) != bad)
    assert np.isnan(g[3, 2]) and (np.isposinf(g[3, k + 5]) if not (norm == BR.MODULUS and p == 3) else not np.isfinite(g[3, k + 5]))
    # the restatement says the same, float for float
    _, wGe, _ = BR.batch_reg(model, k, cs.ent, cs.rel, X, *terms)
    assert np.array_equal(~np.isfinite(wGe), bad)
    # the finite floats of the planted row, every other entity row, the whole relation table, the padding: bitwise what they were
    g0 = unstored(ge0, k, cs.ks, cs.nc)
    assert np.array_equal(g[~bad].view(np.uint32), g0[~bad].view(np.uint32))
    assert np.array_equal(gr1.view(np.uint32), gr0.view(np.uint32)) and cs.padding_untouched(ge1)


# ------------------------------------------------------------------------------------------------------------ end to end
def _fit(model, reg, negatives, loss, **compile_kw):
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    m = ScoringBasedEmbeddingModel(eta=3, k=10, scoring_type=model, seed=2)
    m.compile(optimizer=optimizers.get("sgd", {"learning_rate": 1.0}), loss=loss, entity_relation_regularizer=reg,
              **({"negatives": negatives} if negatives is not None else {}), **compile_kw)
    return m


E2E = [("ComplEx", {"shared": "all", "mask_known": True}, "multiclass_nll"),
       ("TransE", {"shared_distance": 16, "group_size": 20}, "self_adversarial"),
       ("DistMult", None, "nll")]
LAM = 0.0625


def _bound(T0, Ta, Tb, Gd, Gr_ref):
    """per row: see test_one_sgd_step_moves_the_tables_by_the_restatements_gradient"""
    row = lambda A: np.abs(A).max(axis=1, keepdims=True)   # noqa: E731
    return 2e-5 * row(Gd) + 1e-5 * row(Gr_ref) + 2.0 ** -23 * np.maximum(row(Ta), row(Tb))


@pytest.mark.parametrize("model,negatives,loss", E2E, ids=[e[0] for e in E2E])
def test_one_sgd_step_moves_the_tables_by_the_restatements_gradient(gpu_lib, monkeypatch, model, negatives, loss):
    """One epoch of one batch, SGD with learning rate 1: table = fl(T0 - g) with g the step's dense gradient, so
    table_without - table_with = g_with - g_without = the regulariser's gradient, up to
      * each of the two tables rounded once by its sweep: 2^-24 of its magnitude each -> 2^-23 max(|Ta|, |Tb|) of the row;
      * the data gradient, which both runs accumulate with unordered fp32 atomics: each run is within the project's default-mode bar,
        1e-5 of the row's largest data gradient, of the exact sum -> 2e-5 max|g_data| of the row (g_data is read off the run WITHOUT
        the regulariser, T0 - Ta: code that exists without this feature);
      * the regulariser's rows added into that buffer by fp32 atomics: the kernel's own bar, 1e-5 of the row's largest regulariser
        gradient, which covers the one fp32 add per occurrence onto the data gradient.
    The bound is per row, the sum of the three.  The epoch's loss differs by the restatement's penalty (each run's data loss within the
    project's 1e-5 of itself).  DistMult on the per-corruption path: both runs take the dense-gradient step (AMDKGE_TRAIN_PATH=atomic
    for the run without the regulariser), so that the same kernels and the same draw produce the data gradient of both."""
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer

    if negatives is None:
        monkeypatch.setenv("AMDKGE_TRAIN_PATH", "atomic")
    X = toy_graph(seed=4, n=300, N=40, R=3)
    n3 = BatchLPRegularizer(3, LAM)
    m0 = _fit(model, None, negatives, loss)
    m0.fit(X, batch_size=len(X), epochs=0, verbose=False)                              # the initial tables
    T0e, T0r = m0._engine.get_tables()
    Xi = m0.data_indexer.get_indexes(X).astype(np.int32)
    runs = {}
    for name, reg in (("none", None), ("n3", n3), ("pair", [BatchLPRegularizer(2, LAM, "float"), None]), ("zero", BatchLPRegularizer(3, 0.0))):
        m = _fit(model, reg, negatives, loss)
        h = m.fit(X, batch_size=len(X), epochs=1, verbose=False)
        assert np.array_equal(m.data_indexer.get_indexes(X), Xi)
        runs[name] = (m._engine.get_tables(), float(h.history["loss"][0]), m)
    (Tae, Tar), La, _ = runs["none"]
    norm_e = BR.NORMS[n3.norm_for(model, "ent")]
    norm_r = BR.NORMS[n3.norm_for(model, "rel")]
    k = 10
    for name, terms in (("n3", (3, LAM, norm_e, 3, LAM, norm_r)), ("pair", (2, LAM, BR.FLOAT, 2, 0.0, BR.FLOAT))):
        (Tbe, Tbr), Lb, _ = runs[name]
        wR, wGe, wGr = BR.batch_reg(model, k, T0e, T0r, Xi, *terms)
        assert np.abs(wGe).max() > 1e-3 and wR > 1e-3                                  # (the regulariser is no rounding error here)
        for T0, Ta, Tb, w in ((T0e, Tae, Tbe, wGe), (T0r, Tar, Tbr, wGr)):
            diff = Ta.astype(np.float64) - Tb.astype(np.float64)
            bound = _bound(T0, Ta, Tb, T0.astype(np.float64) - Ta.astype(np.float64), w)
            err = np.abs(diff - w)
            print(name, model, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()), "max |reg grad|", float(np.abs(w).max()))
            assert (err <= bound).all(), (name, float((err / bound).max()))
        assert abs((Lb - La) - wR) <= 1e-6 * wR + 2e-5 * max(1.0, abs(La)), (name, La, Lb, wR)
    # lambda == 0 is the fit without a regulariser -- not bitwise: both paths accumulate with unordered atomics
    (Tze, Tzr), Lz, _ = runs["zero"]
    for T0, Ta, Tz in ((T0e, Tae, Tze), (T0r, Tar, Tzr)):
        Gd = T0.astype(np.float64) - Ta.astype(np.float64)
        assert (np.abs(Ta.astype(np.float64) - Tz) <= _bound(T0, Ta, Tz, Gd, np.zeros_like(Gd))).all()
    assert abs(Lz - La) <= 2e-5 * max(1.0, abs(La))


def test_save_and_restore_carry_the_regulariser(gpu_lib, tmp_path):
    """save_model -> restore_model: the restored model's config carries the pair, and one further step (one batch, SGD with rate 1)
    moves its tables as it moves the original's -- the same tables and a step without a draw (every entity is a negative, the object
    is the replaced side of every positive), unordered atomics: 2e-5 of the row's largest gradient plus the two tables' roundings
    (the bound of the test above without a regulariser difference)."""
    from test_gpu_model import toy_graph

    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer, LPRegularizer
    from ampligraph_amd.utils import restore_model, save_model

    X = toy_graph(seed=4, n=300, N=40, R=3)
    reg = [BatchLPRegularizer(3, LAM), LPRegularizer(2, 0.01)]
    sampler = {"shared": "all", "mask_known": True, "side": "o"}
    m = _fit("ComplEx", reg, sampler, "multiclass_nll")
    m.fit(X, batch_size=len(X), epochs=1, verbose=False)
    path = str(tmp_path / "model")
    save_model(m, path)
    r = restore_model(path)
    cfg = r.get_config()
    assert cfg == m.get_config() and cfg["entity_relation_regularizer"] == [{"kind": "batch", "p": 3, "lambda": LAM, "norm": "auto"},
                                                                            {"p": 2, "lambda": 0.01, "p2": 2, "lambda2": 0.0}]
    assert r._regularizers[0] == reg[0] and isinstance(r._regularizers[1], LPRegularizer) and r._regularizers[1].terms == [(2, 0.01)]
    T1 = m._engine.get_tables()
    assert all(np.array_equal(a, b) for a, b in zip(T1, r._engine.get_tables()))
    # (restore_model compiles without the sampler -- it is no part of a checkpoint: the further step of both is given it again)
    from ampligraph_amd.latent_features.negatives import NegativeSampling

    r._negatives = NegativeSampling.get(sampler)
    for mm in (m, r):
        mm.fit(X, batch_size=len(X), epochs=1, verbose=False)
    for T, a, b in zip(T1, m._engine.get_tables(), r._engine.get_tables()):
        G = T.astype(np.float64) - a
        assert np.abs(G).max() > 1e-3
        assert (np.abs(a.astype(np.float64) - b) <= _bound(T, a, b, G, np.zeros_like(G))).all()


def test_fit_refuses_focuse_with_a_batch_regulariser(gpu_lib):
    from test_gpu_model import toy_graph

    X = toy_graph(seed=4, n=60, N=20, R=3)
    Xw = np.concatenate([X.astype(object), np.random.default_rng(0).random((len(X), 1)).astype(object)], 1)
    m = _fit("ComplEx", "N3", None, "nll")
    with pytest.raises(NotImplementedError, match="FocusE"):
        m.fit(Xw, batch_size=30, epochs=1, verbose=False, focusE=True)
