"""GPU parity tests proper: every HIP entry point of libamdkge (called through the C ABI) against the
CPU oracle on the same seeded inputs.  Tolerances: fp32 outputs within 1e-5 relative (north_star);
integer outputs (corruptions, ranks) bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from margins import rel_gap, within
from oracle import kge_oracle as O

pytestmark = pytest.mark.gpu

MODELS = list(O.MODELS)
LOSSES = list(O.LOSS_DEFAULTS)


def make_engine(model, k, N, R, seed=0, scale=None, pad=True):
    """pad=True: the product's stored layout (halves padded to a multiple of 4 units, every k on the 16-byte kernels);
    pad=False: dense rows through the same ABI (k % 4 != 0 then takes the scalar-load kernels)."""
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(model, k, N, R, max_rel_size=R, pad=pad)
    rng = np.random.default_rng(seed)
    K = eng.K
    if scale is None:
        ent = O.glorot_uniform(N, K, rng)
        rel = O.glorot_uniform(R, K, rng)
    else:
        ent = (rng.normal(size=(N, K)) * scale).astype(np.float32)
        rel = (rng.normal(size=(R, K)) * scale).astype(np.float32)
    eng.set_tables(ent, rel)
    return eng, ent, rel


def dense(eng, t):
    """device tensor of stored rows -> dense numpy rows (what the oracle speaks)"""
    return eng.unpack(t).cpu().numpy()


def rand_triples(rng, n, N, R):
    return np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def loss_desc(name, reduction="sum", **kw):
    from ampligraph_amd import _ffi

    prm = dict(O.LOSS_DEFAULTS[name])
    prm.update(kw)
    return _ffi.Loss(_ffi.LOSSES[name], 1 if reduction == "mean" else 0, float(prm.get("margin", 0.0)),
                     float(prm.get("alpha", 0.0)))


# -------------------------------------------------------------------------------- wave reduction
def test_library_loaded(gpu_lib):
    from ampligraph_amd import _ffi

    assert gpu_lib.amdkge_abi_version() == _ffi.ABI_VERSION == 5   # (include/amdkge.h AMDKGE_ABI_VERSION)
    c = C.c_int(0)
    assert gpu_lib.amdkge_device_count(C.byref(c)) == 0 and c.value >= 1


# -------------------------------------------------------------------------------- predict (a20)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", [3, 50, 200, 350, 1000])
def test_score_parity(gpu_lib, model, k):
    N, R, n = 500, 7, 1001
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5 if k < 100 else 0.1)
    rng = np.random.default_rng(1)
    X = rand_triples(rng, n, N, R)
    got = eng.score(dev(X)).cpu().numpy()
    s, p, o = O.lookup(ent, rel, X)
    ref = O.compute_scores(model, s, p, o, max_rel_size=R)
    # relative to the score, floored at a fraction of the typical score magnitude (fp32 summation error is
    # relative to sum|terms|, so scores that cancel to ~0 cannot be held to 1e-5 of themselves)
    scale = np.maximum(np.abs(ref), 0.05 * np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
    assert np.max(np.abs(got - ref) / scale) < 1e-5, (model, k)


@pytest.mark.parametrize("model", MODELS)
def test_score_reference_kat(gpu_lib, model):
    """The reference's own score KATs (test_{TransE,DistMult,ComplEx,HolE,RotatE}.py) through the HIP path."""
    from kat_data import EXPECTED, _cplx_triples, _real_triples
    from ampligraph_amd.engine import KgeEngine

    cplx = model in ("ComplEx", "HolE", "RotatE")
    s, p, o = _cplx_triples() if cplx else _real_triples(model)
    k = 3 if cplx else 7
    eng = KgeEngine(model, k, 4, 2, max_rel_size=2)
    eng.set_tables(np.concatenate([s, o]), p)
    X = np.array([[0, 0, 2], [1, 1, 3]], dtype=np.int32)
    got = np.around(eng.score(dev(X)).cpu().numpy(), 2)
    assert (got == EXPECTED[model]).all(), (model, got)


# -------------------------------------------------------------------------------- sampling (a3)
@pytest.mark.parametrize("B,eta,N", [(1, 1, 1), (7, 3, 10), (1000, 20, 14505), (333, 64, 50_000_000)])
def test_sampler_bit_exact(gpu_lib, B, eta, N):
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine("DistMult", 4, max(N, 2), 3)
    rng = np.random.default_rng(2)
    X = rand_triples(rng, B, max(N, 2), 3)
    got = eng.sample_corruptions(dev(X), eta, seed=12345678901234, step=(1 << 33) + 5, sample_range=N,
                                 row_offset=17, b_global=B + 40).cpu().numpy()
    ref = O.generate_corruptions(X, N, eta, 12345678901234, (1 << 33) + 5, row_offset=17, b_global=B + 40)
    assert (got == ref).all()


# -------------------------------------------------------------------------------- train fwd/bwd
def run_fwdbwd(eng, X, eta, loss_name, reduction, seed, step, negs=None):
    B = X.shape[0]
    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    ps = torch.empty(B, dtype=torch.float32, device="cuda")
    ns = torch.empty(B * eta, dtype=torch.float32, device="cuda")
    eng.train_fwdbwd(dev(X), eta, loss_desc(loss_name, reduction), seed, step,
                     neg_override=None if negs is None else dev(negs), pos_scores=ps, neg_scores=ns)
    torch.cuda.synchronize()
    return (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel),
            ps.cpu().numpy(), ns.cpu().numpy())


def assert_grads_close(G, T, tol=2e-5):
    T = T.astype(np.float64)
    # row-wise scale: atomics reorder fp32 sums, so compare against the row's magnitude
    scale = np.maximum(np.abs(T).max(axis=1, keepdims=True), 1e-6 * max(np.abs(T).max(), 1e-30))
    err = np.abs(G - T) / scale
    assert err.max() < tol, err.max()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_train_fwdbwd_parity(gpu_lib, model, loss):
    N, R, k, B, eta = 300, 5, 32, 257, 6
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    rng = np.random.default_rng(3)
    X = rand_triples(rng, B, N, R)
    for reduction in ("sum", "mean"):
        L, Ge, Gr, ps, ns = run_fwdbwd(eng, X, eta, loss, reduction, seed=9, step=4)
        negs = O.generate_corruptions(X, N, eta, 9, 4)
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, reduction, R)
        assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L)), (L, float(total))
        assert_grads_close(Ge, Te)
        assert_grads_close(Gr, Tr)


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("model,k", [("TransE", 50), ("TransE", 7), ("DistMult", 400), ("ComplEx", 200),
                                       ("ComplEx", 350), ("HolE", 100), ("RotatE", 1000), ("RotatE", 33),
                                       ("ComplEx", 1024), ("DistMult", 2048), ("RotatE", 350), ("HolE", 50)])
def test_train_fwdbwd_geometries(gpu_lib, model, k, pad):
    """Every slot geometry (W waves x CH quads, VEC 1/2/4) against the oracle, incl. a ragged tail block; dense rows
    and the padded stored layout (RotatE's padding units must yield exact zero gradients, not 0/0)."""
    N, R, B, eta = 200, 4, 37, 5
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3 if k < 100 else 0.08, pad=pad)
    rng = np.random.default_rng(4)
    X = rand_triples(rng, B, N, R)
    L, Ge, Gr, ps, ns = run_fwdbwd(eng, X, eta, "self_adversarial", "sum", seed=1, step=0)
    negs = O.generate_corruptions(X, N, eta, 1, 0)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, "self_adversarial", None, "sum", R)
    assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
    assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
    assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L))
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


@pytest.mark.parametrize("k,eta", [(132, 200), (8, 700)])
def test_train_fwdbwd_large_lds(gpu_lib, k, eta):
    """The dense step above 64 KB of dynamic LDS: launch_train_w (kge_train.hip) has to raise the kernel's limit first, once per
    device.  TransE, one wave per positive, LDS = 4 slot_lds_bytes(eta, 1) + 32 [+ 16 K + 256 eta in the 16-byte layout]:
    k = 132 (the 16-byte layout starts above 128 units), eta = 200: 72 672 B; k = 8 (one unit per lane), eta = 700: 67 360 B.
    Two steps on one device -- the second finds the limit already raised -- each against the oracle."""
    slot = ((eta + 1) * 6 * 4 + 8 + 7) & ~7   # slot_lds_bytes(eta, 1), kge_train_common.h
    assert 64 * 1024 < 4 * slot + 32 + (16 * k + 256 * eta if k > 128 else 0) <= 150 * 1024
    N, R, B = 300, 4, 8
    eng, ent, rel = make_engine("TransE", k, N, R, scale=0.3 if k < 100 else 0.08)
    rng = np.random.default_rng(6)
    X = rand_triples(rng, B, N, R)
    for step in (0, 1):
        L, Ge, Gr, ps, ns = run_fwdbwd(eng, X, eta, "self_adversarial", "sum", seed=2, step=step)
        negs = O.generate_corruptions(X, N, eta, 2, step)
        total, Te, Tr, (sp, sn, per) = O.dense_gradients("TransE", ent, rel, X, negs, eta, "self_adversarial", None, "sum", R)
        assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L))
        assert_grads_close(Ge, Te)
        assert_grads_close(Gr, Tr)


def test_train_neg_override_and_duplicates(gpu_lib):
    """Identity corruptions, s == o triples and heavy row duplication (gradient dedup = sum)."""
    N, R, k, eta = 5, 2, 8, 4
    eng, ent, rel = make_engine("ComplEx", k, N, R, scale=0.7)
    X = np.array([[0, 0, 0], [1, 1, 1], [0, 0, 1], [0, 0, 1], [2, 1, 2]], dtype=np.int32)
    negs = np.tile(X, (eta, 1))
    negs[::2, 2] = 3          # object replaced
    negs[1::2, 0] = X[np.arange(1, len(negs), 2) % len(X), 0]  # identity corruption (subject "replaced" by itself)
    L, Ge, Gr, ps, ns = run_fwdbwd(eng, X, eta, "multiclass_nll", "sum", 0, 0, negs=negs)
    total, Te, Tr, _ = O.dense_gradients("ComplEx", ent, rel, X, negs, eta, "multiclass_nll", None, "sum", R)
    assert abs(L - float(total)) <= 1e-5 * max(1.0, abs(L))
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


# -------------------------------------------------------------------------------- owner-computes step
def run_tiled_grads(eng, X, eta, loss_name, reduction, seed, step, negs=None, pos_atomic=False):
    """amdkge_train_step_tiled in its gradient-only form: g_ent is STORED, g_rel accumulated."""
    from ampligraph_amd import _ffi

    eng.prepare_training("adam")
    eng.loss_acc.zero_()
    B = X.shape[0]
    ps = torch.empty(B, dtype=torch.float32, device="cuda")
    ns = torch.empty(B * eta, dtype=torch.float32, device="cuda")
    d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, 0.0, 1)
    if not pos_atomic:
        eng.g_ent.fill_(123.0)   # staged positives: every row is overwritten
    eng.train_step_tiled(dev(X), eta, loss_desc(loss_name, reduction), d, seed, step, grad_only=True, pos_atomic=pos_atomic,
                         neg_override=None if negs is None else dev(negs), pos_scores=ps, neg_scores=ns)
    torch.cuda.synchronize()
    return (float(eng.loss_acc[0].item()), dense(eng, eng.g_ent), dense(eng, eng.g_rel),
            ps.cpu().numpy(), ns.cpu().numpy())


@pytest.mark.parametrize("pos_atomic", [False, True])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("loss", LOSSES)
def test_tiled_gradients_parity(gpu_lib, model, loss, pos_atomic):
    """Bucketed owner-computes backward == oracle dense gradients (all models x losses x reductions; positives' own
    rows staged or through atomics)."""
    N, R, k, B, eta = 300, 5, 32, 257, 6
    eng, ent, rel = make_engine(model, k, N, R, scale=0.6)
    assert eng.tiled_supported(B, eta)
    rng = np.random.default_rng(3)
    X = rand_triples(rng, B, N, R)
    for reduction in ("sum", "mean"):
        L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, loss, reduction, seed=9, step=4, pos_atomic=pos_atomic)
        negs = O.generate_corruptions(X, N, eta, 9, 4)
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, reduction, R)
        assert np.allclose(ps, sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L))
        assert_grads_close(Ge, Te)
        assert_grads_close(Gr, Tr)


@pytest.mark.parametrize("k", [32, 50, 300])   # 50: padded rows (the padding units are exact zeros of another kind)
@pytest.mark.parametrize("loss", ["self_adversarial", "pairwise"])
def test_tiled_transe_exact_zero_units(gpu_lib, k, loss):
    """TransE with tables on a coarse grid: s + p - o is EXACTLY zero in many units, where the gradient of |.| is 0
    (sign(0) = 0, the oracle's and the reference's convention).  The single-pass forward kernel and the sign codes it hands
    to the tile pass take their exact forms for such rows / entries; gradients == oracle."""
    from ampligraph_amd.engine import KgeEngine

    N, R, B, eta = 120, 3, 200, 7
    eng = KgeEngine("TransE", k, N, R, max_rel_size=R)
    rng = np.random.default_rng(12)
    ent = (rng.integers(-2, 3, size=(N, k)) * 0.25).astype(np.float32)
    rel = (rng.integers(-1, 2, size=(R, k)) * 0.25).astype(np.float32)
    eng.set_tables(ent, rel)
    X = rand_triples(rng, B, N, R)
    negs = O.generate_corruptions(X, N, eta, 5, 2)
    s, p, o = O.lookup(ent, rel, negs)
    assert 0.05 < np.mean((s + p - o) == 0) < 0.9          # the case is what it claims to be
    L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, loss, "sum", seed=5, step=2)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients("TransE", ent, rel, X, negs, eta, loss, None, "sum", R)
    assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
    assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L))
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


@pytest.mark.parametrize("model,k,N", [("ComplEx", 200, 700), ("DistMult", 400, 5000), ("ComplEx", 352, 300),
                                         ("TransE", 52, 40000), ("RotatE", 260, 200), ("HolE", 100, 64),
                                         ("DistMult", 4, 3), ("TransE", 512, 1000),
                                         # one positive per workgroup (k > 512): 1 and 2 quads per lane, ragged rows
                                         ("RotatE", 1000, 300), ("ComplEx", 1024, 150), ("DistMult", 2048, 90),
                                         ("TransE", 600, 200), ("HolE", 516, 64), ("TransE", 2044, 50),
                                         # k % 4 != 0: the stored layout pads each half to a multiple of 4 units
                                         ("TransE", 7, 300), ("TransE", 50, 14505), ("DistMult", 350, 500), ("ComplEx", 350, 700),
                                         ("HolE", 350, 200), ("RotatE", 350, 300), ("RotatE", 33, 100), ("ComplEx", 50, 2000),
                                         ("ComplEx", 3, 40), ("RotatE", 1001, 120), ("DistMult", 2047, 60)])
def test_tiled_geometries(gpu_lib, model, k, N):
    """1 and 2 quads per lane, one-row tiles, tiles larger than the table, ragged last tile, padded halves."""
    R, B, eta = 4, 37, 5
    eng, ent, rel = make_engine(model, k, N, R, scale=0.3 if k < 100 else 0.08)
    rng = np.random.default_rng(4)
    X = rand_triples(rng, B, N, R)
    L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, "self_adversarial", "sum", seed=1, step=0)
    negs = O.generate_corruptions(X, N, eta, 1, 0)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, "self_adversarial", None, "sum", R)
    assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L))
    assert_grads_close(Ge, Te)
    assert_grads_close(Gr, Tr)


def test_tiled_unsupported_shapes(gpu_lib):
    from ampligraph_amd import _ffi

    assert make_engine("DistMult", 6, 50, 3, scale=0.1)[0].tiled_supported(10, 2)   # padded to 8 units by the engine
    for model, k in (("DistMult", 6), ("ComplEx", 2052), ("TransE", 7)):
        eng, _, _ = make_engine(model, k, 50, 3, scale=0.1, pad=False)   # dense rows: the ABI's own limits
        assert not eng.tiled_supported(10, 2)
        eng.prepare_training("sgd")
        with pytest.raises(_ffi.AmdKgeError):
            eng._twork = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
            _ffi.check(eng.lib.amdkge_train_step_tiled(
                C.byref(eng.model), C.byref(loss_desc("nll")), C.byref(_ffi.Opt(0, 2, 1e-2, .9, .999, 1e-7, 0.0, 1)),
                eng.ent.data_ptr(), eng.rel.data_ptr(), None, None, None, None, 0.0,
                dev(np.zeros((10, 3), np.int32)).data_ptr(), 10, 2,
                0, 50, 0, 0, 0, 0, None, eng.g_ent.data_ptr(), eng.g_rel.data_ptr(), 1, 0, eng.loss_acc.data_ptr(), None, None, None,
                eng._twork.data_ptr(), None))


@pytest.mark.parametrize("pos_atomic", [False, True])
@pytest.mark.parametrize("model", ["ComplEx", "TransE"])
def test_tiled_overflow_buckets_and_duplicates(gpu_lib, model, pos_atomic):
    """Every positive shares one subject (its tile's bucket overflows into the shared list), s == o triples,
    identity corruptions, inactive margins (g == 0 entries are skipped)."""
    N, R, k, eta, B = 300, 3, 16, 2, 3000
    eng, ent, rel = make_engine(model, k, N, R, scale=0.4)
    rng = np.random.default_rng(8)
    X = rand_triples(rng, B, N, R)
    X[:, 0] = 7
    X[::5, 2] = 7
    negs = O.generate_corruptions(X, N, eta, 5, 2)
    negs[:B // 2] = X[:B // 2]
    negs[:B // 2, 2] = 11   # first half of the j = 0 corruptions: object replaced by one hot row
    for loss in ("pairwise", "nll"):
        L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, loss, "sum", 5, 2, negs=negs, pos_atomic=pos_atomic)
        total, Te, Tr, _ = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, "sum", R)
        assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L))
        assert_grads_close(Ge, Te, tol=1e-4)   # thousands of fp32 terms per hot row, unordered
        assert_grads_close(Gr, Tr, tol=1e-4)


@pytest.mark.parametrize("pos_atomic", [False, True])
@pytest.mark.parametrize("opt", ["adam", "adagrad", "sgd", "sgd+momentum", "rmsprop", "rmsprop+momentum", "adadelta", "adamax"])
@pytest.mark.parametrize("model,reg", [("ComplEx", None), ("DistMult", (2, 1e-3)), ("RotatE", (3, 1e-2)), ("TransE", None)])
def test_tiled_step_in_place_parity(gpu_lib, opt, model, reg, pos_atomic):
    """Whole owner-computes steps (tables + slots updated from LDS) == oracle train_step, 3 steps."""
    from ampligraph_amd import _ffi

    N, R, k, B, eta = 150, 4, 12, 200, 4
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
    w, mk = make_optimizer(opt.split("+")[0], {"momentum": 0.7} if "+" in opt else {})
    opt = w.name
    eng.prepare_training(opt)
    st = mk(ent, rel)
    rng = np.random.default_rng(6)
    oreg = None if reg is None else dict(p=reg[0], lam_e=reg[1], lam_r=reg[1])
    lam = reg[1] if reg else 0.0
    for t in range(1, 4):
        X = rand_triples(rng, B, N, R)
        eng.loss_acc.zero_()
        d = w.to_ffi(t, reg[0] if reg else 2)
        eng.train_step_tiled(dev(X), eta, loss_desc("self_adversarial"), d, 77, t, reg_e=lam, reg_r=lam, pos_atomic=pos_atomic)
        assert float(eng.g_rel.abs().max()) == 0.0   # relation gradient consumed by the fused / trailing sweep
        assert float(eng.g_ent.abs().max()) == 0.0   # the positives' own rows were folded in and reset by the tiles
        ref_loss = float(O.train_step(st, model, X, eta, "self_adversarial", 77, t, max_rel_size=R, reg=oreg))
        torch.cuda.synchronize()
        got_loss = float(eng.loss_acc[0].item()) + float(eng.loss_acc[1].item())
        assert abs(got_loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (t, got_loss, ref_loss)
        e, r = eng.get_tables()
        # Adam's m/(sqrt(v)+eps) amplifies fp32 summation-order noise where g ~ 0: compare the bulk tightly
        ce = np.abs(e - st.ent) <= 1e-5 + 1e-4 * np.abs(st.ent)
        cr = np.abs(r - st.rel) <= 1e-5 + 1e-4 * np.abs(st.rel)
        assert ce.mean() > 0.995 and cr.mean() > 0.99, (opt, model, t, ce.mean(), cr.mean())
        assert np.abs(e - st.ent).max() < 2.5e-2   # a sign flip of a ~0 gradient moves Adam by at most 2*lr
        for nme in st.slots:
            # RMSprop-with-momentum's lr*g/sqrt(r + eps) is as ill-conditioned at g ~ 0 as Adam's update: bulk comparison
            # (elements that cancel to ~0 carry the absolute noise of their terms: floor relative to the tensor's magnitude)
            ok = np.isclose(dense(eng, eng.slots[nme]), st.slots[nme], rtol=1e-3, atol=1e-6 + 2e-5 * np.abs(st.slots[nme]).max())
            assert ok.mean() > (0.99 if opt == "rmsprop_mom" and nme.startswith("mom") else 0.9999), (nme, t, ok.mean())


# -------------------------------------------------------------------------------- optimizer (a17/a18)
OPT_SPECS = [("adam", {}), ("adagrad", {}), ("sgd", {}), ("sgd", {"momentum": 0.9}), ("sgd", {"momentum": 0.8, "nesterov": True}),
             ("rmsprop", {}), ("rmsprop", {"momentum": 0.5, "rho": 0.8}), ("adadelta", {}), ("adamax", {}),
             ("adam", {"beta_1": 0.8, "beta_2": 0.99, "epsilon": 1e-6})]


def make_optimizer(name, hp, lr=1e-2):
    """(product OptimizerWrapper, oracle TrainState factory) for one Keras optimizer spec."""
    from ampligraph_amd.latent_features import optimizers

    w = optimizers.get(name, dict(hp, learning_rate=lr))
    return w, (lambda ent, rel: O.TrainState(ent, rel, w.name, lr, **hp))


@pytest.mark.parametrize("name,hp", OPT_SPECS)
@pytest.mark.parametrize("reg", [None, (2, 1e-3), (3, 1e-2)])
def test_opt_step_parity(gpu_lib, name, hp, reg):
    """amdkge_opt_step == the oracle's Keras-legacy rules for every supported optimizer (descriptor built by the product's
    OptimizerWrapper.to_ffi, so the hyper-parameter mapping is covered), tables AND state tensors, 4 steps."""
    from ampligraph_amd import _ffi

    N, R, k = 123, 3, 9   # 123*9 is not a multiple of 4: exercises the scalar tail
    eng, ent, rel = make_engine("DistMult", k, N, R, scale=0.5, pad=False)
    w, mk = make_optimizer(name, hp)
    eng.prepare_training(w.name)
    st = mk(ent, rel)
    rng = np.random.default_rng(5)
    for t in range(1, 5):
        Ge = rng.normal(size=ent.shape) * (rng.random(size=ent.shape) < 0.3)
        Gr = rng.normal(size=rel.shape)
        eng.g_ent.copy_(dev(Ge.astype(np.float32)))
        eng.g_rel.copy_(dev(Gr.astype(np.float32)))
        eng.loss_acc.zero_()
        d = w.to_ffi(t, reg[0] if reg else 2)
        lam = reg[1] if reg else 0.0
        reg_loss = 0.0
        Ge32, Gr32 = Ge.astype(np.float32).astype(np.float64), Gr.astype(np.float32).astype(np.float64)
        if reg:
            for x, G in ((st.ent, Ge32), (st.rel, Gr32)):
                xx = x.astype(np.float64)
                reg_loss += lam * float((np.abs(xx) ** reg[0]).sum())
                G += lam * reg[0] * np.abs(xx) ** (reg[0] - 1) * np.sign(xx)
        eng.opt_step(d, lam, lam)
        O.apply_optimizer(st, Ge32, Gr32)
        torch.cuda.synchronize()
        e, r = eng.get_tables()
        assert np.abs(e - st.ent).max() <= 2e-6 * max(1.0, np.abs(st.ent).max()), (name, t)
        assert np.abs(r - st.rel).max() <= 2e-6 * max(1.0, np.abs(st.rel).max())
        assert float(eng.g_ent.abs().max()) == 0.0 and float(eng.g_rel.abs().max()) == 0.0  # gradient reset
        assert set(eng.slots) == set(st.slots) and len(st.slots) == 2 * len(_ffi.OPT_SLOTS[w.name])
        for nme, ref in st.slots.items():
            # (with a regulariser the test forms its gradient term in fp64, the kernel in fp32)
            assert np.allclose(eng.slots[nme].cpu().numpy(), ref, rtol=2e-5 if reg else 2e-6, atol=2e-7 * np.abs(ref).max()), (name, nme, t)
        if reg:
            assert abs(float(eng.loss_acc[1]) - reg_loss) <= 1e-5 * reg_loss
    with pytest.raises(ValueError):
        make_optimizer("adam", {"amsgrad": True})
    with pytest.raises(ValueError):
        make_optimizer("nadam", {})


# -------------------------------------------------------------------------------- ranks (a9-a11)
def dyadic_tables(rng, N, R, K):
    """Tables whose products/sums are exact in fp32 in any order -> bit-exact rank parity, many ties."""
    ent = (rng.integers(-4, 5, size=(N, K)) / 8.0).astype(np.float32)
    rel = (rng.integers(-4, 5, size=(R, K)) / 8.0).astype(np.float32)
    return ent, rel


def csr_filters(fl, n):
    lens = np.array([len(x) for x in fl], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.asarray(x, dtype=np.int32) for x in fl] + [np.zeros(0, np.int32)]).astype(np.int32)
    if ids.size == 0:
        ids = np.zeros(1, np.int32)
    return dev(off[:-1]), dev(off[1:]), dev(ids)


def gpu_ranks(eng, X, corrupt_side, strategy, fs=None, fo=None, subset=None):
    from ampligraph_amd import _ffi

    n = X.shape[0]
    Xd = dev(X)
    ent_ids = subset_pos = None
    if subset is not None:
        ent_ids = dev(np.asarray(subset, dtype=np.int32))
        pos = np.full(eng.n_ents, -1, dtype=np.int32)
        pos[np.asarray(subset)] = np.arange(len(subset), dtype=np.int32)
        subset_pos = dev(pos)
    cols = []
    if "s" in corrupt_side:
        flt = csr_filters(fs, n) if fs is not None else None
        cols.append(eng.rank_side(Xd, _ffi.SIDE_S, strategy, flt, ent_ids, subset_pos)[0])
    if "o" in corrupt_side:
        flt = csr_filters(fo, n) if fo is not None else None
        cols.append(eng.rank_side(Xd, _ffi.SIDE_O, strategy, flt, ent_ids, subset_pos)[0])
    r = torch.stack(cols, 1).cpu().numpy()
    if corrupt_side == "s+o":
        r = r.sum(1, keepdims=True) - 1
    return r


def test_ranks_reference_kat(gpu_lib):
    """test_AbstractScoringLayer.py:15-53 through the HIP path (values there are 0-based; +1 here)."""
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine("DistMult", 3, 4, 2)
    eng.set_tables(np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]], np.float32),
                   np.array([[10, 10, 10], [100, 100, 100]], np.float32))
    X = np.array([[0, 0, 2], [1, 1, 3]], dtype=np.int32)
    assert (gpu_ranks(eng, X, "s,o", "worst") == np.array([[4, 2], [3, 1]]) + 1).all()
    fs, fo = [[0], [1]], [[2], [3]]
    assert (gpu_ranks(eng, X, "s,o", "worst", fs, fo) == np.array([[3, 1], [2, 0]]) + 1).all()
    assert (gpu_ranks(eng, X, "s", "worst", fs, None) == np.array([[3], [2]]) + 1).all()
    assert (gpu_ranks(eng, X, "o", "worst", None, fo) == np.array([[1], [0]]) + 1).all()


@pytest.mark.parametrize("model", ["TransE", "DistMult", "ComplEx", "HolE"])
@pytest.mark.parametrize("strategy", ["worst", "best", "middle"])
def test_ranks_bit_exact_dyadic(gpu_lib, model, strategy):
    from ampligraph_amd.engine import KgeEngine

    rng = np.random.default_rng(6)
    N, R, k, n = 777, 5, 12, 301
    K = O.internal_k(model, k)
    ent, rel = dyadic_tables(rng, N, R, K)
    eng = KgeEngine(model, k, N, R)
    eng.set_tables(ent, rel)
    X = rand_triples(rng, n, N, R)
    train = rand_triples(rng, 4000, N, R)
    fs, fo = O.filter_sets(X, [train, X])
    for side in ("s,o", "s", "o", "s+o"):
        ref = O.evaluate_ranks(model, ent, rel, X, fs if "s" in side else None, fo if "o" in side else None,
                               side, strategy)
        got = gpu_ranks(eng, X, side, strategy, fs if "s" in side else None, fo if "o" in side else None)
        assert (got == ref).all(), (model, strategy, side, np.abs(got - ref).max())
    ref = O.evaluate_ranks(model, ent, rel, X, None, None, "s,o", strategy)
    assert (gpu_ranks(eng, X, "s,o", strategy) == ref).all()


@pytest.mark.parametrize("model", ["DistMult", "TransE"])
def test_ranks_entities_subset(gpu_lib, model):
    from ampligraph_amd.engine import KgeEngine

    rng = np.random.default_rng(7)
    N, R, k, n = 300, 3, 8, 100
    ent, rel = dyadic_tables(rng, N, R, O.internal_k(model, k))
    eng = KgeEngine(model, k, N, R)
    eng.set_tables(ent, rel)
    X = rand_triples(rng, n, N, R)
    subset = rng.permutation(N)[:97]
    fs, fo = O.filter_sets(X, [X, rand_triples(rng, 3000, N, R)])
    ref = O.evaluate_ranks(model, ent, rel, X, fs, fo, "s,o", "worst", entities_subset=subset)
    got = gpu_ranks(eng, X, "s,o", "worst", fs, fo, subset=subset)
    assert (got == ref).all()


@pytest.mark.parametrize("model,k", [("TransE", 50), ("DistMult", 400), ("ComplEx", 200), ("HolE", 30),
                                       ("RotatE", 40), ("RotatE", 7)])
def test_ranks_random_fp32(gpu_lib, model, k):
    """Non-exact inputs: ranks may differ from the fp64-accumulated oracle only on comparisons that are
    fragile under fp32 summation-order noise; the bound is checked per triple, MRR within 2e-3."""
    N, R, n = 1500, 6, 200
    eng, ent, rel = make_engine(model, k, N, R, scale=0.4)
    rng = np.random.default_rng(8)
    X = rand_triples(rng, n, N, R)
    fs, fo = O.filter_sets(X, [X, rand_triples(rng, 20000, N, R)])
    ref = O.evaluate_ranks(model, ent, rel, X, fs, fo, "s,o", "worst", max_rel_size=R)
    got = gpu_ranks(eng, X, "s,o", "worst", fs, fo)
    for c, side in enumerate(("s", "o")):
        frag = O.fragile_rank_mask(model, ent, rel, X, side, max_rel_size=R)
        diff = np.abs(got[:, c] - ref[:, c])
        assert (diff <= 2 * frag).all(), (model, side, diff.max(), frag[diff > 0])
    assert (got != ref).mean() < 0.02
    assert abs(O.mrr_score(got) - O.mrr_score(ref)) < 2e-3


def test_rank_filter_consistent_with_tile_kernel(gpu_lib):
    """Filtering every entity must cancel the worst-case count exactly: the filter kernel reproduces the
    tile kernel's scores bit for bit (same k-ordered chain), for all four kernel modes."""
    rng = np.random.default_rng(9)
    for model, k in (("DistMult", 37), ("ComplEx", 200), ("TransE", 50), ("RotatE", 24)):
        N, R, n = 130, 3, 50
        eng, ent, rel = make_engine(model, k, N, R, scale=0.5)
        X = rand_triples(rng, n, N, R)
        allids = [np.arange(N, dtype=np.int32)] * n
        got = gpu_ranks(eng, X, "s,o", "worst", allids, allids)
        assert (got == 1).all(), (model, got.min(), got.max())


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("model,k,N,n", [("DistMult", 37, 130, 50), ("ComplEx", 200, 1000, 333), ("HolE", 66, 257, 129),
                                           ("DistMult", 400, 4100, 300), ("DistMult", 16, 300, 77), ("DistMult", 32, 300, 77),
                                           ("ComplEx", 24, 300, 200), ("ComplEx", 2, 150, 40), ("ComplEx", 350, 600, 150),
                                           ("DistMult", 50, 500, 100), ("HolE", 7, 200, 64)])
def test_rank_mfma_kernel_bitwise_equals_valu_kernel(gpu_lib, model, k, N, n, pad):
    """v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain: the MFMA tile kernels (the software-pipelined default for rows of
    whole float4s -- every k in the padded stored layout --, the first kernel otherwise / with amdkge_set_rank_kernel(2))
    must return exactly the (greater, equal) counts of the VALU tile kernel on random fp32 tables (ragged tiles, both
    sides, subset; rows of 4..800 units: one stage, a half-empty last stage, odd and even stage counts).  The padded and
    the dense layout must also agree with each other: padding units add exact zeros to the chain."""
    from ampligraph_amd import _ffi

    rng = np.random.default_rng(11)
    eng, ent, rel = make_engine(model, k, N, 5, scale=0.3, pad=pad)
    other, _, _ = make_engine(model, k, N, 5, scale=0.3, pad=not pad)
    X = rand_triples(rng, n, N, 5)
    sub = dev(np.sort(rng.choice(N, N // 3, replace=False)).astype(np.int32))
    try:
        for side in (_ffi.SIDE_S, _ffi.SIDE_O):
            for ent_ids in (None, sub):
                _ffi.check(gpu_lib.amdkge_set_rank_kernel(0))
                c_mfma = eng.rank_side(dev(X), side, "worst", ent_ids=ent_ids)[1].cpu().numpy()
                c_other = other.rank_side(dev(X), side, "worst", ent_ids=ent_ids)[1].cpu().numpy()
                _ffi.check(gpu_lib.amdkge_set_rank_kernel(2))
                c_mfma0 = eng.rank_side(dev(X), side, "worst", ent_ids=ent_ids)[1].cpu().numpy()
                _ffi.check(gpu_lib.amdkge_set_rank_kernel(1))
                c_valu = eng.rank_side(dev(X), side, "worst", ent_ids=ent_ids)[1].cpu().numpy()
                assert (c_mfma == c_valu).all(), (model, side, np.abs(c_mfma - c_valu).max())
                assert (c_mfma0 == c_valu).all(), (model, side, np.abs(c_mfma0 - c_valu).max())
                assert (c_other == c_valu).all(), (model, side, "padded vs dense layout")
                m = N if ent_ids is None else int(ent_ids.shape[0])
                assert (c_mfma.sum(1) <= m).all() and c_mfma.min() >= 0
    finally:
        gpu_lib.amdkge_set_rank_kernel(0)


# -------------------------------------------------------------------------------- FocusE (a23)
@pytest.mark.parametrize("nl", ["linear", "tanh", "sigmoid", "softplus"])
@pytest.mark.parametrize("model,k,path", [("ComplEx", 32, "tiled"), ("DistMult", 7, "atomic"), ("TransE", 32, "tiled"),
                                          ("RotatE", 16, "atomic"), ("HolE", 16, "tiled")])
def test_focuse_gradients_parity(gpu_lib, nl, model, k, path):
    """FocusE score transform + chain rule inside the fused kernels (single-pass, two-pass staged, atomic) == oracle."""
    from ampligraph_amd import _ffi

    N, R, B, eta = 120, 4, 150, 5
    # distance models: keep |score| ~ 1 so that tanh / sigmoid are not saturated (f' == 0 in fp32 otherwise)
    eng, ent, rel = make_engine(model, k, N, R, scale=0.5 if model in ("ComplEx", "DistMult", "HolE") else 0.03)
    rng = np.random.default_rng(12)
    X = rand_triples(rng, B, N, R)
    wmean = rng.random(B).astype(np.float32)
    beta = 0.37
    wd = dev(wmean)
    for loss in ("self_adversarial", "nll", "pairwise"):
        ld = loss_desc(loss)
        ld.focus_nonlinearity = _ffi.FOCUS_NONLINEARITY[nl]
        ld.focus_beta = beta
        ld.d_focus_w = wd.data_ptr()
        eng.prepare_training("adam")
        eng.loss_acc.zero_()
        ps = torch.empty(B, dtype=torch.float32, device="cuda")
        ns = torch.empty(B * eta, dtype=torch.float32, device="cuda")
        if path == "tiled":
            d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, 0.0, 1)
            eng.train_step_tiled(dev(X), eta, ld, d, 3, 7, grad_only=True, pos_scores=ps, neg_scores=ns)
        else:
            eng.train_fwdbwd(dev(X), eta, ld, 3, 7, pos_scores=ps, neg_scores=ns)
        torch.cuda.synchronize()
        negs = O.generate_corruptions(X, N, eta, 3, 7)
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, "sum", R,
                                                         focus=(wmean, beta, nl))
        assert np.allclose(ps.cpu().numpy(), sp, rtol=2e-5, atol=2e-5 * np.abs(sp).max()), (loss, nl)
        assert np.allclose(ns.cpu().numpy(), sn, rtol=2e-5, atol=2e-5 * np.abs(sn).max())
        L = float(eng.loss_acc[0].item())
        assert abs(L - float(per.astype(np.float64).sum())) <= 2e-5 * max(1.0, abs(L)), (loss, nl, L)
        assert_grads_close(dense(eng, eng.g_ent), Te, tol=4e-5)
        assert_grads_close(dense(eng, eng.g_rel), Tr, tol=4e-5)


@pytest.mark.parametrize("model", ["ComplEx", "TransE"])
@pytest.mark.parametrize("B,eta", [(1, 1), (3, 64), (5, 100), (2, 7)])
def test_train_edge_shapes(gpu_lib, model, B, eta):
    """One positive, one corruption, eta at and beyond the wave width (lane loops, side-sorted permutation over several
    ballots), batches smaller than a workgroup -- both fused paths against the oracle."""
    N, R, k = 40, 3, 16
    eng, ent, rel = make_engine(model, k, N, R, scale=0.4)
    rng = np.random.default_rng(B * 1000 + eta)
    X = rand_triples(rng, B, N, R)
    negs = O.generate_corruptions(X, N, eta, 2, 3)
    for loss in ("self_adversarial", "multiclass_nll", "pairwise"):
        total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, "mean", R)
        for path in ("atomic", "tiled"):
            if path == "atomic":
                L, Ge, Gr, ps, ns = run_fwdbwd(eng, X, eta, loss, "mean", 2, 3)
            else:
                L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, loss, "mean", 2, 3)
            assert np.allclose(ns, sn, rtol=1e-5, atol=1e-5 * max(np.abs(sn).max(), 1e-6)), (path, loss)
            assert abs(L - float(per.astype(np.float64).sum())) <= 2e-5 * max(1.0, abs(L)), (path, loss)
            assert_grads_close(Ge, Te, tol=4e-5)
            assert_grads_close(Gr, Tr, tol=4e-5)


def test_empty_inputs(gpu_lib):
    """Empty batches / test sets are no-ops with well-formed outputs (the reference's loaders can yield them)."""
    from ampligraph_amd import _ffi

    eng, ent, rel = make_engine("DistMult", 8, 20, 2, scale=0.3)
    empty = torch.empty(0, 3, dtype=torch.int32, device="cuda")
    assert eng.score(empty).shape[0] == 0
    r, c, s = eng.rank_side(empty, _ffi.SIDE_S, "worst")
    assert r.shape[0] == 0 and c.shape == (0, 2)
    eng.prepare_training("adam")
    eng.train_fwdbwd(empty, 3, loss_desc("nll"), 0, 0)
    assert float(eng.g_ent.abs().max()) == 0.0 and float(eng.loss_acc[0]) == 0.0
    before = eng.ent.clone()
    d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, 0.0, 1)
    eng.train_step_tiled(empty, 3, loss_desc("nll"), d, 0, 0)          # a zero-gradient Adam step: tables unchanged
    torch.cuda.synchronize()
    assert torch.equal(eng.ent, before)


def test_filter_ranges_kernel_equals_host_lookup(gpu_lib):
    """amdkge_filter_ranges (binary search per test triple on the device) == FilterIndex.subject_ranges / object_ranges
    (numpy searchsorted), including triples whose (p,o) / (s,p) key is absent and an empty index."""
    from ampligraph_amd.datasets.filters import FilterIndex

    rng = np.random.default_rng(21)
    N, R = 300, 7
    eng, _, _ = make_engine("DistMult", 8, N, R)
    X = rand_triples(rng, 4000, N, R)
    T = rand_triples(rng, 1000, N, R)
    T[:300] = X[rng.integers(0, len(X), 300)]
    for fi in (FilterIndex([X], N, R), FilterIndex([X[:1]], N, R), FilterIndex([], N, R)):
        for sd, fn in (("s", fi.subject_ranges), ("o", fi.object_ranges)):
            lo, hi = fn(T)
            l2, h2, ids = fi.device_filter(eng, dev(T), sd)
            assert np.array_equal(lo, l2.cpu().numpy()) and np.array_equal(hi, h2.cpu().numpy()), sd


def filter_range_case():
    """(X, T, N, R) for the range lookup of all three key forms at N = 57, R = 9: 300 filter triples with s, o in [1, N - 2] and
    p in [1, R - 2], (1, 1, 1) and (N - 2, R - 2, N - 2) among them -- the first and the last group of every form; 200 queries:
    70 copied from X, 126 random ones over the whole id range, then T[-4:] = a hit on the first group, a hit on the last group,
    (0, 0, 0) -- key 0, below the first key of every form -- and (N - 1, R - 1, N - 1), above the last."""
    rng = np.random.default_rng(57)
    N, R = 57, 9
    X = np.stack([rng.integers(1, N - 1, 298), rng.integers(1, R - 1, 298), rng.integers(1, N - 1, 298)], 1)
    X = np.concatenate([X, [[1, 1, 1], [N - 2, R - 2, N - 2]]]).astype(np.int32)
    T = np.concatenate([X[rng.integers(0, 298, 70)], rand_triples(rng, 126, N, R),
                        [[1, 1, 1], [N - 2, R - 2, N - 2], [0, 0, 0], [N - 1, R - 1, N - 1]]]).astype(np.int32)
    return X, T, N, R


def check_filter_range_case(keys, q, lo, hi):
    """the host side of filter_range_case for one key form (q: the queries' group keys): the case holds what it claims"""
    assert len(q) == 200 and keys.size > 0
    assert q[-4] == keys[0] and hi[-4] > lo[-4] and lo[-4] == 0            # hit on the first group
    assert q[-3] == keys[-1] and hi[-3] > lo[-3]                           # hit on the last group
    assert q[-2] < keys[0] and q[-1] > keys[-1] and hi[-2] == 0 and hi[-1] == 0
    assert 3 * int((hi == 0).sum()) >= len(q) and int((hi > lo).sum()) >= 72


def test_filter_index_built_on_device_equals_host_build(gpu_lib):
    """amdkge_filter_build (keys, radix sort, scan, scatter on the device) produces the very arrays of the host build
    (datasets/filters.py: numpy unique / searchsorted, itself pinned by the reference's KAT and the oracle's sets): group keys,
    CSR offsets and ids, for overlapping datasets (duplicates collapse), the reference's KAT, an empty index, one triple, and
    ids near the top of a 50 M-entity range (keys beyond 2^53)."""
    from ampligraph_amd.datasets.filters import FilterIndex

    eng, _, _ = make_engine("DistMult", 8, 16, 3)
    rng = np.random.default_rng(4)
    cases = []
    X = rand_triples(rng, 20000, 300, 7)
    cases.append(([X, X[:5000], rand_triples(rng, 3000, 300, 7)], 300, 7))
    cases.append(([np.array([[1, 1, 2], [1, 1, 3], [1, 1, 4], [5, 1, 3], [5, 1, 4], [6, 1, 3], [6, 1, 2], [6, 1, 4], [6, 1, 7]]),
                   np.array([[3, 1, 2], [4, 1, 3], [5, 1, 4], [5, 1, 2], [1, 1, 5]]), np.array([[3, 1, 6], [2, 1, 2], [1, 1, 6]])], 8, 2))
    cases.append(([], 8, 2))
    cases.append(([np.array([[7, 1, 0]])], 8, 2))
    N_big = 50_000_000
    big = np.stack([rng.integers(N_big - 1000, N_big, 5000), rng.integers(0, 1000, 5000), rng.integers(N_big - 50, N_big, 5000)], 1)
    cases.append(([big, big[:100]], N_big, 1000))
    for datasets, N, R in cases:
        host = FilterIndex(datasets, N, R)
        devi = FilterIndex(datasets, N, R, engine=eng)
        for nm in ("po_keys", "po_start", "s_ids", "sp_keys", "sp_start", "o_ids"):
            a, b = getattr(host, nm), getattr(devi, nm)
            assert a.shape == b.shape and np.array_equal(a, b), (nm, N, a[:5], b[:5])
        T = np.concatenate([np.asarray(d) for d in datasets])[:500] if datasets else rand_triples(rng, 10, N, R)
        for sd, fn in (("s", host.subject_ranges), ("o", host.object_ranges)):
            lo, hi = fn(T)
            l2, h2, ids = devi.device_filter(eng, dev(T.astype(np.int32)), sd)
            assert np.array_equal(lo, l2.cpu().numpy()) and np.array_equal(hi, h2.cpu().numpy()), sd
    # the one lookup kernel against the host ranges, both entity-side forms (the pair form: test_gpu_relation.py): misses, keys
    # outside the index, the first and the last group, and an index with no keys
    X, T, N, R = filter_range_case()
    host, devi, none = FilterIndex([X], N, R), FilterIndex([X], N, R, engine=eng), FilterIndex([], N, R, engine=eng)
    t = T.astype(np.int64)
    for sd, fn, keys, q in (("s", host.subject_ranges, host.po_keys, t[:, 1] * N + t[:, 2]), ("o", host.object_ranges, host.sp_keys, t[:, 0] * R + t[:, 1])):
        lo, hi = fn(T)
        check_filter_range_case(keys, q, lo, hi)
        l2, h2, _ = devi.device_filter(eng, dev(T), sd)
        assert np.array_equal(lo, l2.cpu().numpy()) and np.array_equal(hi, h2.cpu().numpy()), sd
        l0, h0, ids0 = none.device_filter(eng, dev(T), sd)
        assert l0.shape == (200,) and not l0.any().item() and not h0.any().item() and ids0.numel() >= 1, sd


@pytest.mark.parametrize("model,k", [("ComplEx", 16), ("TransE", 50), ("RotatE", 9), ("DistMult", 600)])
def test_tiled_hot_rows_parity(gpu_lib, model, k):
    """AMDKGE_TILED_HOT_ROWS: a few entities are the s / o of most positives; their own-row gradients go through replica rows
    (atomics spread over 16 rows, summed by the owning tile), everything else stays staged.  Gradient-only and in-place forms
    against the oracle, two steps on one workspace (the replicas must come back zero), then the feature switched off again."""
    from ampligraph_amd import _ffi

    N, R, eta, B = 300, 3, 3, 2000
    eng, ent, rel = make_engine(model, k, N, R, scale=0.4 if k < 100 else 0.05)
    rng = np.random.default_rng(8)
    X = rand_triples(rng, B, N, R)
    X[: B // 2, 0] = 7
    X[::5, 2] = 7
    X[1::7, 2] = 11
    eng.set_hot_rows([7, 11, 299])          # 299: declared hot but (almost) unused
    for loss in ("self_adversarial", "pairwise"):
        L, Ge, Gr, ps, ns = run_tiled_grads(eng, X, eta, loss, "sum", 5, 2)
        assert eng._last_tiled[2] & 4
        negs = O.generate_corruptions(X, N, eta, 5, 2)
        total, Te, Tr, _ = O.dense_gradients(model, ent, rel, X, negs, eta, loss, None, "sum", R)
        assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L))
        assert_grads_close(Ge, Te, tol=1e-4)   # thousands of fp32 terms per hot row, unordered
        assert_grads_close(Gr, Tr, tol=1e-4)
    # complete steps in place (dense and touched-rows optimizer)
    for lazy in (False, True):
        eng2, _, _ = make_engine(model, k, N, R, scale=0.4 if k < 100 else 0.05)
        eng2.set_hot_rows([7, 11])
        w, mk = make_optimizer("adam", {})
        w.lazy = lazy
        eng2.prepare_training(w.name)
        st = mk(ent, rel)
        for t in range(1, 3):
            Xt = X[rng.permutation(B)]
            eng2.loss_acc.zero_()
            eng2.train_step_tiled(dev(Xt), eta, loss_desc("self_adversarial"), w.to_ffi(t, 2), 77, t)
            ref_loss = float(O.train_step(st, model, Xt, eta, "self_adversarial", 77, t, max_rel_size=R, lazy=lazy))
            torch.cuda.synchronize()
            got_loss = float(eng2.loss_acc[0].item()) + float(eng2.loss_acc[1].item())
            assert abs(got_loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (t, got_loss, ref_loss)
            e, r = eng2.get_tables()
            # (a hot row sums ~1 000 fp32 terms in arrival order; where they cancel, Adam's m / sqrt(v) amplifies the noise)
            assert (np.abs(e - st.ent) <= 1e-5 + 1e-4 * np.abs(st.ent)).mean() > (0.94 if model == "TransE" else 0.97) and np.abs(e - st.ent).max() < 2.5e-2
    eng.set_hot_rows(None)
    L2, Ge2, _, _, _ = run_tiled_grads(eng, X, eta, "pairwise", "sum", 5, 2)
    assert not (eng._last_tiled[2] & 4) and within("kernels/hot_rows_off_vs_on/loss", rel_gap(L2, L), 1e-6)   # same tables, forward only
    assert_grads_close(Ge2, Te, tol=1e-4)
