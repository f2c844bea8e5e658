"""Shared-negative training without a GPU: what is the extension header's own (include/amdkge_shared.h; names and
types: tests/test_abi_host.py), the entry points' argument validation (returned before any device work), the numpy
restatement of the draw and of the step's definition (tests/shared_ref.py), SharedNegatives' validation and every refusal of
compile() that needs no device."""
import ctypes as C

import numpy as np
import pytest

import abi_decl
import shared_ref as SR
from ampligraph_amd._ffi import EINVAL, EUNSUPPORTED
from bound_samplers import bound
from oracle import kge_oracle as O

SEED, STEP = 12345678901234, (1 << 33) + 5


def _graph(seed, B, N, R):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ header and binding table
def test_extension_header_and_its_signature_table():
    from ampligraph_amd import _ffi

    text = abi_decl.text("amdkge_shared.h")
    assert _ffi.SHARED_MAX_NEGS == SR.MAX_NEGS == (1 << 24) - 1
    assert "0xF0 << 24" in text and "0xF1 << 24" in text and (SR.TAG_IDS, SR.TAG_SIDE) == (0xF0 << 24, 0xF1 << 24)


def _model(_ffi, name, k=8, N=50, R=4):
    return _ffi.Model(_ffi.SCORING_TYPES[name], k, N, R, R, 0, 0, 0)


def test_argument_validation_without_gpu():
    """Every error below is returned before any device work: the pointers that are set are never dereferenced."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)

    def draw(tri=X, B=5, G=2, M=3, base=0, rng=50, mode=SR.UNIFORM, thr=None, pool=None, pool_n=0, ids=X, side=X):
        return lib.amdkge_sample_shared(tri, B, G, M, base, rng, 1, 2, mode, thr, pool, pool_n, ids, side, None)

    assert draw(ids=None) == EINVAL and b"NULL" in lib.amdkge_last_error()
    assert draw(side=None) == EINVAL
    for bad in (dict(B=-1), dict(G=0), dict(M=0), dict(M=1 << 24), dict(mode=4), dict(mode=-1), dict(mode=SR.BERNOULLI), dict(mode=SR.BERNOULLI, thr=X, tri=None),
                dict(rng=0), dict(rng=1 << 32), dict(base=-1), dict(pool=X, pool_n=0), dict(pool=X, pool_n=1 << 32)):
        assert draw(**bad) == EINVAL, bad
    assert draw(B=0) == 0 and draw(B=0, tri=None) == 0                      # nothing to do

    ls = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)

    def step(model="ComplEx", loss=ls, ent=X, rel=X, tri=X, B=5, G=2, M=3, ids=X, side=X, ge=X, gr=X, acc=X, work=X):
        m = _model(_ffi, model)
        return lib.amdkge_train_shared_fwdbwd(C.byref(m), C.byref(loss) if loss is not None else None, ent, rel, tri, B, G, M, ids, side, ge, gr, acc, None, None,
                                              work, None)

    for model in ("TransE", "RotatE"):
        assert step(model=model) == EUNSUPPORTED and b"contraction" in lib.amdkge_last_error()
        assert lib.amdkge_train_shared_workspace_bytes(C.byref(_model(_ffi, model)), 5, 2, 3) == 0
    for bad in (dict(B=-1), dict(G=0), dict(G=-3), dict(M=0), dict(M=-1), dict(M=1 << 24), dict(loss=None), dict(ent=None), dict(rel=None), dict(ge=None),
                dict(gr=None), dict(acc=None), dict(tri=None), dict(ids=None), dict(side=None), dict(work=None)):
        assert step(**bad) == EINVAL, bad
    assert step(loss=_ffi.Loss(9, 0, 0.0, 0.0)) == EINVAL
    focus = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)
    focus.focus_nonlinearity, focus.d_focus_w = 1, 4096
    assert step(loss=focus) == EUNSUPPORTED and b"FocusE" in lib.amdkge_last_error()
    assert step(B=0, tri=None, ids=None, side=None, work=None) == 0         # nothing to do
    # the workspace: 0 for what the path does not take, otherwise Q, dQ, two floats per positive and a bounded score buffer
    for model, K in (("DistMult", 8), ("ComplEx", 16), ("HolE", 16)):
        m = _model(_ffi, model)
        for B, G, M in ((37, 5, 33), (1, 1, 1), (5, 100, 7)):
            need = lib.amdkge_train_shared_workspace_bytes(C.byref(m), B, G, M)
            assert 4 * (2 * B * K + 2 * B + min(B, -(-B // min(G, B)) * min(G, B)) * M) <= need <= 4 * (2 * B * K + 2 * B + B * M) + 5 * 256
        for B, G, M in ((0, 5, 3), (-1, 5, 3), (5, 0, 3), (5, 5, 0), (5, 5, 1 << 24)):
            assert lib.amdkge_train_shared_workspace_bytes(C.byref(m), B, G, M) == 0
        big = lib.amdkge_train_shared_workspace_bytes(C.byref(m), 100_000, 1024, 1024)   # B * M = 10^8 scores: the buffer holds 2^24 of them
        assert big <= 4 * (2 * 100_000 * K + 2 * 100_000 + (1 << 24)) + 5 * 256


# ------------------------------------------------------------------------------------------------------------ the draw and the definition
@pytest.mark.parametrize("B,G,M,N", [(1, 1, 1, 1), (37, 8, 5, 10), (1000, 256, 256, 14505), (5, 100, 3, 7)])
def test_draw_properties(B, G, M, N):
    X = _graph(0, B, max(N, 2), 5)
    ids, side = SR.sample_shared(X, G, M, SEED, STEP, sample_range=N)
    ng = SR.n_groups(B, G)
    assert ids.shape == (ng, M) and ids.dtype == np.int32 and side.shape == (B,) and side.dtype == np.int32
    assert ids.min() >= 0 and ids.max() < N and set(np.unique(side)) <= {0, 1}
    ids2, _ = SR.sample_shared(X, G, M, SEED, STEP, sample_base=3, sample_range=N)
    assert np.array_equal(ids2, ids + 3)                                    # base + mulhi(x, range)
    pool = np.array([N + 4, 0, N + 4, 2], dtype=np.int32)
    idp, sdp = SR.sample_shared(X, G, M, SEED, STEP, pool=pool)
    assert set(idp.ravel().tolist()) <= set(pool.tolist()) and np.array_equal(sdp, side)   # the side coin does not look at the pool
    # a pure function of (seed, step, group, j) and (seed, step, row): a longer batch extends the shorter one's draw
    Xl = np.concatenate([X, _graph(1, 2 * min(G, B), max(N, 2), 5)])
    if G <= B:                                                              # (G > B: the one group is the whole batch)
        idl, sdl = SR.sample_shared(Xl, G, M, SEED, STEP, sample_range=N)
        assert np.array_equal(idl[:ng], ids) and np.array_equal(sdl[:B], side)
    if B * M >= 64:
        other, oside = SR.sample_shared(X, G, M, SEED, STEP + 1, sample_range=N)
        assert not np.array_equal(other, ids) and not np.array_equal(oside, side)
        assert not np.array_equal(SR.sample_shared(X, G, M, SEED + 1, STEP, sample_range=N)[0], ids)
    # the definition: every positive of a group meets the group's list on its own side, nothing else changes
    rows = SR.override_rows(X, G, ids, side)
    assert rows.shape == (B * M, 3) and rows.dtype == np.int32
    r3 = rows.reshape(M, B, 3)
    Ge = min(G, B)
    for i in range(B):
        assert np.array_equal(r3[:, i, 1], np.full(M, X[i, 1]))
        assert np.array_equal(r3[:, i, 0 if side[i] else 2], ids[i // Ge])
        assert np.array_equal(r3[:, i, 2 if side[i] else 0], np.full(M, X[i, 2 if side[i] else 0]))


def test_side_modes():
    B, R = 4000, 3
    X = _graph(2, B, 50, R)
    assert SR.sample_shared(X, 16, 4, 1, 2, sample_range=50, side_mode=SR.S_ONLY)[1].tolist() == [1] * B
    assert SR.sample_shared(X, 16, 4, 1, 2, sample_range=50, side_mode=SR.O_ONLY)[1].tolist() == [0] * B
    uni = SR.sample_shared(X, 16, 4, 1, 2, sample_range=50)[1]
    assert abs(uni.mean() - 0.5) < 0.04                                     # 5 sigma of a fair coin over 4000 rows
    thr = np.array([0, 0xFFFFFFFF, 0x40000000], dtype=np.uint32)            # never / (almost) always / a quarter
    ber = SR.sample_shared(X, 16, 4, 1, 2, sample_range=50, side_mode=SR.BERNOULLI, side_thr=thr)[1]
    assert ber[X[:, 1] == 0].sum() == 0 and ber[X[:, 1] == 1].mean() == 1.0 and abs(ber[X[:, 1] == 2].mean() - 0.25) < 0.07
    # the ids do not depend on the side mode
    a = SR.sample_shared(X, 16, 4, 1, 2, sample_range=50, side_mode=SR.BERNOULLI, side_thr=thr)[0]
    assert np.array_equal(a, SR.sample_shared(X, 16, 4, 1, 2, sample_range=50, side_mode=SR.S_ONLY)[0])


def test_streams_differ_from_the_default_draw():
    """Same seed and step: neither the ids nor the side coin repeat what oracle.generate_corruptions (= amdkge_sample_corruptions, and
    try 0 of amdkge_sample_negatives) draws for the same rows."""
    B, M, N = 256, 16, 1 << 20
    X = _graph(3, B, N, 5)
    ids, side = SR.sample_shared(X, 1, M, SEED, STEP, sample_range=N)      # G = 1: a list per positive, like the default draw
    ref = O.generate_corruptions(X, N, M, SEED, STEP).reshape(M, B, 3)
    ref_subj = ref[:, :, 2] == X[None, :, 2]                                # (N = 2^20: an identity corruption is improbable)
    ref_repl = np.where(ref_subj, ref[:, :, 0], ref[:, :, 2])
    assert (ref_repl == ids.T).mean() < 0.01
    assert 0.3 < (ref_subj[0] == (side != 0)).mean() < 0.7
    # ... and the two streams of this draw differ from each other: x of the ids against x of the coin for the same index
    assert not np.array_equal(SR._philox_x(np.arange(64, dtype=np.uint32), np.uint32(SR.TAG_IDS), STEP, SEED),
                              SR._philox_x(np.arange(64, dtype=np.uint32), np.uint32(SR.TAG_SIDE), STEP, SEED))


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_shared_negatives_validation():
    from ampligraph_amd.latent_features.negatives import NegativeSampling, SharedNegatives

    d = SharedNegatives(64)
    assert (d.num_negs, d.group_size, d.side, d.entities, d.shared) == (64, 64, "uniform", None, True)
    ok = SharedNegatives(num_negs=48, group_size=20, side="bernoulli", entities=["a", "b"])
    assert (ok.num_negs, ok.group_size, ok.side, list(ok.entities)) == (48, 20, "bernoulli", ["a", "b"])
    for bad in (dict(num_negs=0), dict(num_negs=-1), dict(num_negs=1 << 24), dict(num_negs=2.0), dict(num_negs=True), dict(num_negs=None), dict(num_negs=4, group_size=0),
                dict(num_negs=4, group_size=1.5), dict(num_negs=4, group_size=False), dict(num_negs=4, side="both"), dict(num_negs=4, side=None),
                dict(num_negs=4, entities=[]), dict(num_negs=4, entities="abc"), dict(num_negs=4, entities=[["a"], ["b"]])):
        with pytest.raises(ValueError, match="negatives"):
            SharedNegatives(**bad)
    assert NegativeSampling.get(ok) is ok
    got = NegativeSampling.get({"shared": 32, "group_size": 8, "side": "o"})
    assert isinstance(got, SharedNegatives) and (got.num_negs, got.group_size, got.side) == (32, 8, "o")
    assert got.get_config() == {"shared": 32, "group_size": 8, "side": "o", "entities": None}
    again = NegativeSampling.get(got.get_config())
    assert (again.num_negs, again.group_size, again.side) == (32, 8, "o")
    assert NegativeSampling.get({"shared": 16, "filter": False}).group_size == 16
    with pytest.raises(ValueError, match="breaks the sharing"):
        NegativeSampling.get({"shared": 16, "filter": True})
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"shared": 16, "max_tries": 3})
    with pytest.raises(ValueError, match="num_negs"):
        NegativeSampling.get({"shared": 0})


def test_compile_takes_the_setting_and_refuses_what_it_cannot_run():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import SharedNegatives

    for model in ("DistMult", "ComplEx", "HolE"):
        m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=model)
        m.compile(optimizer="adam", loss="multiclass_nll", negatives=SharedNegatives(64, group_size=16))
        assert isinstance(m._negatives, SharedNegatives) and m._negatives.group_size == 16
        m.compile(optimizer="adam", loss="nll", negatives={"shared": 8})
        assert isinstance(m._negatives, SharedNegatives) and m._negatives.num_negs == 8
        m.compile(optimizer="adam", loss="nll")                            # compiled again without it: off again
        assert m._negatives is None
    for model in ("TransE", "RotatE"):
        m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=model)
        with pytest.raises(NotImplementedError, match="distance"):
            m.compile(optimizer="adam", loss="nll", negatives={"shared": 8})
        m.compile(optimizer="adam", loss="nll", negatives={"side": "o"})   # (the per-positive sampler still compiles)
    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="ComplEx")
    with pytest.raises(NotImplementedError, match="deterministic"):
        m.compile(optimizer="adam", loss="nll", negatives={"shared": 8}, deterministic=True)
    with pytest.raises(NotImplementedError, match="lazy"):
        m.compile(optimizer="adam", loss="nll", negatives={"shared": 8}, optimizer_mode="lazy")
    for sharding in ("rows", "columns"):
        with pytest.raises(NotImplementedError, match="entity_sharding"):
            m.compile(optimizer="adam", loss="nll", negatives={"shared": 8}, entity_sharding=sharding)
    with pytest.raises(ValueError, match="breaks the sharing"):
        m.compile(optimizer="adam", loss="nll", negatives={"shared": 8, "filter": True})


def test_step_loop_takes_the_shared_path_and_refuses_focus_ranks_and_determinism():
    import torch

    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    calls = []

    class Eng:
        scoring_type, k = "ComplEx", 8

        def prepare_training(self, name):
            pass

        def train_shared_fwdbwd(self, triples, G, M, ids, side, loss):
            calls.append(("shared", tuple(triples.shape), G, M, ids, side))

        def train_fwdbwd(self, *a, **kw):
            calls.append(("fwdbwd",))

        def opt_step(self, *a):
            calls.append(("opt",))

    loop = StepLoop(Eng(), 3, loss_functions.get("nll"), optimizers.get("adam"), None, seed=5, dist=None)
    loop.negatives = bound(loop.engine, "shared", calls)
    batch = torch.zeros(10, 3, dtype=torch.int32)
    loop.step(batch, 7)
    assert calls == [("draw", (10, 3), 5, 7), ("shared", (10, 3), 4, 6, "ids", "side"), ("opt",)] and loop.n_steps == 1
    with pytest.raises(NotImplementedError, match="FocusE"):
        loop.step(batch, 8, focus=(torch.zeros(10), 0.5, "linear"))
    loop.deterministic = True
    with pytest.raises(NotImplementedError, match="deterministic"):
        loop.step(batch, 9)
    loop.deterministic, loop.multi = False, True
    with pytest.raises(NotImplementedError, match="one rank"):
        loop.step(batch, 10)
    # without a shared sampler the loop runs what it ran before
    del calls[:]
    loop.multi, loop.negatives, loop.use_tiled = False, None, False
    loop.step(batch, 11)
    assert calls == [("fwdbwd",), ("opt",)]
