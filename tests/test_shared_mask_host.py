"""Masked shared negatives and the all-entities list without a GPU: what is the extension header's own
(include/amdkge_shared_mask.h; names and types: tests/test_abi_host.py), the argument validation of both entry
points (returned before any device work), SharedNegatives' new arguments, the step loop's choice of call, and the numpy
restatement of the mask (tests/shared_mask_ref.py) on a case written out by hand."""
import ctypes as C

import numpy as np
import pytest

import shared_mask_ref as MR
from ampligraph_amd._ffi import EINVAL, EUNSUPPORTED
from bound_samplers import bound
from oracle import kge_oracle as O



# ------------------------------------------------------------------------------------------------------------ header and binding table
def test_extension_header_and_its_signature_table():
    from ampligraph_amd import _ffi

    # the masked step's arguments are the unmasked step's, then the six range arrays, list_mode and d_stats, then the stream
    plain, masked = _ffi.ABI["amdkge_shared.h"]["amdkge_train_shared_fwdbwd"][1], _ffi.ABI["amdkge_shared_mask.h"]["amdkge_train_shared_masked_fwdbwd"][1]
    assert masked[:len(plain) - 1] == plain[:-1] and len(masked) == len(plain) + 8


def _model(_ffi, name, k=8, N=50, R=4):
    return _ffi.Model(_ffi.SCORING_TYPES[name], k, N, R, R, 0, 0, 0)


def test_argument_validation_without_gpu():
    """Every error below is returned before any device work: the pointers that are set are never dereferenced."""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    X = C.c_void_p(4096)
    six = ("s_lo", "s_hi", "s_ids", "o_lo", "o_hi", "o_ids")

    def mask(scores=X, row0=0, rows=5, G=2, M=3, ids=X, side=X, mode=0, stats=X, **rg):
        r = {k: X for k in six}
        r.update(rg)
        return lib.amdkge_shared_mask_scores(scores, row0, rows, G, M, ids, side, *(r[k] for k in six), mode, stats, None)

    for bad in (dict(scores=None), dict(side=None), dict(row0=-1), dict(rows=-1), dict(G=0), dict(M=0), dict(M=1 << 24), dict(mode=2), dict(mode=-1),
                dict(ids=None), dict(ids=None, mode=0)) + tuple({k: None} for k in six):
        assert mask(**bad) == EINVAL, bad
    assert mask(**{k: None for k in six}) == EINVAL and b"required" in lib.amdkge_last_error()   # the mask alone needs its ranges
    assert mask(mode=7) == EINVAL and b"list_mode" in lib.amdkge_last_error()
    assert mask(rows=0) == 0 and mask(rows=0, ids=None, mode=1) == 0 and mask(rows=0, stats=None) == 0   # nothing to do; IDENTITY takes no ids

    ls = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)

    def step(model="ComplEx", loss=ls, ent=X, rel=X, tri=X, B=5, G=2, M=3, ids=X, side=X, ge=X, gr=X, acc=X, work=X, mode=0, stats=X, **rg):
        r = {k: X for k in six}
        r.update(rg)
        m = _model(_ffi, model)
        return lib.amdkge_train_shared_masked_fwdbwd(C.byref(m), C.byref(loss) if loss is not None else None, ent, rel, tri, B, G, M, ids, side, ge, gr, acc, None,
                                                     None, work, *(r[k] for k in six), mode, stats, None)

    none = {k: None for k in six}
    # the existing entry point's rules, with and without ranges
    for rg in ({}, none):
        for model in ("TransE", "RotatE"):
            assert step(model=model, **rg) == EUNSUPPORTED and b"contraction" in lib.amdkge_last_error()
        for bad in (dict(B=-1), dict(G=0), dict(G=-3), dict(M=0), dict(M=-1), dict(M=1 << 24), dict(loss=None), dict(ent=None), dict(rel=None), dict(ge=None),
                    dict(gr=None), dict(acc=None), dict(tri=None), dict(ids=None), dict(side=None), dict(work=None)):
            assert step(**bad, **rg) == EINVAL, bad
        assert step(loss=_ffi.Loss(9, 0, 0.0, 0.0), **rg) == EINVAL
        focus = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)
        focus.focus_nonlinearity, focus.d_focus_w = 1, 4096
        assert step(loss=focus, **rg) == EUNSUPPORTED and b"FocusE" in lib.amdkge_last_error()
        assert step(B=0, tri=None, side=None, work=None, **rg) == 0         # nothing to do
    # the additional ones
    for k in six:
        assert step(**{k: None}) == EINVAL and b"together" in lib.amdkge_last_error(), k
        assert step(**dict(none, **{k: X})) == EINVAL, k
    for mode in (-1, 2, 9):
        assert step(mode=mode) == EINVAL and b"list_mode" in lib.amdkge_last_error()
        assert step(mode=mode, **none) == EINVAL
    assert step(ids=None, mode=0) == EINVAL and b"d_neg_ids" in lib.amdkge_last_error()
    assert step(ids=None, mode=1) == EINVAL                                 # (the products gather by the ids whatever the mask reads)


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_mask_known_and_all_validation_and_config_round_trip():
    from ampligraph_amd.latent_features.negatives import NegativeSampling, SharedNegatives

    d = SharedNegatives(64)
    assert d.mask_known is False and d.get_config() == {"shared": 64, "group_size": 64, "side": "uniform", "entities": None}
    a = SharedNegatives("all")
    assert (a.num_negs, a.group_size, a.mask_known, a.shared) == ("all", SharedNegatives.ALL_GROUP_SIZE, False, True)
    assert SharedNegatives("all", group_size=7).group_size == 7
    valid = np.array([["a", "r", "b"]])
    for ok in (True, False, np.bool_(True), {"valid": valid}):
        m = SharedNegatives(8, mask_known=ok)
        assert m.mask_known is ok if isinstance(ok, dict) else m.mask_known == bool(ok)
    for bad in (None, 1, 0, "train", {}, [valid], valid):
        with pytest.raises(ValueError, match="mask_known"):
            SharedNegatives(8, mask_known=bad)
    for bad in ("ALL", "every", "", "16"):
        with pytest.raises(ValueError, match="num_negs"):
            SharedNegatives(bad)
        with pytest.raises(ValueError, match="num_negs"):
            NegativeSampling.get({"shared": bad})
    got = NegativeSampling.get({"shared": "all", "mask_known": True, "side": "o"})
    assert isinstance(got, SharedNegatives) and (got.num_negs, got.mask_known, got.side) == ("all", True, "o")
    cfg = got.get_config()
    assert cfg == {"shared": "all", "group_size": SharedNegatives.ALL_GROUP_SIZE, "side": "o", "entities": None, "mask_known": True}
    again = NegativeSampling.get(cfg)
    assert again.get_config() == cfg
    dm = NegativeSampling.get({"shared": 48, "group_size": 20, "mask_known": {"valid": valid}})
    assert dm.get_config()["mask_known"]["valid"] is valid and NegativeSampling.get(dm.get_config()).mask_known["valid"] is valid
    assert NegativeSampling.get({"shared": 16, "mask_known": False}).get_config() == SharedNegatives(16).get_config()
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"shared": "all", "mask": True})
    with pytest.raises(ValueError, match="unknown keys"):
        NegativeSampling.get({"shared": 16, "mask_known": True, "max_tries": 3})
    with pytest.raises(ValueError, match="breaks the sharing"):
        NegativeSampling.get({"shared": "all", "mask_known": True, "filter": True})
    with pytest.raises(ValueError, match="mask_known"):
        NegativeSampling.get({"shared": 16, "mask_known": "yes"})


def test_compile_keeps_its_refusals_with_the_new_settings():
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel
    from ampligraph_amd.latent_features.negatives import SharedNegatives

    spec = {"shared": "all", "mask_known": True}
    m = ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type="ComplEx")
    m.compile(optimizer="adam", loss="multiclass_nll", negatives=spec)
    assert isinstance(m._negatives, SharedNegatives) and m._negatives.num_negs == "all" and m._negatives.mask_known is True
    for model in ("TransE", "RotatE"):
        with pytest.raises(NotImplementedError, match="distance"):
            ScoringBasedEmbeddingModel(eta=2, k=4, scoring_type=model).compile(optimizer="adam", loss="nll", negatives=spec)
    with pytest.raises(NotImplementedError, match="deterministic"):
        m.compile(optimizer="adam", loss="nll", negatives=spec, deterministic=True)
    with pytest.raises(NotImplementedError, match="lazy"):
        m.compile(optimizer="adam", loss="nll", negatives=spec, optimizer_mode="lazy")
    for sharding in ("rows", "columns"):
        with pytest.raises(NotImplementedError, match="entity_sharding"):
            m.compile(optimizer="adam", loss="nll", negatives=spec, entity_sharding=sharding)


def test_step_loop_takes_the_masked_call_only_when_a_mask_is_bound():
    import torch

    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    calls = []

    class Eng:
        scoring_type, k, device = "ComplEx", 8, "cpu"

        def prepare_training(self, name):
            pass

        def train_shared_fwdbwd(self, triples, G, M, ids, side, loss):
            calls.append(("shared", tuple(triples.shape), G, M, ids, side))

        def train_shared_masked_fwdbwd(self, triples, G, M, ids, side, loss, s_filter=None, o_filter=None, identity=False, stats=None):
            calls.append(("masked", tuple(triples.shape), G, M, ids, side, s_filter, o_filter, identity, stats))

        def opt_step(self, *a):
            calls.append(("opt",))

    loop = StepLoop(Eng(), 3, loss_functions.get("nll"), optimizers.get("adam"), None, seed=5, dist=None)
    batch = torch.zeros(10, 3, dtype=torch.int32)
    loop.negatives = bound(loop.engine, "masked", calls)
    loop.step(batch, 7)
    assert calls == [("draw", (10, 3), 5, 7), ("mask", (10, 3)), ("masked", (10, 3), 4, 6, "ids", "side", "sf", "of", True, "stats"), ("opt",)]
    del calls[:]
    loop.negatives = bound(loop.engine, "shared", calls)
    loop.step(batch, 8)
    assert calls == [("draw", (10, 3), 5, 8), ("shared", (10, 3), 4, 6, "ids", "side"), ("opt",)] and loop.n_steps == 2
    loop.negatives = bound(loop.engine, "masked", calls)
    with pytest.raises(NotImplementedError, match="FocusE"):
        loop.step(batch, 9, focus=(torch.zeros(10), 0.5, "linear"))
    loop.deterministic = True
    with pytest.raises(NotImplementedError, match="deterministic"):
        loop.step(batch, 9)
    loop.deterministic, loop.multi = False, True
    with pytest.raises(NotImplementedError, match="one rank"):
        loop.step(batch, 10)


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_mask_matrix_by_hand():
    """4 positives in groups of 2, lists of 5.  Row 0 (subject side): two hits, one of them a repeated id.  Row 1 (object side):
    its own entity only.  Row 2: EVERY entry known -> left unmasked and counted.  Row 3: an empty range."""
    X = np.array([[1, 0, 2], [3, 1, 4], [5, 0, 6], [7, 1, 8]], dtype=np.int32)
    ids = np.array([[9, 1, 4, 9, 0], [6, 6, 2, 6, 2]], dtype=np.int32)
    side = np.array([1, 0, 0, 1], dtype=np.int32)
    known_s = [np.array([1, 9, 30]), np.array([0, 1, 4, 9]), np.array([], dtype=np.int64), np.array([], dtype=np.int64)]
    known_o = [np.array([0, 4]), np.array([4]), np.array([2, 6, 11]), np.array([2, 6])]
    mask, masked, unmaskable = MR.mask_matrix(X, 2, ids, side, known_s, known_o)
    want = np.array([[1, 1, 0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=bool)
    assert mask.dtype == bool and np.array_equal(mask, want) and (masked, unmaskable) == (4, 1)
    # a group size larger than the batch is the batch
    one = MR.mask_matrix(X[:2], 100, ids[:1], side[:2], known_s[:2], known_o[:2])
    assert np.array_equal(one[0], want[:2]) and one[1:] == (4, 0)
    lo, hi, flat = MR.csr([known_s[i] if side[i] else known_o[i] for i in range(4)])
    assert lo.tolist() == [0, 3, 4, 0] and hi.tolist() == [3, 4, 7, 0] and flat.tolist() == [1, 9, 30, 4, 2, 6, 11]


def test_known_lists_are_the_filter_index_ranges():
    from ampligraph_amd.datasets.filters import FilterIndex

    rng = np.random.default_rng(0)
    N, R = 12, 2
    X = np.stack([rng.integers(0, N, 80), rng.integers(0, R, 80), rng.integers(0, N, 80)], 1).astype(np.int32)
    extra = X[:10].copy()
    extra[:, 0] = (extra[:, 0] + 1) % N
    ks, ko = MR.known_lists(X, [X, extra], N, R)
    fs, fo = FilterIndex([X, extra], N, R).as_lists(X)
    assert all(np.array_equal(a, b) for a, b in zip(ks, fs)) and all(np.array_equal(a, b) for a, b in zip(ko, fo))
    assert all(X[i, 0] in ks[i] and X[i, 2] in ko[i] for i in range(len(X)))   # a positive's own entity is known


@pytest.mark.parametrize("loss", list(O.LOSS_DEFAULTS))
@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_masked_step_equals_the_step_without_the_masked_corruptions_where_the_divisor_allows(loss, reduction):
    """What -inf means, shown on the oracle: finite everything, zero coefficients at the mask.  For the two losses in which the
    number of corruptions enters through the reduction divisor alone (pairwise, self_adversarial; nll and absolute_margin weigh the
    positive's term by it, multiclass_nll keeps e^-75 per masked entry) the masked "sum" step IS the step without those entries."""
    rng = np.random.default_rng(1)
    N, R, k, B, G, M = 9, 2, 4, 6, 6, 5
    ent, rel = (rng.normal(size=(N, k)) * 0.5).astype(np.float32), (rng.normal(size=(R, k)) * 0.5).astype(np.float32)
    X = np.stack([rng.integers(0, N, B), rng.integers(0, R, B), rng.integers(0, N, B)], 1).astype(np.int32)
    ids = np.array([[0, 1, 2, 3, 4]], dtype=np.int32)
    side = np.ones(B, dtype=np.int32)
    mask = np.zeros((B, M), dtype=bool)
    mask[:, 3:] = True                                                      # the same two entries for every positive
    L, Ge, Gr, sp, sn = MR.masked_step("DistMult", ent, rel, X, G, ids, side, mask, loss, reduction, R)
    assert np.isneginf(sn.reshape(M, B)[3:]).all() and np.isfinite(sn.reshape(M, B)[:3]).all() and np.isfinite(L)
    if reduction == "sum" and loss in ("pairwise", "self_adversarial"):
        L3, Ge3, Gr3, _, _ = MR.masked_step("DistMult", ent, rel, X, G, ids[:, :3], side, mask[:, :3] & False, loss, reduction, R)
        assert np.isclose(L, L3, rtol=1e-6) and np.allclose(Ge, Ge3, rtol=1e-6, atol=1e-9) and np.allclose(Gr, Gr3, rtol=1e-6, atol=1e-9)
