"""The refusals of the five shared-list train steps without a GPU, as ONE table: amdkge_train_shared_fwdbwd, _masked_fwdbwd and
_labels_fwdbwd (matrix products: DistMult / ComplEx / HolE) and amdkge_train_shared_dist_fwdbwd and _dist_labels_fwdbwd (distance
tiles: TransE / RotatE) run one host driver, so each bad argument has one return code and one message text in all five, behind the
prefix of whoever checks it: the family ("train_shared" / "train_shared_dist") for the step's own arguments, the entry point for
its list and range arguments, none for the model descriptor.  Every refusal is returned before any device work: the pointers that
are set are never dereferenced.  The order of the checks is part of the table (test_order_of_the_checks)."""
import ctypes as C

import pytest

OK, EINVAL, EUNSUPPORTED = 0, -1, -5
X = C.c_void_p(4096)
SIX = ("s_lo", "s_hi", "s_ids", "o_lo", "o_hi", "o_ids")
GIVEN, IDENTITY = 0, 1

# entry point -> (family prefix, the entry point's own prefix, kind of argument list, a model it takes, a model of the other family,
#                 what it says to the other family's model)
PRODUCTS_ONLY = "TransE and RotatE score a distance, not a contraction: only DistMult, ComplEx and HolE share negatives"
DISTANCES_ONLY = "DistMult, ComplEx and HolE score a contraction, not a distance: use amdkge_train_shared_fwdbwd"
ENTRIES = {
    "amdkge_train_shared_fwdbwd": ("train_shared", None, "plain", "ComplEx", "TransE", PRODUCTS_ONLY),
    "amdkge_train_shared_masked_fwdbwd": ("train_shared", "train_shared_masked", "masked", "DistMult", "RotatE", PRODUCTS_ONLY),
    "amdkge_train_shared_labels_fwdbwd": ("train_shared", "train_shared_labels", "labels", "HolE", "TransE", PRODUCTS_ONLY),
    "amdkge_train_shared_dist_fwdbwd": ("train_shared_dist", "train_shared_dist", "masked", "TransE", "DistMult", DISTANCES_ONLY),
    "amdkge_train_shared_dist_labels_fwdbwd": ("train_shared_dist", "train_shared_dist_labels", "labels", "RotatE", "HolE", DISTANCES_ONLY),
}
SIZES = "bad sizes (B >= 0, G >= 1, 1 <= M < 2^24)"
TABLES = "NULL table / gradient / loss pointer"
BUFFERS = "NULL triples / ids / sides / workspace"
PARTIAL = {"masked": "the six range arrays are given together or not at all", "labels": "the six range arrays are all required (labels need them)"}


def _call(name, model, loss="nll", ent=X, rel=X, tri=X, B=5, G=2, M=3, ids=X, side=X, ge=X, gr=X, acc=X, work=X, mode=GIVEN, **ranges):
    """the entry point `name` on dummy pointers -> (return code, amdkge_last_error()); model: a scoring type's name, None (a NULL
    descriptor) or an _ffi.Model; loss: a loss name, None (NULL) or an _ffi.Loss"""
    from ampligraph_amd import _ffi

    lib = _ffi.lib()
    kind = ENTRIES[name][2]
    m = _ffi.Model(_ffi.SCORING_TYPES[model], 8, 50, 4, 4, 0, 0, 0) if isinstance(model, str) else model
    ls = _ffi.Loss(_ffi.LOSSES[loss], 0, 0.0, 0.0) if isinstance(loss, str) else loss
    rg = {k: X for k in SIX}
    rg.update(ranges)
    head = (ent, rel, tri, B, G, M, ids, side, ge, gr, acc, None, None, work)
    mref, lref = (C.byref(m) if m is not None else None), (C.byref(ls) if ls is not None else None)
    if kind == "plain":
        args = (mref, lref) + head + (None,)
    elif kind == "masked":
        args = (mref, lref) + head + tuple(rg[k] for k in SIX) + (mode, X, None)
    else:
        args = (mref, 0.0, 0) + head + tuple(rg[k] for k in SIX) + (mode, None, None, X, None)
    rc = getattr(lib, name)(*args)
    return rc, lib.amdkge_last_error().decode()


def _focus():
    from ampligraph_amd import _ffi

    ls = _ffi.Loss(_ffi.LOSSES["nll"], 0, 0.0, 0.0)
    ls.focus_nonlinearity, ls.d_focus_w = 1, 4096
    return ls


def _bad_kind():
    from ampligraph_amd import _ffi

    return _ffi.Loss(9, 0, 0.0, 0.0)


def _table(name):
    """-> [(label, the bad arguments, return code, prefix or None, message text)] in the order in which the entry point checks"""
    family, who, kind, _, other, wrong_family = ENTRIES[name]
    rows = []
    if kind != "plain":                                                         # the list and range arguments: checked first, by the entry point
        for k in SIX:
            rows.append(("five ranges, no " + k, {k: None}, EINVAL, who, PARTIAL[kind]))
        for mode in (-1, 2, 9):
            rows.append((f"list_mode {mode}", dict(mode=mode), EINVAL, who, "unknown list_mode"))
        rows.append(("GIVEN without ids", dict(ids=None, mode=GIVEN), EINVAL, who, "AMDKGE_SHARED_LIST_GIVEN needs d_neg_ids"))
    rows.append(("NULL model", dict(model=None), EINVAL, None, "model descriptor is NULL"))
    rows.append(("wrong-family model", dict(model=other), EUNSUPPORTED, family, wrong_family))
    if kind != "labels":
        rows.append(("NULL loss", dict(loss=None), EINVAL, family, "unknown loss kind"))
        rows.append(("bad loss kind", dict(loss=_bad_kind()), EINVAL, family, "unknown loss kind"))
        rows.append(("FocusE", dict(loss=_focus()), EUNSUPPORTED, family, "FocusE is not offered with shared negatives"))
    for bad in (dict(G=0), dict(M=0), dict(M=1 << 24), dict(B=-1)):
        rows.append((str(bad), bad, EINVAL, family, SIZES))
    for p in ("ent", "rel", "ge", "gr", "acc"):
        rows.append(("NULL " + p, {p: None}, EINVAL, family, TABLES))
    for p in ("tri", "ids", "side", "work"):
        bad = {p: None}
        if p == "ids" and kind != "plain":
            bad["mode"] = IDENTITY                                              # (the tiles gather by the ids whatever the mask or the labels read)
        rows.append(("NULL " + p, bad, EINVAL, family, BUFFERS))
    return rows


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refusal_table(name):
    model = ENTRIES[name][3]
    assert _call(name, model, B=0, tri=None, side=None, work=None)[0] == OK    # nothing to do: after the table pointers, before the buffers
    for label, bad, code, prefix, text in _table(name):
        rc, msg = _call(name, **dict(dict(model=model), **bad))
        assert rc == code and msg == (prefix + ": " if prefix else "") + text, (name, label, rc, msg)
    # B == 0 returns OK only where every check in front of it passes
    rc, msg = _call(name, model, B=0, tri=None, acc=None)
    assert rc == EINVAL and msg == ENTRIES[name][0] + ": " + TABLES
    rc, msg = _call(name, model, B=0, G=0, tri=None)
    assert rc == EINVAL and msg == ENTRIES[name][0] + ": " + SIZES


@pytest.mark.parametrize("name", list(ENTRIES))
def test_order_of_the_checks(name):
    """One fault per check, all of them in ONE call, then one fewer from the front each time: the call reports the first that is
    left.  (Faults that need the same argument, as G = 0 and a clamped G, take one representative.)"""
    family, who, kind, model, other, wrong_family = ENTRIES[name]
    chain = []
    if kind != "plain":
        chain += [(dict(s_hi=None), EINVAL, who, PARTIAL[kind]), (dict(mode=7), EINVAL, who, "unknown list_mode")]
    chain += [(dict(model=other), EUNSUPPORTED, family, wrong_family)]
    if kind != "labels":
        chain += [(dict(loss=_focus()), EUNSUPPORTED, family, "FocusE is not offered with shared negatives")]
    chain += [(dict(M=0), EINVAL, family, SIZES), (dict(gr=None), EINVAL, family, TABLES), (dict(work=None), EINVAL, family, BUFFERS)]
    for i in range(len(chain)):
        kw = dict(model=model)
        for bad, _, _, _ in chain[i:]:
            kw.update(bad)
        rc, msg = _call(name, **kw)
        assert rc == chain[i][1] and msg == chain[i][2] + ": " + chain[i][3], (name, i, rc, msg)
    # a NULL or unknown descriptor is refused in front of everything the family checks, behind what the entry point checks
    from ampligraph_amd import _ffi

    for m, text in ((None, "model descriptor is NULL"), (_ffi.Model(17, 8, 50, 4, 4, 0, 0, 0), "unknown scoring_type (expected TransE/DistMult/ComplEx/HolE/RotatE)")):
        rc, msg = _call(name, m, loss=None, M=0, ent=None, work=None)
        assert rc == EINVAL and msg == text
        if kind != "plain":
            rc, msg = _call(name, m, mode=7)
            assert rc == EINVAL and msg == who + ": unknown list_mode"


def test_the_two_families_say_the_same_but_for_prefix_and_model():
    """the sibling entry points (masked <-> dist, labels <-> dist_labels) agree row by row on code and text"""
    for a, b in (("amdkge_train_shared_masked_fwdbwd", "amdkge_train_shared_dist_fwdbwd"), ("amdkge_train_shared_labels_fwdbwd", "amdkge_train_shared_dist_labels_fwdbwd")):
        ta, tb = _table(a), _table(b)
        assert len(ta) == len(tb)
        for (la, _, ca, _, xa), (lb, _, cb, _, xb) in zip(ta, tb):
            assert (la, ca) == (lb, cb) and (xa == xb or la == "wrong-family model")
