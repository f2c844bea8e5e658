"""Guard-band tests: no C-ABI call may write, or depend on, a byte outside the buffers it was handed.

Every device argument of a case is a `guarded` buffer (tests/guarded.py) of exactly the size include/amdkge.h gives it -- workspaces
exactly what the matching *_workspace_bytes returns, handed over 16 bytes behind a 256-byte boundary so that the self-alignment
slack they budget is consumed; strided blocks end with their last live element, not with a whole last row.  Each case runs three
times from identical payloads -- bands on fill A, bands on fill B, ordinary torch tensors -- and asserts

  (a) after the call both bands of every argument still hold their fill, and no input payload changed a bit;
  (b) every output payload is bit-identical between fill A and fill B (nothing read outside a buffer reaches a result);
  (c) the outputs equal those on ordinary tensors, bit for bit; gap columns [m, ld) and elements between strided ranks keep
      their pre-filled value.

Where an entry adds fp32 / fp64 values with atomics in arrival order (amdkge_train_fwdbwd, the default tiled step, the fp64 loss
and regulariser accumulators) those outputs are held, in all three runs, to the oracle comparison the entry already has in the
suite, with that test's bar (named at each such case); everything else of the case stays bitwise.  Lists the ABI fills "in no
particular order" are compared as sets.

CASES, the table below, is data: tests/test_guard_bands_host.py checks it against the header without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import guarded, guarded_host
from oracle import kge_oracle as O
from test_gpu_kernels import assert_grads_close, loss_desc, make_optimizer, rand_triples

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = np.float32, np.float64, np.int32, np.int64, np.uint8
COMPLEX = ("ComplEx", "HolE", "RotatE")

# entry point -> [(case function, its arguments), ...]
CASES = {
    "amdkge_score": [("score", dict(model="ComplEx", k=7, pad=False, n=37)), ("score", dict(model="TransE", k=50, pad=True, n=1)),
                     ("score", dict(model="DistMult", k=200, pad=True, n=37)), ("score", dict(model="RotatE", k=350, pad=True, n=37)),
                     ("score", dict(model="HolE", k=516, pad=True, n=37))],
    "amdkge_sample_corruptions": [("sample_corruptions", dict(B=37, eta=3)), ("sample_corruptions", dict(B=1, eta=1))],
    "amdkge_pack_rows": [("pack_rows", dict(model="ComplEx", k=7, n=37, unpack=False)), ("pack_rows", dict(model="TransE", k=50, n=1, unpack=False))],
    "amdkge_unpack_rows": [("pack_rows", dict(model="ComplEx", k=7, n=37, unpack=True)), ("pack_rows", dict(model="RotatE", k=350, n=37, unpack=True))],
    "amdkge_train_fwdbwd": [("train_fwdbwd", dict(model="TransE", k=7, pad=False)), ("train_fwdbwd", dict(model="ComplEx", k=50, pad=True)),
                            ("train_fwdbwd", dict(model="DistMult", k=200, pad=True)), ("train_fwdbwd", dict(model="RotatE", k=350, pad=True))],
    "amdkge_opt_step": [("opt_step", dict(lazy=0)), ("opt_step", dict(lazy=1))],
    "amdkge_train_step_tiled": [("tiled", dict(model="ComplEx", k=50, mode="grad_det")), ("tiled", dict(model="TransE", k=7, mode="grad")),
                                ("tiled", dict(model="RotatE", k=350, mode="grad")), ("tiled", dict(model="DistMult", k=200, mode="grad")),
                                ("tiled", dict(model="ComplEx", k=50, mode="step_det", lazy=0)), ("tiled", dict(model="ComplEx", k=50, mode="step_det", lazy=1)),
                                ("tiled", dict(model="HolE", k=516, mode="grad", direct=1)), ("tiled", dict(model="HolE", k=516, mode="grad", direct=0)),
                                ("tiled", dict(model="ComplEx", k=16, mode="bucket_overflow")), ("tiled", dict(model="ComplEx", k=50, mode="grad_atomic")),
                                ("tiled", dict(model="RotatE", k=12, mode="step", lazy=0)), ("tiled", dict(model="DistMult", k=12, mode="step", lazy=1))],
    "amdkge_train_tiled_set_hot_rows": [("tiled", dict(model="ComplEx", k=16, mode="hot"))],
    "amdkge_cols_partial_scores": [("cols_partial", dict(model="ComplEx", k=200, W=4)), ("cols_partial", dict(model="TransE", k=64, W=4))],
    "amdkge_cols_loss": [("cols_loss", dict(B=37, eta=3)), ("cols_loss", dict(B=1, eta=1))],
    "amdkge_platt_step": [("platt", dict(n_pos=37, n_neg=130)), ("platt", dict(n_pos=1, n_neg=9))],
    "amdkge_rank_counts": [("rank_counts", dict(model="TransE", k=7, pad=False, n=37, N=130, kernel=1)),
                           ("rank_counts", dict(model="DistMult", k=50, pad=True, n=37, N=257, kernel=1)),
                           ("rank_counts", dict(model="DistMult", k=50, pad=True, n=37, N=257, kernel=2)),
                           ("rank_counts", dict(model="ComplEx", k=200, pad=True, n=37, N=130, kernel=3)),
                           ("rank_counts", dict(model="HolE", k=350, pad=True, n=1, N=257, kernel=0)),
                           ("rank_counts", dict(model="RotatE", k=50, pad=True, n=37, N=130, kernel=0)),
                           ("rank_counts", dict(model="TransE", k=200, pad=True, n=37, N=257, kernel=0, ids=130)),
                           ("rank_counts", dict(model="ComplEx", k=50, pad=True, n=37, N=130, kernel=0, ids=9)),
                           ("rank_counts", dict(model="DistMult", k=50, pad=True, n=130, N=257, kernel=3)),
                           ("rank_counts", dict(model="TransE", k=50, pad=True, n=130, N=130, kernel=1)),
                           ("rank_counts", dict(model="RotatE", k=350, pad=True, n=37, N=130, kernel=0))],
    "amdkge_rank_counts_screened": [("screened", dict(model="ComplEx", k=50, how="screen")), ("screened", dict(model="DistMult", k=50, how="screen")),
                                    ("screened", dict(model="ComplEx", k=50, how="null")), ("screened", dict(model="ComplEx", k=50, how="too_small")),
                                    ("screened", dict(model="ComplEx", k=50, how="one_byte_short")), ("screened", dict(model="ComplEx", k=50, how="overflow")),
                                    ("screened", dict(model="TransE", k=64, how="screen")), ("screened", dict(model="RotatE", k=64, how="screen")),
                                    ("screened", dict(model="TransE", k=64, how="overflow"))],
    "amdkge_filter_build": [("filter_build", dict(form="s", m=37)), ("filter_build", dict(form="o", m=130)), ("filter_build", dict(form="o", m=1))],
    "amdkge_pair_filter_build": [("filter_build", dict(form="pair", m=130))],
    "amdkge_filter_ranges": [("filter_ranges", dict(form="s", n=37)), ("filter_ranges", dict(form="o", n=1))],
    "amdkge_pair_filter_ranges": [("filter_ranges", dict(form="pair", n=37))],
    "amdkge_rank_filter": [("rank_filter", dict(model="ComplEx", k=50, subset=False)), ("rank_filter", dict(model="TransE", k=7, subset=True))],
    "amdkge_rank_compose": [("rank_compose", dict(n=37, stride=2, sub=True)), ("rank_compose", dict(n=1, stride=1, sub=False))],
    "amdkge_corruption_scores": [("corruption_scores", dict(model="DistMult", k=50, n=37, N=130, ids=0)),
                                 ("corruption_scores", dict(model="TransE", k=7, n=37, N=257, ids=0)),
                                 ("corruption_scores", dict(model="RotatE", k=50, n=1, N=130, ids=9)),
                                 ("corruption_scores", dict(model="ComplEx", k=200, n=37, N=257, ids=130))],
    "amdkge_row_dots": [("row_dots", dict(n=37, Kf=104, N=130, ids=0)), ("row_dots", dict(n=1, Kf=7, N=257, ids=9))],
    "amdkge_row_sqnorms": [("row_sqnorms", dict(Kf=104, N=130, ids=0, rsqrt=0)), ("row_sqnorms", dict(Kf=7, N=257, ids=130, rsqrt=1))],
    "amdkge_topk_rows": [("topk", dict(n=37, m=130, k=10, extras=True)), ("topk", dict(n=1, m=9, k=12, extras=False)),
                         ("topk", dict(n=37, m=130, k=10, extras=True, largest=0)),
                         ("topk", dict(n=37, m=1500, k=1024, extras=False))],
    "amdkge_topk_rows_excluding": [("topk_excluding", dict(n=37, m=130, k=10, ids=True)), ("topk_excluding", dict(n=1, m=9, k=12, ids=False))],
    "amdkge_pair_distances": [("pair_distances", dict(n=37, Kf=104, k=5, cosine=0)), ("pair_distances", dict(n=1, Kf=7, k=3, cosine=1))],
    "amdkge_join_nearest": [("join_nearest", dict(n=130, d=7)), ("join_nearest", dict(n=257, d=52)), ("join_nearest", dict(n=1, d=3))],
    "amdkge_join_radius": [("join_radius", dict(n=130, d=7, overflow=False)), ("join_radius", dict(n=257, d=52, overflow=False)),
                           ("join_radius", dict(n=130, d=7, overflow=True))],
    "amdkge_join_dbscan": [("join_dbscan", dict(n=130, d=7)), ("join_dbscan", dict(n=257, d=52))],
    "amdkge_kmeans_assign": [("kmeans_assign", dict(n=130, d=7, k=3, runs=2)), ("kmeans_assign", dict(n=257, d=52, k=37, runs=1)),
                             ("kmeans_assign", dict(n=257, d=9, k=130, runs=1))],
    "amdkge_kmeans_lloyd": [("kmeans_lloyd", dict(n=130, d=7, k=3, runs=2)), ("kmeans_lloyd", dict(n=257, d=52, k=37, runs=1))],
    "amdkge_discover_select": [("discover_select", dict(n=37, m=130, overflow=False, given=0)), ("discover_select", dict(n=1, m=9, overflow=False, given=1)),
                               ("discover_select", dict(n=37, m=130, overflow=True, given=0))],
    "amdkge_relation_scores": [("relation_scores", dict(model="ComplEx", k=50, n=37, R=9, ids=0)), ("relation_scores", dict(model="TransE", k=7, n=37, R=130, ids=0)),
                               ("relation_scores", dict(model="RotatE", k=50, n=37, R=130, ids=9)), ("relation_scores", dict(model="DistMult", k=200, n=1, R=9, ids=0)),
                               ("relation_scores", dict(model="HolE", k=350, n=37, R=130, ids=0))],
    "amdkge_relation_rank_counts": [("relation_rank_counts", dict(n=37, m=130, flt=True)), ("relation_rank_counts", dict(n=1, m=9, flt=False))],
    "amdkge_shard_route": [("shard_route", dict(b=37, nneg=0, cap=40)), ("shard_route", dict(b=37, nneg=111, cap=130)),
                           ("shard_route", dict(b=130, nneg=0, cap=9))],
    "amdkge_gather_rows": [("gather_rows", dict(Kf=104, n=37)), ("gather_rows", dict(Kf=8, n=1))],
    "amdkge_scatter_add_rows": [("scatter_add_rows", dict(Kf=104, n=37)), ("scatter_add_rows", dict(Kf=7, n=130))],
    "amdkge_opt_step_merged": [("opt_step_merged", dict(n_elems=1107, n_parts=3))],
    "amdkge_synth_triples": [("synth_triples", dict(n=37)), ("synth_triples", dict(n=257))],
    "amdkge_session_score": [("session", dict(what="score"))],
    "amdkge_session_rank": [("session", dict(what="rank"))],
    "amdkge_session_get_rows": [("session", dict(what="get_rows"))],
    "amdkge_session_group_get_rows": [("session", dict(what="group_get_rows"))],
    "amdkge_session_group_rank": [("session", dict(what="group_rank"))],
}


# ------------------------------------------------------------------------------------------------------------------ the arena
def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def HP(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Arena:
    """The buffers of one run of a case.  mode 'A' / 'B': every buffer between guard bands on that fill; 'plain': ordinary tensors."""

    def __init__(self, mode):
        self.mode = mode
        self.items = {}       # name -> (tensor or numpy payload, guard or None, role, initial numpy copy)
        self.loose = set()    # outputs held to an oracle instead of bitwise equality between the runs
        self.canon = {}       # name -> canonical form of an unordered output
        self.keeps = []       # (name, flat boolean mask): elements that must keep their pre-filled bits
        self.expects = []     # callables(outs): the case's own assertions, run on every mode
        self.cleanups = []

    def put(self, name, data, role="in", offset=0):
        """data: numpy array, the payload's content on entry.  role: 'in' (must come back unchanged), 'out' (compared between the
        runs) or 'work' (scratch: guarded, never compared).  -> the device tensor the call is handed."""
        data = np.ascontiguousarray(data)
        assert name not in self.items and role in ("in", "out", "work"), name
        if data.size == 0:
            self.items[name] = (None, None, role, data)
            return None
        if self.mode == "plain":
            g, t = None, torch.empty(data.shape, dtype=getattr(torch, data.dtype.name), device="cuda")
        else:
            g = guarded(data.shape, data.dtype, "cuda", self.mode, offset=offset, name=name)
            t = g.tensor
            assert t.data_ptr() % 256 == offset and t.numel() * t.element_size() == data.nbytes
        t.copy_(torch.as_tensor(data))
        self.items[name] = (t, g, role, data.copy())
        return t

    def out(self, name, shape, dtype, prefill):
        return self.put(name, np.full(shape, prefill, dtype=dtype), "out")

    def work(self, name, nbytes):
        """a workspace the library aligns itself: exactly nbytes, zero-filled, 16 bytes behind a 256-byte boundary"""
        assert nbytes >= 0, (name, nbytes)
        return self.put(name, np.zeros(int(nbytes), U8), "work", offset=16)

    def host(self, name, shape, dtype, prefill):
        """a host output array of the session layer"""
        if self.mode == "plain":
            g, a = None, np.empty(shape, dtype=dtype)
        else:
            g = guarded_host(shape, dtype, self.mode, name=name)
            a = g.array
        a[...] = prefill
        self.items[name] = (a, g, "out", a.copy())
        return a

    def keep(self, name, mask):
        self.keeps.append((name, np.asarray(mask).reshape(-1)))

    def tensor(self, name):
        return self.items[name][0]

    def finish(self):
        torch.cuda.synchronize()
        for fn in self.cleanups:
            fn()
        outs = {}
        for name, (t, g, role, init) in self.items.items():
            if g is not None:
                g.check()                                               # (a) both bands intact
            if t is None:
                continue
            now = t.cpu().numpy() if torch.is_tensor(t) else t.copy()
            if role == "in":
                assert same_bits(now, init), f"input {name} was written"   # (a) inputs are not written at all
            elif role == "out":
                outs[name] = now
        for name, mask in self.keeps:                                   # (c) gaps keep their pre-filled value
            now, init = _bits(outs[name]).reshape(mask.size, -1), _bits(self.items[name][3]).reshape(mask.size, -1)
            assert np.array_equal(now[mask], init[mask]), f"{name}: elements outside the block were written"
        for fn in self.expects:
            fn(outs)
        return {k: (self.canon[k](v, outs) if k in self.canon else v) for k, v in outs.items() if k not in self.loose}


def run_case(fn, kw):
    from ampligraph_amd import _ffi

    res = {}
    try:
        for mode in ("A", "B", "plain"):
            ar = Arena(mode)
            try:
                fn(ar, **kw)
                res[mode] = ar.finish()
            except RuntimeError as e:
                for c in ar.cleanups:
                    c()
                if any(w in str(e) for w in ("illegal memory access", "launch failure", "hardware exception")):
                    pytest.exit(f"GPU fault in {fn.__name__}{kw} ({mode}): nothing more runs on this device -- {e}", returncode=3)
                raise
            except BaseException:
                for c in ar.cleanups:
                    c()
                raise
    finally:
        _ffi.lib().amdkge_release_scratch()   # (the per-accumulator loss partials amdkge_train_fwdbwd keys by pointer)
    for other, what in (("B", "(b) depends on bytes outside its buffers"), ("plain", "(c) differs from the call on ordinary tensors")):
        assert res[other].keys() == res["A"].keys()
        for name, a in res["A"].items():
            assert same_bits(a, res[other][name]), f"{name}: {what}"


def _params():
    for entry, cases in CASES.items():
        for fn, kw in cases:
            yield pytest.param(fn, kw, id=entry[len("amdkge_"):] + "-" + "-".join(str(v) for v in kw.values()))


@pytest.mark.parametrize("fn,kw", list(_params()))
def test_guard_bands(gpu_lib, fn, kw):
    run_case(globals()["case_" + fn], kw)


def test_harness_sees_a_byte_on_the_device(gpu_lib):
    """The self-test of tests/test_guard_bands_host.py on device memory: one byte behind / in front of the payload, written through the
    allocation's own oversized view (inside the allocation: nothing faults), fails .check() with its offset; restored, it passes."""
    g = guarded((37, 130), torch.float32, "cuda", "B", offset=16, name="probe")
    assert g.tensor.data_ptr() % 256 == 16 and g.nbytes == 19240
    g.tensor.fill_(3.0)
    g.check()
    for at, off in ((g.lead + g.nbytes, 19240), (g.lead - 1, -1)):
        old = int(g.raw[at])
        g.raw[at] = old ^ 0x40
        with pytest.raises(AssertionError, match=f"payload offset {off}"):
            g.check()
        g.raw[at] = old
        g.check()


# ------------------------------------------------------------------------------------------------------------------ helpers
def _lib():
    from ampligraph_amd import _ffi

    return _ffi, _ffi.lib()


def stored(dense, k, ks, nc):
    """dense rows [n, nc * k] -> stored rows [n, nc * ks] (include/amdkge.h "STORED row layout")"""
    out = np.zeros((dense.shape[0], nc * ks), F32)
    for h in range(nc):
        out[:, h * ks:h * ks + k] = dense[:, h * k:(h + 1) * k]
    return out


def unstored(rows, k, ks, nc):
    return np.concatenate([rows[:, h * ks:h * ks + k] for h in range(nc)], 1)


class Tables:
    def __init__(self, model, k, N, R, pad=True, seed=0, scale=None, k_full=0):
        _ffi, _ = _lib()
        rng = np.random.default_rng(seed)
        self.model, self.k, self.N, self.R = model, k, N, R
        self.nc = 2 if model in COMPLEX else 1
        self.ks = (k + 3) // 4 * 4 if pad else k
        self.Ks = self.nc * self.ks
        scale = (0.3 if k < 100 else 0.08) if scale is None else scale
        self.ent = (rng.normal(size=(N, self.nc * k)) * scale).astype(F32)
        self.rel = (rng.normal(size=(R, self.nc * k)) * scale).astype(F32)
        self.m = _ffi.Model(_ffi.SCORING_TYPES[model], k, N, R, R, self.ks, k_full, 0)

    @property
    def ent_s(self):
        return stored(self.ent, self.k, self.ks, self.nc)

    @property
    def rel_s(self):
        return stored(self.rel, self.k, self.ks, self.nc)

    def dense(self, rows):
        return unstored(rows, self.k, self.ks, self.nc)


def edge_triples(seed, n, N, R):
    """random triples that also touch the first and the last row of both tables"""
    X = rand_triples(np.random.default_rng(seed), n, N, R)
    X[0] = (N - 1, R - 1, 0)
    X[-1, 2] = N - 1
    return X


def block_mask(n, m, ld):
    """flat mask of the elements of an [n, m] block with leading dimension ld inside its exact (n - 1) * ld + m buffer"""
    idx = np.arange((n - 1) * ld + m)
    return idx % ld < m


def loss_bar(got, ref, rel):
    assert abs(got - ref) <= rel * max(1.0, abs(ref)), (got, ref)


# ------------------------------------------------------------------------------------------------------------------ predict, sampling, rows
def case_score(ar, model, k, pad, n, N=130, R=9):
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad)
    if T.ent_s.nbytes % 512 == 0:      # a whole number of allocator blocks: an odd row count instead
        T = Tables(model, k, 257, R, pad)
    X = edge_triples(1, n, T.N, R)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    out = ar.out("scores", (n,), F32, 7.0)
    _ffi.check(lib.amdkge_score(C.byref(T.m), P(ent), P(rel), P(tri), n, P(out), None))


def case_sample_corruptions(ar, B, eta, N=130):
    _ffi, lib = _lib()
    tri = ar.put("triples", edge_triples(2, B, N, 5))
    out = ar.out("negs", (B * eta, 3), I32, 1)
    _ffi.check(lib.amdkge_sample_corruptions(P(tri), B, eta, 0, N, 12345678901234, (1 << 33) + 5, 17, B + 40, P(out), None))


def case_pack_rows(ar, model, k, n, unpack):
    _ffi, lib = _lib()
    T = Tables(model, k, n, 3)
    if unpack:
        src, dst = ar.put("stored", T.ent_s), ar.out("dense", (n, T.nc * k), F32, 7.0)
        _ffi.check(lib.amdkge_unpack_rows(C.byref(T.m), P(src), n, P(dst), None))
        ar.expects.append(lambda o: np.testing.assert_array_equal(o["dense"], T.ent))
    else:
        src, dst = ar.put("dense", T.ent), ar.out("stored", (n, T.Ks), F32, 7.0)
        _ffi.check(lib.amdkge_pack_rows(C.byref(T.m), P(src), n, P(dst), None))
        ar.expects.append(lambda o: np.testing.assert_array_equal(o["stored"], T.ent_s))


# ------------------------------------------------------------------------------------------------------------------ training
def case_train_fwdbwd(ar, model, k, pad, N=130, R=4, B=37, eta=5):
    """fp32 atomics into both gradient tables, an fp64 atomic into the loss: (b) / (c) of those three outputs are the oracle comparison
    of test_gpu_kernels.py::test_train_fwdbwd_geometries (assert_grads_close at its default 2e-5, loss within 2e-5); the scores bitwise."""
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad)
    X = edge_triples(4, B, N, R)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    ge, gr = ar.out("g_ent", (N, T.Ks), F32, 0.0), ar.out("g_rel", (R, T.Ks), F32, 0.0)
    ls = ar.out("loss", (1,), F64, 0.0)
    ps, ns = ar.out("pos_scores", (B,), F32, 7.0), ar.out("neg_scores", (B * eta,), F32, 7.0)
    _ffi.check(lib.amdkge_train_fwdbwd(C.byref(T.m), C.byref(loss_desc("self_adversarial")), P(ent), P(rel), P(tri), B, eta, 0, N, 1, 0, 0, 0, None,
                                       P(ge), P(gr), P(ls), P(ps), P(ns), None))
    ar.loose |= {"g_ent", "g_rel", "loss"}
    negs = O.generate_corruptions(X, N, eta, 1, 0)
    total, Te, Tr, (sp, sn, per) = O.dense_gradients(model, T.ent, T.rel, X, negs, eta, "self_adversarial", None, "sum", R)

    def oracle(o):
        assert np.allclose(o["pos_scores"], sp, rtol=1e-5, atol=1e-5 * np.abs(sp).max())
        assert np.allclose(o["neg_scores"], sn, rtol=1e-5, atol=1e-5 * np.abs(sn).max())
        assert abs(float(o["loss"][0]) - float(total)) <= 2e-5 * max(1.0, abs(float(o["loss"][0])))
        assert_grads_close(T.dense(o["g_ent"]), Te)
        assert_grads_close(T.dense(o["g_rel"]), Tr)

    ar.expects.append(oracle)


def case_opt_step(ar, lazy, rows=123, lam=1e-3):
    """Dense: 123 rows of 9 floats = 1107 floats, the sweep's scalar tail; lazy: rows of 12 (the mode needs whole float4 rows).  The regulariser value is an fp64 atomic per block: held to
    test_gpu_kernels.py::test_opt_step_parity's bar (1e-5 of the value), tables and slots bitwise."""
    _ffi, lib = _lib()
    rng = np.random.default_rng(5)
    rf = 12 if lazy else 9
    n = rows * rf
    x0 = (rng.normal(size=(rows, rf)) * 0.5).astype(F32)
    g0 = (rng.normal(size=(rows, rf)) * (rng.random(size=(rows, 1)) < 0.7)).astype(F32)   # some rows without a gradient (lazy skips them)
    g0[-1] = 1.0
    d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, lam, 1, lazy, rf)
    x, g = ar.put("x", x0.reshape(-1), "out"), ar.put("grad", g0.reshape(-1), "out")
    s0 = ar.put("slot0", (rng.normal(size=n) * 0.01).astype(F32), "out")
    s1 = ar.put("slot1", (rng.random(size=n) * 0.01).astype(F32), "out")
    reg = ar.out("reg", (1,), F64, 0.0)
    _ffi.check(lib.amdkge_opt_step(C.byref(d), P(x), P(g), P(s0), P(s1), n, P(reg), None))
    ar.loose.add("reg")
    touched = (g0 != 0).any(1) if lazy else np.ones(rows, bool)
    want = lam * float((x0[touched].astype(F64) ** 2).sum())

    def oracle(o):
        assert abs(float(o["reg"][0]) - want) <= 1e-5 * want
        assert not o["grad"].any()                                        # the gradient is consumed
        if lazy:
            assert same_bits(o["x"].reshape(rows, rf)[~touched], x0[~touched])

    ar.expects.append(oracle)


def case_opt_step_merged(ar, n_elems, n_parts, lam=1e-3):
    """the gradient slices end with the last slice's last live element: (n_parts - 1) * part_stride + n_elems floats.  Regulariser value:
    the bar of test_gpu_shard_kernels.py::test_opt_step_merged_equals_sum_then_sweep (2e-5 of the value)."""
    _ffi, lib = _lib()
    rng = np.random.default_rng(3)
    stride = (n_elems + 3) // 4 * 4 + 4
    x0 = (rng.normal(size=n_elems) * 0.5).astype(F32)
    d = _ffi.Opt(_ffi.OPTIMIZERS["adam"], 2, 1e-2, 0.9, 0.999, 1e-7, lam, 1, 0, 0)
    x = ar.put("x", x0, "out")
    parts = ar.put("parts", (rng.normal(size=(n_parts - 1) * stride + n_elems) * 0.1).astype(F32))
    s0, s1 = ar.put("slot0", np.zeros(n_elems, F32), "out"), ar.put("slot1", np.zeros(n_elems, F32), "out")
    reg = ar.out("reg", (1,), F64, 0.0)
    _ffi.check(lib.amdkge_opt_step_merged(C.byref(d), P(x), P(parts), n_parts, stride, P(s0), P(s1), n_elems, P(reg), None))
    ar.loose.add("reg")
    want = lam * float((x0.astype(F64) ** 2).sum())
    ar.expects.append(lambda o: loss_bar(float(o["reg"][0]), want, 2e-5))


def case_tiled(ar, model, k, mode, lazy=0, direct=None):
    """amdkge_train_step_tiled through KgeEngine.train_step_tiled, every tensor of the engine replaced by a guarded one.
    mode grad_det / step_det: AMDKGE_TILED_DETERMINISTIC, gradient-only / in place -- tables, gradients and slots bitwise, the fp64 loss
        accumulators (atomics) to the oracle with the 2e-5 of test_gpu_kernels.py::test_tiled_geometries / ::test_tiled_step_in_place_parity;
    mode grad: the default (arrival-order) gradient-only step: test_gpu_kernels.py::test_tiled_geometries' bars (loss 2e-5, assert_grads_close 2e-5);
    mode grad_atomic: AMDKGE_TILED_POS_ATOMIC, the bars of ::test_tiled_gradients_parity (loss 1e-5 against the fp64 sum of the oracle's
        per-positive losses, assert_grads_close 2e-5);
    mode step: the default step in place, the bars of ::test_tiled_step_in_place_parity (loss 2e-5; tables within 1e-5 + 1e-4 |x| on 99.5 % /
        99 % of the entity / relation elements and 2.5e-2 everywhere; slots np.isclose(rtol 1e-3, atol 1e-6 + 2e-5 max) on 99.99 %);
    mode hot: AMDKGE_TILED_HOT_ROWS after amdkge_train_tiled_set_hot_rows on the guarded workspace, and mode bucket_overflow (every positive
        shares one subject: its tile's bucket overflows into the shared list): the bars of ::test_tiled_hot_rows_parity resp.
        ::test_tiled_overflow_buckets_and_duplicates (loss 2e-5, assert_grads_close tol 1e-4)."""
    _ffi, lib = _lib()
    from ampligraph_amd.engine import KgeEngine

    N, R, B, eta = (300, 3, 3000, 2) if mode == "bucket_overflow" else (300, 3, 2000, 3) if mode == "hot" else (130, 4, 37, 5)
    T = Tables(model, k, N, R, scale=0.4 if mode in ("hot", "bucket_overflow") else None)
    X = edge_triples(8, B, N, R)
    if mode == "bucket_overflow":
        X[:, 0] = 7
        X[::5, 2] = 7
    if mode == "hot":
        X[: B // 2, 0] = 7
        X[::5, 2] = 7
        X[1::7, 2] = 11
    step = mode in ("step_det", "step")
    atomic = mode == "grad_atomic"
    eng = KgeEngine(model, k, N, R, max_rel_size=R)
    assert eng.Ks == T.Ks
    eng.ent, eng.rel = ar.put("ent", T.ent_s, "out" if step else "in"), ar.put("rel", T.rel_s, "out" if step else "in")
    eng.opt_kind = "adam"
    eng.g_ent = ar.put("g_ent", np.full((N, T.Ks), 0.0 if step or atomic else 123.0, F32), "out")   # staged gradient-only form: every row is overwritten
    eng.g_rel = ar.put("g_rel", np.zeros((R, T.Ks), F32), "out")
    eng.slots = {}
    for nme in ("m", "v"):
        for tab, rows in (("e", N), ("r", R)):
            eng.slots[f"{nme}_{tab}"] = ar.put(f"slot_{nme}_{tab}", np.zeros((rows, T.Ks), F32), "out" if step else "in")
    eng.loss_acc = ar.put("loss_acc", np.zeros(3, F64), "out")
    ar.loose.add("loss_acc")
    tri = ar.put("triples", X)
    ps, ns = ar.out("pos_scores", (B,), F32, 7.0), ar.out("neg_scores", (B * eta,), F32, 7.0)
    need = int(lib.amdkge_train_tiled_workspace_bytes(C.byref(eng.model), B, eta))
    assert need > 0
    eng._twork = ar.work("twork", need)
    eng._hot_applied = False
    if mode == "hot":
        eng._hot_ids = ar.put("hot_ids", np.array([7, 11, 299], I32))
    if direct is not None:
        _ffi.check(lib.amdkge_set_tile_direct(direct))
        ar.cleanups.append(lambda: lib.amdkge_set_tile_direct(1))
    w, mk = make_optimizer("adam", {})
    w.lazy = bool(lazy)
    det = mode.endswith("_det")
    eng.train_step_tiled(tri, eta, loss_desc("self_adversarial"), w.to_ffi(1, 2), 77, 1, grad_only=not step, deterministic=det, pos_atomic=atomic, pos_scores=ps,
                         neg_scores=ns)
    assert eng._twork.data_ptr() == ar.tensor("twork").data_ptr() and bool(eng._last_tiled[2] & 4) == (mode == "hot")
    if not det:
        ar.loose |= {"g_ent", "g_rel"}
    if step:
        st = mk(T.ent, T.rel)
        ref = float(O.train_step(st, model, X, eta, "self_adversarial", 77, 1, max_rel_size=R, lazy=bool(lazy)))
        ar.expects.append(lambda o: loss_bar(float(o["loss_acc"][0] + o["loss_acc"][1]), ref, 2e-5))
        if not det:
            ar.loose |= {"ent", "rel"} | {f"slot_{a}_{b}" for a in "mv" for b in "er"}

            def tables_close(o):
                e, r = T.dense(o["ent"]), T.dense(o["rel"])
                ce, cr = np.abs(e - st.ent) <= 1e-5 + 1e-4 * np.abs(st.ent), np.abs(r - st.rel) <= 1e-5 + 1e-4 * np.abs(st.rel)
                assert ce.mean() > 0.995 and cr.mean() > 0.99 and np.abs(e - st.ent).max() < 2.5e-2, (ce.mean(), cr.mean())
                for nme, want in st.slots.items():
                    a, b = nme.split("_")
                    ok = np.isclose(T.dense(o[f"slot_{a}_{b}"]), want, rtol=1e-3, atol=1e-6 + 2e-5 * np.abs(want).max())
                    assert ok.mean() > 0.9999, (nme, ok.mean())

            ar.expects.append(tables_close)
        return
    negs = O.generate_corruptions(X, N, eta, 77, 1)
    total, Te, Tr, (_, _, per) = O.dense_gradients(model, T.ent, T.rel, X, negs, eta, "self_adversarial", None, "sum", R)
    tol = 1e-4 if mode in ("hot", "bucket_overflow") else 2e-5

    def oracle(o):
        L = float(o["loss_acc"][0])
        if atomic:
            assert abs(L - float(per.astype(np.float64).sum())) <= 1e-5 * max(1.0, abs(L)), (L, float(total))
        else:
            assert abs(L - float(total)) <= 2e-5 * max(1.0, abs(L)), (L, float(total))
        assert_grads_close(T.dense(o["g_ent"]), Te, tol=tol)
        assert_grads_close(T.dense(o["g_rel"]), Tr, tol=tol)

    ar.expects.append(oracle)


def case_cols_partial(ar, model, k, W, N=130, R=4, B=37, eta=3):
    _ffi, lib = _lib()
    T = Tables(model, k // W, N, R, k_full=k)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", edge_triples(1, B, N, R))
    out = ar.out("scores", (B * (1 + eta),), F32, 7.0)
    _ffi.check(lib.amdkge_cols_partial_scores(C.byref(T.m), P(ent), P(rel), P(tri), B, eta, 0, N, 9, 3, 0, 0, None, P(out), None))


def case_cols_loss(ar, B, eta):
    """the data loss is an fp64 atomic: test_gpu_cols.py::test_cols_phases_against_oracle's bar (3e-5); the coefficients bitwise"""
    _ffi, lib = _lib()
    T = Tables("DistMult", 8, 10, 3)
    sc0 = (np.random.default_rng(1).normal(size=B * (1 + eta)) * 2).astype(F32)
    sc = ar.put("scores", sc0, "out")
    ls = ar.out("loss", (1,), F64, 0.0)
    ld = loss_desc("self_adversarial")
    _ffi.check(lib.amdkge_cols_loss(C.byref(T.m), C.byref(ld), P(sc), B, eta, P(ls), None))
    ar.loose.add("loss")
    total = O.loss_and_grads("self_adversarial", sc0[:B], sc0[B:], eta, {"margin": ld.margin, "alpha": ld.alpha}, "sum")[0]
    ar.expects.append(lambda o: loss_bar(float(o["loss"][0]), float(total), 3e-5))


def case_platt(ar, n_pos, n_neg):
    """three fp64 atomics: the bar of test_gpu_model.py::test_platt_kernel_parity (rtol 2e-5, atol 1e-6)"""
    _ffi, lib = _lib()
    rng = np.random.default_rng(3)
    sp0, sn0 = (rng.normal(size=n_pos) * 3).astype(F32), (rng.normal(size=n_neg) * 3 - 1).astype(F32)
    _, _, labels, _, rate = O.platt_init(n_pos, n_neg)
    sp, sn = ar.put("scores_pos", sp0), ar.put("scores_neg", sn0)
    out = ar.out("out3", (3,), F64, 0.0)
    _ffi.check(lib.amdkge_platt_step(P(sp), n_pos, P(sn), n_neg, -1.5, 0.2, labels[0], labels[1], n_neg / n_pos, (1 - rate) / rate, P(out), None))
    ar.loose.add("out3")
    ref = O.platt_loss_and_grads(sp0, sn0, -1.5, 0.2, labels, rate)
    ar.expects.append(lambda o: np.testing.assert_allclose(o["out3"], ref, rtol=2e-5, atol=1e-6))


# ------------------------------------------------------------------------------------------------------------------ evaluate
def _candidates(ar, N, ids, seed=7):
    """(d_ent_ids or None, ent_lo, ent_hi): a window of the table, or of a candidate id list of `ids` entries that names the last row"""
    if not ids:
        return None, 3, N - 5
    lst = np.random.default_rng(seed).permutation(N)[:ids].astype(I32)
    lst[-2] = N - 1
    return ar.put("ent_ids", lst), 1, ids - 1


def case_rank_counts(ar, model, k, pad, n, N, kernel, ids=0, R=9):
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", edge_triples(1, n, N, R))
    d_ids, lo, hi = _candidates(ar, N, ids)
    work = ar.work("work", lib.amdkge_rank_workspace_bytes(C.byref(T.m), n))
    for side, name in ((_ffi.SIDE_S, "counts_s"), (_ffi.SIDE_O, "counts_o")):
        counts = ar.out(name, (n, 2), I32, 0)
        _ffi.check(lib.amdkge_set_rank_kernel(kernel))
        try:
            _ffi.check(lib.amdkge_rank_counts(C.byref(T.m), P(ent), P(rel), P(tri), n, side, P(d_ids), lo, hi, P(counts), P(work), None))
        finally:
            lib.amdkge_set_rank_kernel(0)
    ar.expects.append(lambda o: [np.testing.assert_array_equal(o[nm].sum(1) <= hi - lo, True) for nm in ("counts_s", "counts_o")])


def _planted_tables(model, k, N, R, n, copies, seed=5):
    """Tables and n queries (object side) for the overflowing lists: every query's object is one of `copies` rows that all hold the SAME
    values V, spread evenly over the table, so each query ties with `copies` candidates exactly -- pairs no partial sum (TransE) and, with
    the tied score on a quantisation boundary, no error bound (ComplEx) can decide."""
    T = Tables(model, k, N, R, seed=seed)
    rng = np.random.default_rng(seed)
    hot = np.linspace(0, N - 1, copies).astype(np.int64)
    V = T.ent[hot[0]].copy()
    T.ent[hot] = V
    X = rand_triples(rng, n, N, R)
    X[:, 2] = hot[rng.integers(0, copies, n)]
    if model == "ComplEx":         # V = (1 + 0i) in unit 0 and nothing else; every subject (1 + 0i) there, every relation real part 1: the tied
        cold = np.setdiff1d(np.arange(N), hot)   # scores are exactly 1.0 = 1000 quanta, a value no error bound can keep on one side
        X[:, 0] = cold[np.arange(n) % cold.size]
        V = np.zeros_like(V)
        V[0] = 1.0
        T.ent[hot] = V
        T.ent[cold, 0], T.ent[cold, k], T.rel[:, 0] = 1.0, 0.0, 1.0
    if model == "TransE":          # s + p lands next to V: the positive (and its copies) score near the top, everything else is decided early
        cold = np.setdiff1d(np.arange(N), hot)
        X[:, 0] = cold[np.arange(n) % cold.size]
        T.ent[cold] += 3.0
        for i in range(n):
            T.ent[X[i, 0]] = V - T.rel[X[i, 1]] + rng.normal(size=V.shape).astype(F32) * 0.01
    return T, X


def case_screened(ar, model, k, how, R=7):
    """amdkge_rank_counts_screened on the smallest problem its passes accept (contraction models: n >= 128 queries and >= 512 candidates,
    the int8 screening pass -- ComplEx k = 50: rank_screen_kernel_r, DistMult k = 50: rank_screen_kernel_v1; TransE / RotatE: n >= 64, >= 256
    candidates, >= 64 units, the exact early exit with its probe off).  Counts are integers: everything bitwise, and equal to the plain
    kernel's (amdkge_set_rank_kernel 3 resp. 1, as test_gpu_rank_screen.py / test_gpu_rank_early.py anchor them).
      how null           d_screen = NULL: the documented fall-back;
      how too_small      screen_bytes one byte below the smallest size the passes accept (their fixed part + 64 KiB of list): the other
                         documented fall-back -- d_screen is an INPUT of this case: not one byte of it may change;
      how one_byte_short one byte less than amdkge_rank_screen_workspace_bytes: the pass runs on a list one entry shorter (what
                         test_gpu_rank_screen.py::test_screened_overflowing_recheck_list_falls_back relies on) inside the bytes it was given;
      how overflow       room for 8 200 pairs and planted ties far beyond it: flag and count as that test (resp.
                         test_gpu_rank_early.py::test_early_exit_overflowing_list_falls_back) asserts them, counts from the fall-back."""
    _ffi, lib = _lib()
    dist = model in ("TransE", "RotatE")
    n, N = (200, 531) if dist and how == "overflow" else (70, 270) if dist else (130, 531)
    if how == "overflow":
        T, X = _planted_tables(model, k, N, R, n, copies=56 if dist else 100)
        lo, hi = 0, N
    else:
        T, X = Tables(model, k, N, R), edge_triples(1, n, N, R)
        lo, hi = 3, N - 5
    mcand = hi - lo
    side = _ffi.SIDE_O
    if dist:
        _ffi.check(lib.amdkge_set_rank_early(1, 1, 1, 1, 0) if how == "overflow" else lib.amdkge_set_rank_early(1, 4, 1, 16, 0))
        ar.cleanups.append(lambda: lib.amdkge_set_rank_early(1, 4, 1, 16, 1))
    need = int(lib.amdkge_rank_screen_workspace_bytes(C.byref(T.m), n, mcand))
    pairs = max(1 << 18 if dist else 1 << 20, n * mcand // 32)      # the list's entries inside `need` (kge_rank.hip)
    least = need - pairs * 8 - 512 + (1 << 16)                       # the smallest workspace the passes accept
    assert need > least > 0
    nbytes = {"screen": need, "null": 0, "too_small": least - 1, "one_byte_short": need - 1, "overflow": need - (pairs - 8200) * 8}[how]
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    work = ar.work("work", lib.amdkge_rank_workspace_bytes(C.byref(T.m), n))
    counts = ar.out("counts", (n, 2), I32, 0)
    if how == "too_small":
        screen = ar.put("screen", np.full(nbytes, 0x5A, U8), "in", offset=16)
    else:
        screen = ar.work("screen", nbytes)
    _ffi.check(lib.amdkge_rank_counts_screened(C.byref(T.m), P(ent), P(rel), P(tri), n, side, None, lo, hi, P(counts), P(work), P(screen), nbytes, None))
    # the anchor: the plain kernel on ordinary tensors
    pe, pr, px = (torch.as_tensor(a).cuda() for a in (T.ent_s, T.rel_s, X))
    pw = torch.empty(int(lib.amdkge_rank_workspace_bytes(C.byref(T.m), n)), dtype=torch.uint8, device="cuda")
    pc = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    _ffi.check(lib.amdkge_set_rank_kernel(1 if dist else 3))
    try:
        _ffi.check(lib.amdkge_rank_counts(C.byref(T.m), P(pe), P(pr), P(px), n, side, None, lo, hi, P(pc), P(pw), None))
    finally:
        lib.amdkge_set_rank_kernel(0)
    torch.cuda.synchronize()
    exact = pc.cpu().numpy()
    head = None
    if how in ("screen", "one_byte_short", "overflow"):
        off = (-screen.data_ptr()) % 256                              # the statistics words: the workspace aligned up to 256 bytes
        head = screen[off:off + 12].cpu().numpy().view(I32)

    def expect(o):
        np.testing.assert_array_equal(o["counts"], exact)
        if how == "overflow":
            assert head[1] != 0 and head[0] > 8200, head
        elif head is not None:
            assert head[1] == 0, head
            if not dist:
                assert head[0] > 0, head                              # the screening pass really ran (some pairs always need the exact chain)

    ar.expects.append(expect)


def _filter_data(form, m, N=23, R=5, seed=3):
    X = rand_triples(np.random.default_rng(seed), m, N, R)
    X[: m // 3] = X[0]                                                # duplicates: the datasets may overlap
    X[-1] = (N - 1, R - 1, N - 1)
    return X, N, R


def _filter_ref(X, form, N, R):
    """the CSR of amdkge_filter_build / amdkge_pair_filter_build in numpy: (keys, start, ids)"""
    X = X.astype(np.int64)
    key = {"s": X[:, 1] * N + X[:, 2], "o": X[:, 0] * R + X[:, 1], "pair": X[:, 0] * N + X[:, 2]}[form]
    val = {"s": X[:, 0], "o": X[:, 2], "pair": X[:, 1]}[form]
    kv = np.unique(np.stack([key, val], 1), axis=0)
    keys, first = np.unique(kv[:, 0], return_index=True)
    return keys, np.append(first, len(kv)).astype(I64), kv[:, 1].astype(I32)


def case_filter_build(ar, form, m):
    """the outputs are valid up to n_groups / n_unique (d_counts); what lies behind is unspecified, so the compared form is the valid part"""
    _ffi, lib = _lib()
    X, N, R = _filter_data(form, m)
    tri = ar.put("triples", X)
    keys, start, ids = ar.out("keys", (m,), I64, 1), ar.out("start", (m + 1,), I64, 1), ar.out("ids", (m,), I32, 1)
    counts = ar.out("counts", (2,), I64, 0)
    work = ar.work("work", lib.amdkge_filter_build_workspace_bytes(m, N, R))
    if form == "pair":
        _ffi.check(lib.amdkge_pair_filter_build(P(tri), m, N, R, P(keys), P(start), P(ids), P(counts), P(work), None))
    else:
        _ffi.check(lib.amdkge_filter_build(P(tri), m, 1 if form == "s" else 2, N, R, P(keys), P(start), P(ids), P(counts), P(work), None))
    ar.canon["keys"] = lambda v, o: v[:o["counts"][0]]
    ar.canon["start"] = lambda v, o: v[:o["counts"][0] + 1]
    ar.canon["ids"] = lambda v, o: v[:o["counts"][1]]
    rk, rs, ri = _filter_ref(X, form, N, R)

    def expect(o):
        ng, nu = (int(c) for c in o["counts"])
        assert (ng, nu) == (len(rk), len(ri))
        assert np.array_equal(o["keys"][:ng], rk) and np.array_equal(o["start"][:ng + 1], rs) and np.array_equal(o["ids"][:nu], ri)

    ar.expects.append(expect)


def case_filter_ranges(ar, form, n):
    _ffi, lib = _lib()
    F, N, R = _filter_data(form, 130)
    rk, rs, _ = _filter_ref(F, form, N, R)
    X = rand_triples(np.random.default_rng(9), n, N, R)
    X[0] = F[-1]                                                      # the last key of the index
    keys, start, tri = ar.put("keys", rk.astype(I64)), ar.put("start", rs), ar.put("triples", X)
    lo, hi = ar.out("lo", (n,), I64, 1), ar.out("hi", (n,), I64, 1)
    if form == "pair":
        _ffi.check(lib.amdkge_pair_filter_ranges(P(keys), P(start), len(rk), P(tri), n, N, P(lo), P(hi), None))
    else:
        _ffi.check(lib.amdkge_filter_ranges(P(keys), P(start), len(rk), P(tri), n, 1 if form == "s" else 2, N, R, P(lo), P(hi), None))
    X64 = X.astype(np.int64)
    q = {"s": X64[:, 1] * N + X64[:, 2], "o": X64[:, 0] * R + X64[:, 1], "pair": X64[:, 0] * N + X64[:, 2]}[form]
    pos = np.searchsorted(rk, q)
    hit = (pos < len(rk)) & (rk[np.minimum(pos, len(rk) - 1)] == q)
    want_lo, want_hi = np.where(hit, rs[np.minimum(pos, len(rk) - 1)], 0), np.where(hit, rs[np.minimum(pos + 1, len(rk))], 0)
    ar.expects.append(lambda o: (np.testing.assert_array_equal(o["lo"], want_lo), np.testing.assert_array_equal(o["hi"], want_hi)))


def case_rank_filter(ar, model, k, subset, n=37, N=130, R=5):
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad=k % 4 == 0 or model != "TransE")
    rng = np.random.default_rng(2)
    X = edge_triples(2, n, N, R)
    cnt = rng.integers(0, 6, n)
    cnt[-1] = 5
    start = np.zeros(n + 1, I64)
    start[1:] = np.cumsum(cnt)
    ids = rng.integers(0, N, int(start[-1])).astype(I32)
    ids[-1] = N - 1
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    lo, hi, fid = ar.put("flt_lo", start[:-1].copy()), ar.put("flt_hi", start[1:].copy()), ar.put("flt_ids", ids)
    spos = None
    if subset:
        pos = np.full(N, -1, I32)
        sel = rng.permutation(N)[:40]
        pos[sel] = np.arange(40, dtype=I32)
        spos = ar.put("subset_pos", pos)
    sub = ar.out("sub", (n,), I32, 0)
    work = ar.work("work", lib.amdkge_rank_workspace_bytes(C.byref(T.m), n))
    _ffi.check(lib.amdkge_rank_filter(C.byref(T.m), P(ent), P(rel), P(tri), n, _ffi.SIDE_S, P(lo), P(hi), P(fid), P(spos), 3, N - 5, P(sub), P(work), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal((o["sub"] >= 0) & (o["sub"] <= cnt), True))


def case_rank_compose(ar, n, stride, sub):
    _ffi, lib = _lib()
    rng = np.random.default_rng(1)
    c0 = rng.integers(0, 50, (n, 2)).astype(I32)
    s0 = rng.integers(0, 3, n).astype(I32)
    counts, d_sub = ar.put("counts", c0), (ar.put("sub", s0) if sub else None)
    ranks = ar.out("ranks", ((n - 1) * stride + 1,), I32, 1)          # rank i at i * stride: the buffer ends with the last rank
    _ffi.check(lib.amdkge_rank_compose(P(counts), P(d_sub), n, _ffi.RANK_STRATEGY["worst"], P(ranks), stride, None))
    ar.keep("ranks", np.arange((n - 1) * stride + 1) % stride != 0)
    want = c0.sum(1) - (s0 if sub else 0) + 1
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["ranks"][::stride], want))


# ------------------------------------------------------------------------------------------------------------------ discovery
def case_corruption_scores(ar, model, k, n, N, ids, R=9):
    """the score block is strided: ld = m + 15, and ends with the last query's last candidate"""
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad=(k % 4 == 0) or model != "TransE")
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", edge_triples(1, n, N, R))
    d_ids, lo, hi = _candidates(ar, N, ids)
    m = hi - lo
    ld = m + 15
    work = ar.work("work", lib.amdkge_rank_workspace_bytes(C.byref(T.m), n))
    for side, name in ((_ffi.SIDE_S, "scores_s"), (_ffi.SIDE_O, "scores_o")):
        out = ar.out(name, ((n - 1) * ld + m,), F32, 7.0)
        _ffi.check(lib.amdkge_corruption_scores(C.byref(T.m), P(ent), P(rel), P(tri), n, side, P(d_ids), lo, hi, P(out), ld, P(work), None))
        ar.keep(name, ~block_mask(n, m, ld))


def case_row_dots(ar, n, Kf, N, ids):
    _ffi, lib = _lib()
    rng = np.random.default_rng(4)
    q, table = ar.put("q", rng.normal(size=(n, Kf)).astype(F32)), ar.put("table", rng.normal(size=(N, Kf)).astype(F32))
    d_ids, lo, hi = _candidates(ar, N, ids)
    m = hi - lo
    ld = m + 15
    out = ar.out("out", ((n - 1) * ld + m,), F32, 7.0)
    _ffi.check(lib.amdkge_row_dots(P(q), n, P(table), Kf, P(d_ids), lo, hi, P(out), ld, None))
    ar.keep("out", ~block_mask(n, m, ld))


def case_row_sqnorms(ar, Kf, N, ids, rsqrt):
    _ffi, lib = _lib()
    table = ar.put("table", np.random.default_rng(4).normal(size=(N, Kf)).astype(F32))
    d_ids, lo, hi = _candidates(ar, N, ids)
    out = ar.out("out", (hi - lo,), F32, 7.0)
    _ffi.check(lib.amdkge_row_sqnorms(P(table), Kf, P(d_ids), lo, hi - lo, -0.5, rsqrt, P(out), None))


def case_topk(ar, n, m, k, extras, largest=1):
    _ffi, lib = _lib()
    rng = np.random.default_rng(6)
    ld = m + 15
    size = (n - 1) * ld + m
    vals = ar.put("vals", np.round(rng.normal(size=size), 1).astype(F32))   # (rounded: equal values, decided by the column)
    scale = ar.put("col_scale", rng.uniform(0.5, 2, m).astype(F32)) if extras else None
    bias = ar.put("col_bias", rng.normal(size=m).astype(F32)) if extras else None
    payload = ar.put("payload", rng.integers(0, 1000, size).astype(I32)) if extras else None
    idx, val = ar.out("out_idx", (n, k), I32, 1), ar.out("out_val", (n, k), F32, 7.0)
    _ffi.check(lib.amdkge_topk_rows(P(vals), n, m, ld, P(scale), P(bias), P(payload), k, largest, P(idx), P(val), None))
    if not extras:
        ar.expects.append(lambda o: np.testing.assert_array_equal((o["out_idx"] >= -1) & (o["out_idx"] < m), True))


def case_topk_excluding(ar, n, m, k, ids):
    _ffi, lib = _lib()
    rng = np.random.default_rng(6)
    ld = m + 15
    vals = ar.put("vals", np.round(rng.normal(size=(n - 1) * ld + m), 1).astype(F32))
    col = np.sort(rng.permutation(4 * m)[:m]).astype(I32)
    col_ids = ar.put("col_ids", col) if ids else None
    cnt = rng.integers(0, 6, n)
    start = np.zeros(n + 1, I64)
    start[1:] = np.cumsum(cnt + 1)
    ex = np.concatenate([np.sort(rng.choice(col if ids else np.arange(5, 5 + m), c + 1, replace=False)) for c in cnt]).astype(I32)
    lo, hi, exi = ar.put("ex_lo", start[:-1].copy()), ar.put("ex_hi", start[1:].copy()), ar.put("ex_ids", ex)
    own = ar.put("own", (col if ids else np.arange(5, 5 + m))[rng.integers(0, m, n)].astype(I32))
    idx, val = ar.out("out_idx", (n, k), I32, 1), ar.out("out_val", (n, k), F32, 7.0)
    _ffi.check(lib.amdkge_topk_rows_excluding(P(vals), n, m, ld, P(col_ids), 5, P(lo), P(hi), P(exi), P(own), k, P(idx), P(val), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal((o["out_idx"] >= -1) & (o["out_idx"] < m), True))


def case_pair_distances(ar, n, Kf, k, cosine, N=130):
    _ffi, lib = _lib()
    rng = np.random.default_rng(4)
    q, table = ar.put("q", rng.normal(size=(n, Kf)).astype(F32)), ar.put("table", rng.normal(size=(N, Kf)).astype(F32))
    lst = rng.permutation(N)[:40].astype(I32)
    lst[-1] = N - 1
    d_ids = ar.put("ids", lst)
    pos0 = rng.integers(-1, 37, (n, k)).astype(I32)
    pos0[-1, -1] = 36                                                 # lo + pos = the list's last entry = the table's last row
    pos = ar.put("pos", pos0)
    out = ar.out("out", (n, k), F32, 7.0)
    _ffi.check(lib.amdkge_pair_distances(P(q), n, P(table), Kf, P(d_ids), 3, P(pos), k, cosine, P(out), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal(np.isinf(o["out"]), pos0 < 0))


def _points(n, d, seed=1):
    """rows in a few tight groups: neighbours, clusters and duplicates exist at every n"""
    rng = np.random.default_rng(seed)
    X = (rng.integers(0, 5, (n, 1)) * 4.0 + rng.normal(size=(n, d)) * 0.2).astype(F32)
    if n > 4:
        X[-1] = X[0]
    return X


def case_join_nearest(ar, n, d):
    _ffi, lib = _lib()
    x = ar.put("x", _points(n, d))
    dist, idx, mx = ar.out("dist", (n,), F32, 7.0), ar.out("idx", (n,), I32, 1), ar.out("max", (1,), F32, 7.0)
    work = ar.put("work", np.zeros(8 * n, U8), "work")               # 8 n bytes of 8-byte keys: not self-aligned by the library
    _ffi.check(lib.amdkge_join_nearest(P(x), n, d, P(dist), P(idx), P(mx), P(work), None))
    if n > 4:
        ar.expects.append(lambda o: (o["idx"][-1] == 0 and o["dist"][-1] == 0.0) or pytest.fail("the planted duplicate was not found"))


def _sorted_pairs(v, count):
    v = v[:count]
    return v[np.lexsort((v[:, 1], v[:, 0]))]


def case_join_radius(ar, n, d, overflow):
    """the pair list is filled in no particular order: compared as a sorted set.  overflow: cap = 37 against thousands of pairs -- the count
    is the true one (test_gpu_duplicates.py relaunches on it), the list holds exactly cap distinct valid pairs (WHICH ones is arrival
    order: not compared between the runs), the band behind it is clean."""
    _ffi, lib = _lib()
    X = _points(n, d)
    thr = 0.2 * 0.2 * 2 * d * 4
    d2 = ((X[:, None, :].astype(F64) - X[None, :, :]) ** 2).sum(-1)
    iu = np.triu_indices(n, 1)
    true = int((d2[iu] <= thr * 0.999).sum())
    cap = 37 if overflow else int((d2[iu] <= thr * 1.001).sum()) + 3
    assert true > (20 * cap if overflow else 50)
    x = ar.put("x", X)
    pairs, count = ar.out("pairs", (cap, 2), I32, 1), ar.out("count", (1,), I64, 1)
    _ffi.check(lib.amdkge_join_radius(P(x), n, d, thr, P(pairs), cap, P(count), None))
    if overflow:
        ar.loose.add("pairs")
    else:
        ar.canon["pairs"] = lambda v, o: _sorted_pairs(v, int(o["count"][0]))

    def expect(o):
        c = int(o["count"][0])
        assert (c > cap) == overflow and c >= true
        p = o["pairs"][:min(c, cap)].astype(np.int64)
        assert ((0 <= p[:, 0]) & (p[:, 0] < p[:, 1]) & (p[:, 1] < n)).all() and len(np.unique(p, axis=0)) == len(p)
        assert (d2[p[:, 0], p[:, 1]] <= thr * 1.001).all()
        assert same_bits(o["pairs"][min(c, cap):], np.full((cap - min(c, cap), 2), 1, I32))   # nothing behind the count

    ar.expects.append(expect)


def case_join_dbscan(ar, n, d):
    _ffi, lib = _lib()
    x = ar.put("x", _points(n, d))
    labels, core, ncl = ar.out("labels", (n,), I32, 1), ar.out("core", (n,), U8, 1), ar.out("n_clusters", (1,), I32, 1)
    work = ar.put("work", np.zeros(int(lib.amdkge_join_dbscan_workspace_bytes(n)), U8), "work")   # three int32 arrays: not self-aligned
    _ffi.check(lib.amdkge_join_dbscan(P(x), n, d, 0.2 * 0.2 * 2 * d * 4, 3, P(labels), P(core), P(ncl), P(work), None))
    ar.expects.append(lambda o: 1 <= int(o["n_clusters"][0]) <= 5 or pytest.fail(str(o["n_clusters"])))


def case_kmeans_assign(ar, n, d, k, runs):
    _ffi, lib = _lib()
    X = _points(n, d)
    rng = np.random.default_rng(2)
    cen = np.stack([X[rng.permutation(n)[:k]] for _ in range(runs)])
    x, c = ar.put("x", X), ar.put("centres", cen)
    labels, mind2 = ar.out("labels", (runs, n), I32, 1), ar.out("mind2", (runs, n), F32, 7.0)
    _ffi.check(lib.amdkge_kmeans_assign(P(x), n, d, P(c), k, runs, P(labels), P(mind2), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal((o["labels"] >= 0) & (o["labels"] < k), True))


def case_kmeans_lloyd(ar, n, d, k, runs):
    _ffi, lib = _lib()
    X = _points(n, d)
    rng = np.random.default_rng(2)
    cen = np.stack([X[rng.permutation(n)[:k]] for _ in range(runs)])
    x, c = ar.put("x", X), ar.put("centres", cen, "out")
    labels, mind2 = ar.out("labels", (runs, n), I32, -1), ar.out("mind2", (runs, n), F32, 7.0)
    state, inertia = ar.out("state", (runs, 4), I32, 0), ar.out("inertia", (runs,), F64, 0.0)
    need = int(lib.amdkge_kmeans_workspace_bytes(n, d, k, runs))
    assert need > 0
    work = ar.put("work", np.zeros(need, U8), "work")                # parts on 8-byte boundaries of the pointer: not self-aligned
    _ffi.check(lib.amdkge_kmeans_lloyd(P(x), n, d, P(c), k, runs, 3, 0.0, P(labels), P(mind2), P(state), P(inertia), P(work), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["state"][:, 0] >= 1, True))


def case_discover_select(ar, n, m, overflow, given):
    """the pair list follows amdkge_join_radius' protocol: sorted set, or -- overflowing -- cap valid distinct pairs and the true count"""
    _ffi, lib = _lib()
    rng = np.random.default_rng(5)
    ld = m + 15
    sc0 = np.round(rng.normal(size=(n - 1) * ld + m), 2).astype(F32)
    Q = rand_triples(rng, n, m, 3)
    cnt = rng.integers(0, 4, n)
    start = np.zeros(n + 1, I64)
    start[1:] = np.cumsum(cnt + 1)
    fids = np.concatenate([np.sort(rng.choice(m, c + 1, replace=False)) for c in cnt]).astype(I32)
    R, margin = (m if overflow else 3), 5
    cap = 37 if overflow else 4 * n * (3 + 8) + 64
    scores, queries = ar.put("scores", sc0), ar.put("queries", Q)
    lo, hi, fid = ar.put("flt_lo", start[:-1].copy()), ar.put("flt_hi", start[1:].copy()), ar.put("flt_ids", fids)
    thr0 = np.full(n, -3000, I32)
    thr = ar.put("thr", thr0, "in") if given else ar.out("thr", (n,), I32, 1)
    pairs, count = ar.out("pairs", (cap, 2), I32, 1), ar.out("count", (1,), I64, 1)
    _ffi.check(lib.amdkge_discover_select(P(scores), n, m, ld, P(queries), _ffi.SIDE_O, P(lo), P(hi), P(fid), R, margin, P(thr), given, 100, P(pairs), cap,
                                          P(count), None))
    if overflow:
        ar.loose.add("pairs")
    else:
        ar.canon["pairs"] = lambda v, o: _sorted_pairs(v, int(o["count"][0]))
    blk = np.full((n, m), np.nan, F32)
    for i in range(n):
        blk[i] = sc0[i * ld:i * ld + m]
    qz = np.trunc(blk * np.float32(1000.0)).astype(np.int64)          # the rank kernels' quantisation, in fp32

    def expect(o):
        c = int(o["count"][0])
        assert (c > cap) == overflow, (c, cap)
        p = o["pairs"][:min(c, cap)].astype(np.int64)
        row, colj = p[:, 0] - 100, p[:, 1]
        assert ((0 <= row) & (row < n) & (0 <= colj) & (colj < m)).all() and len(np.unique(p, axis=0)) == len(p)
        T_ = thr0 if given else o["thr"]
        for r, j in zip(row, colj):
            assert j != Q[r, 0] and j not in fids[start[r]:start[r + 1]] and qz[r, j] >= int(T_[r]) - margin, (r, j)
        assert same_bits(o["pairs"][min(c, cap):], np.full((cap - min(c, cap), 2), 1, I32))

    ar.expects.append(expect)


# ------------------------------------------------------------------------------------------------------------------ relation prediction
def case_relation_scores(ar, model, k, n, R, ids, N=130):
    _ffi, lib = _lib()
    T = Tables(model, k, N, R, pad=(k % 4 == 0) or model != "TransE")
    X = edge_triples(1, n, N, R)
    ent, rel, tri = ar.put("ent", T.ent_s), ar.put("rel", T.rel_s), ar.put("triples", X)
    if ids:
        lst = np.random.default_rng(7).permutation(R)[:ids].astype(I32)
        lst[-2] = R - 1
        d_ids, lo, hi = ar.put("rel_ids", lst), 1, ids - 1
    else:
        lst, d_ids, lo, hi = np.arange(R), None, (3 if R > 20 else 0), (R - 5 if R > 20 else R)
    m = hi - lo
    ld = m + 15
    out = ar.out("scores", ((n - 1) * ld + m,), F32, 7.0)
    need = int(lib.amdkge_relation_workspace_bytes(C.byref(T.m), m))
    assert need >= 0 and (need > 0) == (model == "RotatE")
    work = ar.work("work", need)
    _ffi.check(lib.amdkge_relation_scores(C.byref(T.m), P(ent), P(rel), P(tri), n, P(d_ids), lo, hi, P(out), ld, P(work), None))
    ar.keep("scores", ~block_mask(n, m, ld))
    # every score has the bits amdkge_score gives the materialised triple (include/amdkge.h): the anchor, on ordinary tensors
    M = np.repeat(X, m, axis=0)
    M[:, 1] = np.tile(lst[lo:hi], n)
    pe, pr, px = (torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in (T.ent_s, T.rel_s, M))
    ref = torch.empty(n * m, dtype=torch.float32, device="cuda")
    _ffi.check(lib.amdkge_score(C.byref(T.m), P(pe), P(pr), P(px), n * m, P(ref), None))
    torch.cuda.synchronize()
    ref = ref.cpu().numpy().reshape(n, m)
    ar.expects.append(lambda o: [same_bits(o["scores"][i * ld:i * ld + m], ref[i]) or pytest.fail(f"row {i} differs from amdkge_score") for i in range(n)])


def case_relation_rank_counts(ar, n, m, flt):
    _ffi, lib = _lib()
    rng = np.random.default_rng(5)
    ld = m + 15
    n_rels = 2 * m
    sc0 = np.round(rng.normal(size=(n - 1) * ld + m), 2).astype(F32)
    col = rng.permutation(n_rels)[:m].astype(I32)
    scores, pos, col_ids = ar.put("scores", sc0), ar.put("pos", np.round(rng.normal(size=n), 2).astype(F32)), ar.put("col_ids", col)
    counts = ar.out("counts", (n, 2), I32, 0)
    lo = hi = fid = spos = sub = None
    if flt:
        cnt = rng.integers(0, 4, n)
        start = np.zeros(n + 1, I64)
        start[1:] = np.cumsum(cnt + 1)
        fids = np.concatenate([np.sort(rng.choice(n_rels, c + 1, replace=False)) for c in cnt]).astype(I32)
        lo, hi, fid = ar.put("flt_lo", start[:-1].copy()), ar.put("flt_hi", start[1:].copy()), ar.put("flt_ids", fids)
        sp = np.full(n_rels, -1, I32)
        sp[col] = np.arange(m, dtype=I32)
        spos = ar.put("subset_pos", sp)
        sub = ar.out("sub", (n,), I32, 0)
    _ffi.check(lib.amdkge_relation_rank_counts(P(scores), n, m, ld, P(pos), P(col_ids), 0, P(lo), P(hi), P(fid), P(spos), P(counts), P(sub), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["counts"].sum(1) <= m, True))


# ------------------------------------------------------------------------------------------------------------------ multi-GPU data path
def case_shard_route(ar, b, nneg, cap, N=1000, world=4, rank=2):
    """Request slots are handed out in arrival order: the compared form of the rewritten batch maps every scratch row back to the global id
    its request list holds, and of the lists their sorted content.  cap = 9 is below every owner's count: the sticky flag is set (what
    test_gpu_shard_kernels.py::test_shard_route_invariants asserts), every list is full of valid row indices, the band behind is clean."""
    _ffi, lib = _lib()
    rng = np.random.default_rng(world * 100 + rank)
    X = rand_triples(rng, b, N, 5)
    X[: b // 4, 0] = X[0, 0]
    X[-1, 2] = N - 1
    negs = rand_triples(rng, nneg, N, 5) if nneg else None
    rows_per = (N + world - 1) // world
    r_lo, r_hi = rows_per * rank, min(N, rows_per * (rank + 1))
    tri = ar.put("triples", X)
    d_negs = ar.put("negs", negs) if nneg else None
    xl = ar.out("out_triples", (b, 3), I32, 1)
    nl = ar.out("out_negs", (nneg, 3), I32, 1) if nneg else None
    send, counts = ar.out("send_ids", (world * cap,), I32, 1), ar.out("counts", (world + 1,), I32, 0)
    work = ar.work("work", lib.amdkge_shard_route_workspace_bytes(b, nneg))
    _ffi.check(lib.amdkge_shard_route(N, world, rank, P(tri), b, P(d_negs), nneg, cap, P(xl), P(nl), P(send), P(counts), P(work), None))
    ids = np.concatenate([X[:, 0], X[:, 2]] + ([negs[:, 0], negs[:, 2]] if nneg else [])).astype(np.int64)
    local = (ids >= r_lo) & (ids < r_hi)
    want = np.bincount(np.unique(ids[~local]) // rows_per, minlength=world)
    overflow = bool((want > cap).any())
    assert overflow == (cap == 9) and (not overflow or (want[np.arange(world) != rank] > cap).all())

    def back(v, o):   # local index space -> global ids
        v = v.astype(np.int64).copy()
        for c in (0, 2):
            remote = v[:, c] >= r_hi - r_lo
            slot = v[remote, c] - (r_hi - r_lo)
            v[remote, c] = o["send_ids"][slot].astype(np.int64) + (slot // cap) * rows_per
            v[~remote, c] += r_lo
        return v

    if overflow:
        ar.loose |= {"out_triples", "send_ids"}
    else:
        ar.canon["out_triples"] = back
        ar.canon["out_negs"] = back
        ar.canon["send_ids"] = lambda v, o: np.sort(v.reshape(world, cap), axis=1)

    def expect(o):
        assert np.array_equal(o["counts"][:world], want) and bool(o["counts"][world]) == overflow
        lists = o["send_ids"].reshape(world, cap)
        for q in range(world):
            fill = min(int(want[q]), cap)
            rows_q = min(N, rows_per * (q + 1)) - rows_per * q
            assert ((lists[q, :fill] >= 0) & (lists[q, :fill] < rows_q)).all() and (lists[q, fill:] == -1).all()
            assert len(np.unique(lists[q, :fill])) == fill
        if not overflow:
            assert np.array_equal(back(o["out_triples"], o), X) and (not nneg or np.array_equal(back(o["out_negs"], o), negs))

    ar.expects.append(expect)


def case_gather_rows(ar, Kf, n, N=130):
    _ffi, lib = _lib()
    rng = np.random.default_rng(1)
    t0 = rng.normal(size=(N, Kf)).astype(F32)
    i0 = rng.integers(-1, N, n).astype(I32)
    i0[-1] = N - 1
    table, idx = ar.put("table", t0), ar.put("idx", i0)
    out = ar.out("out", (n, Kf), F32, 7.0)
    _ffi.check(lib.amdkge_gather_rows(P(table), Kf, P(idx), n, P(out), None))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["out"], np.where(i0[:, None] < 0, 0, t0[np.maximum(i0, 0)]).astype(F32)))


def case_scatter_add_rows(ar, Kf, n, N=130):
    """fp32 atomics onto repeated rows.  The addends are small integers, whose fp32 sums are exact in every order: the result is one bit
    pattern however the atomics arrive, so (b) and (c) stay bitwise and equal the integer sum."""
    _ffi, lib = _lib()
    rng = np.random.default_rng(1)
    i0 = rng.integers(-1, N, n).astype(I32)
    i0[:7 if n > 7 else 1] = 11
    i0[-1] = N - 1
    s0 = rng.integers(-8, 9, (n, Kf)).astype(F32)
    t0 = rng.integers(-8, 9, (N, Kf)).astype(F32)
    table, idx, src = ar.put("table", t0, "out"), ar.put("idx", i0), ar.put("src", s0)
    _ffi.check(lib.amdkge_scatter_add_rows(P(table), Kf, P(idx), n, P(src), None))
    want = t0.astype(F64)
    np.add.at(want, i0[i0 >= 0], s0[i0 >= 0].astype(F64))
    ar.expects.append(lambda o: np.testing.assert_array_equal(o["table"], want.astype(F32)))


def case_synth_triples(ar, n):
    _ffi, lib = _lib()
    out = ar.out("out", (n, 3), I32, 1)
    _ffi.check(lib.amdkge_synth_triples(12345678901, 10**9 + 7, n, 50_000_000, 1000, P(out), None))
    ar.expects.append(lambda o: (o["out"][:, 1] < 1000).all() and (o["out"][:, [0, 2]] < 50_000_000).all() or pytest.fail("ids out of range"))


# ------------------------------------------------------------------------------------------------------------------ session layer
def case_session(ar, what):
    """Host arrays the session layer fills (guarded_host).  n = 37: no multiple of the query chunk of the row-sharded group (scratch rows
    / 2 with max_batch = 8), of the replica count, or of any tile."""
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.session import Session, SessionGroup

    _ffi, lib = _lib()
    N, R, k, n = 130, 5, 7, 37
    T = Tables("ComplEx", k, N, R, pad=False)
    X = edge_triples(3, n, N, R)
    mk = lambda: (loss_functions.get("nll"), optimizers.get("adam", {"learning_rate": 1e-2}))   # noqa: E731
    group = what.startswith("group")
    s = (SessionGroup([0, 0], "ComplEx", k, N, R, 3, *mk(), rows=what == "group_get_rows", max_batch=8 if what == "group_get_rows" else None)
         if group else Session("ComplEx", k, N, R, 3, *mk()))
    try:
        s.set_rows("ent", T.ent)
        s.set_rows("rel", T.rel)
        h = s._g if group else s._h
        if what == "score":
            out = ar.host("scores", (n,), F32, 7.0)
            _ffi.check(lib.amdkge_session_score(h, HP(X), n, HP(out)))
        elif what in ("rank", "group_rank"):
            cnt = np.random.default_rng(1).integers(0, 4, n)
            off = np.zeros(n + 1, I64)
            off[1:] = np.cumsum(cnt)
            fid = np.random.default_rng(2).integers(0, N, int(off[-1])).astype(I32)
            out = ar.host("ranks", (n, 2), I32, 1)
            fn = lib.amdkge_session_group_rank if group else lib.amdkge_session_rank
            _ffi.check(fn(h, HP(X), n, HP(off), HP(fid), HP(off), HP(fid), None, 0, _ffi.CORRUPT_SIDES["s,o"], _ffi.RANK_STRATEGY["worst"], HP(out)))
            ar.expects.append(lambda o: np.testing.assert_array_equal((o["ranks"] >= 1) & (o["ranks"] <= N + 1), True))
        else:
            fn = lib.amdkge_session_group_get_rows if group else lib.amdkge_session_get_rows
            ids = np.random.default_rng(4).integers(0, N, n).astype(I32)
            ids[-1] = N - 1
            by_id, by_range = ar.host("rows_by_id", (n, 2 * k), F32, 7.0), ar.host("rows_by_range", (n, 2 * k), F32, 7.0)
            _ffi.check(fn(h, _ffi.TABLES["ent"], HP(ids), 0, n, HP(by_id)))
            _ffi.check(fn(h, _ffi.TABLES["ent"], None, N - n, n, HP(by_range)))
            ar.expects.append(lambda o: (np.testing.assert_array_equal(o["rows_by_id"], T.ent[ids]), np.testing.assert_array_equal(o["rows_by_range"], T.ent[N - n:])))
    finally:
        s.close()
