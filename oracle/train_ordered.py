"""TEST INFRASTRUCTURE -- second oracle mode for fit(): one training step in the kernels' DECLARED fp32 order.

`oracle/kge_oracle.py` restates ScoringBasedEmbeddingModel.train_step (ScoringBasedEmbeddingModel.py:370-429) with fp64
accumulation.  For the models that are smooth in their parameters that is enough: GPU and oracle trajectories stay within
1e-5.  TransE is not smooth (d|x|/dx = sign(x), TransE.py:51-53; the pairwise hinge, loss_functions.py:302-308, adds a second
discontinuity): a score that differs in its last bit flips a hinge term, an embedding that differs in its last bit flips a sign,
and two fp32 evaluations of one schedule in different summation orders part (tests/test_gpu_learning.py measures it).  As for
the ranks (oracle/rank_ordered.py) ONE order has to be fixed for "identical" to be testable -- the one the train kernels declare
(ampligraph_amd/csrc/kge_train_kernel.h, kge_train_tile.hip, kge_train_tiled.hip, kge_opt.h):

  * d = fl(fl(s + p) - o) per unit (TransE.py:51-53), for a corruption fl(fl(s + p) - e) (object replaced) or
    fl(fl(e + p) - o) (subject replaced), rounded where the reference rounds;
  * a score = -(sum of |d|): a lane of the wave adds the units it holds in order (which units: the kernel's row layout, see
    _lane_sums -- quads per lane in the owner-computes pair, single units per lane in the atomic-scatter path's narrow-row
    geometry), the 64 lane sums are combined by the wave64 DPP tree (rank_ordered.wave_sum); rows of up to 512 units;
  * the pairwise hinge in fp32: h_j = fl(fl(margin - P) + n_j), active iff h_j >= 0 (tf.maximum passes the gradient to its
    first argument on ties), per-positive loss = the wave64 tree over the lanes' max(h_j, 0) (lane j % 64 adds its terms in
    increasing j), reduction "sum";
  * with that loss every gradient entry is an INTEGER (a signed count of active hinge terms per unit: dL/dscore is -1 / +1,
    d score / d row is -/+ sign(d)), so the row sums are exact in fp32 in ANY order -- bucket order, atomics and the
    deterministic mode's sorted order all give the same bits;
  * Adam per element as kge_opt.h opt_elem writes it (Keras legacy rule, optimizers.py:136-168): m = fl(fl(m b1) + fl(g (1 - b1))),
    v = fl(fl(v b2) + fl(fl(g g) (1 - b2))), x = fl(x - fl(fl(lr_t m) / fl(sqrt(v) + eps))), lr_t formed in fp64 from the fp32
    hyper-parameters and rounded once, dense over both tables.

Only the fp64 sum of the per-positive losses is order-dependent (~1e-16 relative; nothing feeds back).  Pinned on the CPU
(tests/test_oracle_train_ordered.py): equal to kge_oracle.train_step wherever no decision is within rounding of its boundary
(dyadic tables: bit for bit), and the wave tree against an independent restatement.

The losses with transcendentals and the other four models (round 4, second half).  The default kernels evaluate exp / log / rcp /
sqrt with the hardware approximations (1-2 ulp, implementation-defined bits), which no CPU can reproduce; the DETERMINISTIC mode
(AMDKGE_TILED_DETERMINISTIC) uses declared forms built from IEEE operations only -- det_exp / det_log12 / det_sig_logsig below are
the same formulas in numpy -- and IEEE sqrtf / division, adds every gradient row's entries in a canonical sorted order and the
relation gradient in batch order.  Restated here for that mode, whole steps:
  * transe_step_det       TransE x {nll, self_adversarial, multiclass_nll} (rows of up to 256 units);
  * trilinear_step_det    DistMult / ComplEx / HolE x the same losses, every launch geometry of the forward kernel
                          (DistMult.py:48, ComplEx.py:58-62,93-107,138-150, HolE.py:45);
  * rotate_step_det       RotatE (RotatE.py:62-105), every launch geometry;
with the shared protocol of the single-pass forward kernel (_det_row_protocol: rows ordered by side, groups of PF rows, the
online softmax of the self-adversarial loss with its rescale), its closing arithmetic (_det_finish), the sorted tile sums
(_sorted_row_sums) and the batch-ordered relation gradient (_batch_order_row_sums).  fmaf32 restates the one-rounding fma (numpy
has none) and is pinned against libm's.  Pinned on the CPU against kge_oracle's fp64 loss and dense gradients to a few 1e-6; on the
GPU the deterministic fits are BIT-IDENTICAL to replay_learning for all five models (tests/test_gpu_learning.py,
test_gpu_deterministic.py, test_gpu_fullsize.py).
"""
import math

import numpy as np

from . import kge_oracle as O
from .philox import sample_corruption_draws
from .rank_ordered import wave_sum

F32 = np.float32


def _lane_sums(absd, layout="quad"):
    """[n, K] per-unit |d| -> [n, 64] lane sums of one wave, as the forward kernels lay a row out over the lanes:
      "quad": lane l holds the QUADS l, l + 64 (units 4 q .. 4 q + 3 each) -- the 16-byte geometry of the owner-computes pair (any
              k, stored halves are whole float4s) and of the atomic-scatter path for rows of 129 .. 512 units; a quad's units are
              added in order from 0, the lane's quads one after the other;
      "unit": lane l holds the UNITS l, l + 64, ... -- the one-unit-per-lane geometry the atomic-scatter path takes for rows of up
              to 128 stored units (kge_train.hip launch_train_m).
    K <= 512 (one wave per positive)."""
    n, K = absd.shape
    assert K <= 512, "ordered TransE step: rows of up to 512 units (one wave per positive)"
    lanes = np.zeros((n, 64), dtype=F32)
    if layout == "unit":
        for c0 in range(0, K, 64):
            blk = absd[:, c0:c0 + 64]
            lanes[:, :blk.shape[1]] = (lanes[:, :blk.shape[1]] + blk).astype(F32)   # (first chunk: 0 + |d|, exact)
        return lanes
    assert layout == "quad" and K % 4 == 0
    q = absd.reshape(n, K // 4, 4)
    acc = np.zeros((n, K // 4), dtype=F32)
    for u in range(4):
        acc = (acc + q[:, :, u]).astype(F32)
    for c0 in range(0, K // 4, 64):
        blk = acc[:, c0:c0 + 64]
        lanes[:, :blk.shape[1]] = (lanes[:, :blk.shape[1]] + blk).astype(F32)
    return lanes


def transe_scores(s, p, o, layout="quad"):
    """-(sum |fl(fl(s + p) - o)|) in the declared order; s, p, o fp32 [n, K].  Rows beyond 512 units (quad layout only): four
    waves per positive, their sums added in wave order (_reduce_quads)."""
    d = ((s + p).astype(F32) - o).astype(F32)
    if d.shape[1] > 512:
        assert layout == "quad"
        return (F32(-1.0) * _unit_chain(np.abs(d))).astype(F32), d
    return (F32(-1.0) * wave_sum(_lane_sums(np.abs(d), layout))).astype(F32), d


class OptState:
    """Both tables with their optimizer state tensors, fp32, updated by kge_opt.h's opt_elem rule for rule `kind` -- every rule is
    element-wise IEEE arithmetic (+, *, /, sqrt, max) in a fixed operation order, so numpy float32 reproduces it bit for bit.
    Hyper-parameters are the fp32 values the descriptor carries (OptimizerWrapper.to_ffi): lr, beta1 / beta2 (or the rule's rho /
    momentum in their place, as include/amdkge.h documents), epsilon."""

    def __init__(self, ent, rel, kind="adam", lr=1e-3, beta1=None, beta2=None, eps=1e-7):
        self.ent, self.rel = np.array(ent, dtype=F32), np.array(rel, dtype=F32)
        self.kind = kind
        d1 = {"adam": 0.9, "adamax": 0.9, "momentum": 0.0, "rmsprop": 0.9, "rmsprop_mom": 0.9, "adadelta": 0.95}.get(kind, 0.9)
        d2 = {"adam": 0.999, "adamax": 0.999}.get(kind, 0.0)
        self.lr, self.b1, self.b2, self.eps = F32(lr), F32(d1 if beta1 is None else beta1), F32(d2 if beta2 is None else beta2), F32(eps)
        ns = {"sgd": 0, "adagrad": 1, "momentum": 1, "rmsprop": 1}.get(kind, 2)
        fill = F32(0.1) if kind == "adagrad" else F32(0.0)   # Keras legacy Adagrad: initial_accumulator_value = 0.1
        self.s0 = [np.full_like(self.ent, fill), np.full_like(self.rel, fill)] if ns >= 1 else [None, None]
        self.s1 = [np.zeros_like(self.ent), np.zeros_like(self.rel)] if ns == 2 else [None, None]
        self.iterations = 0

    # (Adam's slots under the names the tests of the Adam-only first version use)
    @property
    def m(self):
        return self.s0

    @property
    def v(self):
        return self.s1

    def apply(self, Ge, Gr):
        """kge_opt.h: fill_opt_args (lr_t and 1 - beta formed in fp64 from the fp32 values, rounded once) + opt_elem<KIND>."""
        self.iterations += 1
        t = float(self.iterations)
        b1d, b2d, lrd = float(self.b1), float(self.b2), float(self.lr)
        omb1, omb2 = F32(1.0 - b1d), F32(1.0 - b2d)
        if self.kind == "adamax":
            lr_t = F32(lrd / (1.0 - math.pow(b1d, t)))
        else:
            lr_t = F32(lrd * math.sqrt(1.0 - math.pow(b2d, t)) / (1.0 - math.pow(b1d, t))) if self.kind == "adam" else F32(0)
        lr, b1, b2, eps = self.lr, self.b1, self.b2, self.eps
        f = lambda a: a.astype(F32)   # noqa: E731  (every operation rounds to fp32 once, as the kernel's does)
        for i, (x, g) in enumerate(((self.ent, Ge), (self.rel, Gr))):
            g = np.asarray(g).astype(F32)
            s0, s1 = self.s0[i], self.s1[i]
            k = self.kind
            if k == "adam":
                s0[...] = f(f(s0 * b1) + f(g * omb1))
                s1[...] = f(f(s1 * b2) + f(f(g * g) * omb2))
                x[...] = f(x - f(f(lr_t * s0) / f(f(np.sqrt(s1)) + eps)))
            elif k == "adagrad":
                s0[...] = f(s0 + f(g * g))
                x[...] = f(x - f(f(lr * g) / f(f(np.sqrt(s0)) + eps)))
            elif k == "momentum":     # beta1 = momentum, beta2 != 0: nesterov
                s0[...] = f(f(s0 * b1) - f(lr * g))
                x[...] = f(x + (f(f(s0 * b1) - f(lr * g)) if b2 != 0 else s0))
            elif k == "rmsprop":      # beta1 = rho
                s0[...] = f(s0 + f(f(f(g * g) - s0) * omb1))
                x[...] = f(x - f(f(lr * g) / f(f(np.sqrt(s0)) + eps)))
            elif k == "rmsprop_mom":  # beta1 = rho, beta2 = momentum
                s0[...] = f(s0 + f(f(f(g * g) - s0) * omb1))
                s1[...] = f(f(s1 * b2) + f(f(lr * g) / f(np.sqrt(f(s0 + eps)))))
                x[...] = f(x - s1)
            elif k == "adadelta":     # beta1 = rho
                s0[...] = f(f(s0 * b1) + f(f(g * g) * omb1))
                u = f(f(f(np.sqrt(f(s1 + eps))) * f(F32(1.0) / f(np.sqrt(f(s0 + eps))))) * g)
                x[...] = f(x - f(u * lr))
                s1[...] = f(f(s1 * b1) + f(f(u * u) * omb1))
            elif k == "adamax":
                s0[...] = f(s0 + f(f(g - s0) * omb1))
                s1[...] = np.maximum(f(b2 * s1), np.abs(g)).astype(F32)
                x[...] = f(x - f(f(lr_t * s0) / f(s1 + eps)))
            elif k == "sgd":
                x[...] = f(x - f(lr * g))
            else:
                raise ValueError(k)


def AdamState(ent, rel, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
    return OptState(ent, rel, "adam", lr, beta1, beta2, eps)


def transe_pairwise_step(state, pos, eta, seed, step, margin=1.0, n_ents=None, row_offset=0, b_global=None, return_grads=False,
                         loss="pairwise", layout="quad"):
    """One step of TransE / pairwise or absolute_margin (reduction "sum") on `pos` (int [B, 3]) in the declared order, then
    `state.apply`; corruptions from the shared Philox contract (oracle/philox.py, rows j * b_global + row_offset + i).  Updates
    `state` in place; returns the batch loss (fp64 sum of the fp32 per-positive losses).  layout: how the kernel that is being
    restated lays a row over the lanes (_lane_sums).
    absolute_margin (loss_functions.py:458-464): sum_j max(margin + n_j, 0) - eta P, i.e. dL/dP = -eta whatever is active."""
    assert loss in ("pairwise", "absolute_margin")
    pos = np.asarray(pos, dtype=np.int64)
    B = pos.shape[0]
    ent, rel = state.ent, state.rel
    N = ent.shape[0] if n_ents is None else int(n_ents)
    bg = B if b_global is None else int(b_global)
    margin = F32(margin)
    s, p, o = ent[pos[:, 0]], rel[pos[:, 1]], ent[pos[:, 2]]
    P, d_pos = transe_scores(s, p, o, layout)
    Ge = np.zeros(ent.shape, dtype=np.float64)   # integers throughout: exact in fp32 as in fp64, in any order
    Gr = np.zeros(rel.shape, dtype=np.float64)
    n_act = np.zeros(B, dtype=np.int64)
    h_lanes = np.zeros((B, 64), dtype=F32)   # lane j % 64 adds max(h_j, 0) for its j in increasing order
    sp = (s + p).astype(F32)
    mP = (margin - P).astype(F32)
    for j in range(eta):
        rows = np.uint64(j) * np.uint64(bg) + np.uint64(row_offset) + np.arange(B, dtype=np.uint64)
        keep, repl = sample_corruption_draws(rows, step, seed, N)
        e = ent[repl]
        keep = keep.astype(bool)
        # object replaced: fl(fl(s + p) - e); subject replaced: fl(fl(e + p) - o)
        d = np.where(keep[:, None], (sp - e).astype(F32), ((e + p).astype(F32) - o).astype(F32))
        n_j = ((F32(-1.0) * _unit_chain(np.abs(d))) if d.shape[1] > 512 else (F32(-1.0) * wave_sum(_lane_sums(np.abs(d), layout)))).astype(F32)
        h = (mP + n_j).astype(F32) if loss == "pairwise" else (margin + n_j).astype(F32)
        act = h >= 0
        h_lanes[:, j % 64] = (h_lanes[:, j % 64] + np.maximum(h, F32(0))).astype(F32)
        n_act += act
        # dL/dn_j = +1 for an active term; d n_j / d(row) = -/+ sign(d): replaced row gets +sign(d) (object) or -sign(d) (subject)
        sg = np.sign(d).astype(np.float64) * act[:, None]
        np.add.at(Ge, repl[keep], sg[keep])            # (s, p, e): d/de = +sign(d)
        np.add.at(Ge, pos[keep, 0], -sg[keep])         #            d/ds = -sign(d)
        np.add.at(Ge, repl[~keep], -sg[~keep])         # (e, p, o): d/de = -sign(d)
        np.add.at(Ge, pos[~keep, 2], sg[~keep])        #            d/do = +sign(d)
        np.add.at(Gr, pos[:, 1], -sg)                  # d/dp = -sign(d) on either side
    # positive: dL/dP = -(number of active terms); d P / d(s, p, o) = (-, -, +) sign(d)
    if loss == "absolute_margin":
        n_act = np.full(B, eta, dtype=np.int64)
    sgp = np.sign(d_pos).astype(np.float64) * n_act[:, None].astype(np.float64)
    np.add.at(Ge, pos[:, 0], sgp)
    np.add.at(Gr, pos[:, 1], sgp)
    np.add.at(Ge, pos[:, 2], -sgp)
    per = wave_sum(h_lanes)
    if loss == "absolute_margin":   # per = (wave_sum(acc) - feta * P) / red, red = 1 (kge_loss.h loss_call over WaveWalk)
        per = (per - (F32(eta) * P).astype(F32)).astype(F32)
    assert np.abs(Ge).max() < 2 ** 24 and np.abs(Gr).max() < 2 ** 24
    if return_grads:   # (tests: the step's ingredients, nothing applied)
        return float(per.astype(np.float64).sum()), Ge, Gr
    state.apply(Ge, Gr)
    return float(per.astype(np.float64).sum())


def replay_learning(model, loss, seed, cfg, planted_kg, initialise, epochs=None, opt="adam", opt_hp=None, layout="quad"):
    """The schedule of tests/test_gpu_learning.py (planted graph, Glorot tables as the drop-in class draws them, sequential
    batches) through transe_pairwise_step / transe_step_det / trilinear_step_det -> (loss history, state, id triples of train / test).  opt / opt_hp: the update rule
    (kge_opt.h kind name) and its (beta1, beta2) descriptor fields."""
    assert model in ("TransE", "DistMult", "ComplEx", "HolE", "RotatE") and loss in ("pairwise", "absolute_margin", "nll", "self_adversarial", "multiclass_nll")
    assert model == "TransE" or loss in ("nll", "self_adversarial", "multiclass_nll")
    d = planted_kg(model, seed=seed)
    train, test = d["train"].astype(str), d["test"].astype(str)
    ents, rels = O.first_seen_index(train)
    Xi = O.to_indexes(train, ents, rels)
    N, R, K = len(ents), len(rels), O.internal_k(model, cfg["k"])
    rng = np.random.Generator(np.random.PCG64(seed))
    st = OptState(initialise("glorot_uniform", (N, K), rng), initialise("glorot_uniform", (R, K), rng), opt, cfg["lr"], *(opt_hp or (None, None)))
    steps = (len(Xi) + cfg["batch"] - 1) // cfg["batch"]
    hist = []
    for ep in range(cfg["epochs"] if epochs is None else epochs):
        tot = 0.0
        for b in range(steps):
            xb = Xi[b * cfg["batch"]:(b + 1) * cfg["batch"]]
            if model == "RotatE":                                       # (deterministic mode only)
                tot += rotate_step_det(st, xb, cfg["eta"], seed, ep * steps + b, loss, max_rel_size=R)
            elif model != "TransE":                                     # (deterministic mode only)
                tot += trilinear_step_det(model, st, xb, cfg["eta"], seed, ep * steps + b, loss)
            elif loss in ("nll", "self_adversarial", "multiclass_nll"):   # (deterministic mode only: the owner-computes pair, quad layout)
                tot += transe_step_det(st, xb, cfg["eta"], seed, ep * steps + b, loss)
            else:
                tot += transe_pairwise_step(st, xb, cfg["eta"], seed, ep * steps + b, loss=loss, layout=layout)
        hist.append(tot / steps)
    return np.asarray(hist), st, Xi, O.to_indexes(test, ents, rels)


# ---------------------------------------------------------------------------------------------------------------------------------
# TransE / nll in DETERMINISTIC mode (AMDKGE_TILED_DETERMINISTIC): real-valued coefficients, so the order of every fp32 addition
# into a gradient row matters -- the mode's canonical order is restated: the loss terms from the DECLARED transcendentals
# (kge_train_kernel.h det_exp / det_log12: IEEE operations only), the single-pass forward kernel's per-side sums in corruption
# order, the tile pass adding a row's entries sorted by (positive, role, bits of g), the relation gradient in batch order.
# ---------------------------------------------------------------------------------------------------------------------------------
def _f(a):
    return np.asarray(a).astype(F32)


def det_exp(x):
    x = np.clip(_f(x), F32(-80.0), F32(80.0))
    n = np.rint(_f(x * F32(1.4426950216293335)))
    r = _f(_f(x - _f(n * F32(0.693359375))) - _f(n * F32(-2.12194440e-4)))
    p = np.full_like(r, F32(1.0) / F32(5040.0))
    for c in (F32(1.0) / F32(720.0), F32(1.0) / F32(120.0), F32(1.0) / F32(24.0), F32(1.0) / F32(6.0), F32(0.5), F32(1.0), F32(1.0)):
        p = _f(_f(p * r) + c)
    return np.ldexp(p, n.astype(np.int32)).astype(F32)


def det_log12(u):
    u = _f(u)
    z = _f(_f(u - F32(1.0)) / _f(u + F32(1.0)))
    w = _f(z * z)
    p = np.full_like(z, F32(1.0) / F32(15.0))
    for c in (F32(1.0) / F32(13.0), F32(1.0) / F32(11.0), F32(1.0) / F32(9.0), F32(1.0) / F32(7.0), F32(1.0) / F32(5.0), F32(1.0) / F32(3.0), F32(1.0)):
        p = _f(_f(p * w) + c)
    return _f(_f(F32(2.0) * z) * p)


def det_sig_logsig(y):
    """(sigma(y), log sigma(-y)) as kge_train_kernel.h det_sig_logsig."""
    y = _f(y)
    t = det_exp(-np.abs(y))
    u = _f(F32(1.0) + t)
    sig = np.where(y >= 0, _f(F32(1.0) / u), _f(t / u)).astype(F32)
    ls = _f(np.minimum(-y, F32(0.0)) - _f(det_log12(u) + _f(_f(t - _f(u - F32(1.0))) / u)))
    return sig, ls


def transe_step_det(state, pos, eta, seed, step, loss="nll", margin=None, alpha=0.5, n_ents=None, return_grads=False):
    """One step of TransE with a transcendental loss -- "nll", "self_adversarial" or "multiclass_nll", reduction "sum" -- as the
    owner-computes pair carries it out in DETERMINISTIC mode (rows of up to 256 units: one wave per positive, one quad per lane).
    The single-pass forward kernel's protocol is restated group by group (kge_train_kernel.h onepass_coeff / onepass_kappa /
    onepass_finish): corruptions ordered by side (object-replaced first), scored PF = 6 at a time, lane f of a group holding row f's
    loss terms and its share of the running statistics; self_adversarial's online softmax (running maximum, rescale of everything
    accumulated so far when it grows).  Updates `state`; returns the batch loss."""
    assert loss in ("nll", "self_adversarial", "multiclass_nll")
    PF = 6
    pos = np.asarray(pos, dtype=np.int64)
    B = pos.shape[0]
    ent, rel = state.ent, state.rel
    K = ent.shape[1]
    assert K % 4 == 0 and K <= 256
    N = ent.shape[0] if n_ents is None else int(n_ents)
    gamma = F32(3.0 if margin is None else margin)   # self_adversarial's margin (loss_functions.py:26)
    alpha = F32(alpha)
    feta = F32(float(eta))
    s, p, o = ent[pos[:, 0]], rel[pos[:, 1]], ent[pos[:, 2]]
    P, d_pos = transe_scores(s, p, o, "quad")
    sp = _f(s + p)
    keep = np.zeros((B, eta), dtype=bool)
    repl = np.zeros((B, eta), dtype=np.int64)
    sgn = np.zeros((B, eta, K), dtype=F32)
    nsc = np.zeros((B, eta), dtype=F32)
    for j in range(eta):
        rows = np.uint64(j) * np.uint64(B) + np.arange(B, dtype=np.uint64)
        kj, rj = sample_corruption_draws(rows, step, seed, N)
        keep[:, j], repl[:, j] = kj.astype(bool), rj
        e = ent[rj]
        d = np.where(keep[:, j][:, None], _f(sp - e), _f(_f(e + p) - o))
        sgn[:, j] = np.sign(d)
        nsc[:, j] = _f(F32(-1.0) * wave_sum(_lane_sums(np.abs(d), "quad")))
    ar = np.arange(B)
    order = np.argsort(~keep, axis=1, kind="stable")            # object-replaced (keep) first, j ascending within a side
    nkeep = keep.sum(1)
    av1 = np.zeros((2, B, K), dtype=F32)
    av2 = np.zeros((2, B, K), dtype=F32)
    two = loss == "self_adversarial"

    def add_rows(side, m_, jcol, c1, c2):                        # a row joins its side's sums: c sign(d)
        sg_f = sgn[ar, jcol]
        av1[side][m_] = _f(av1[side][m_] + _f(c1[:, None] * sg_f)[m_])
        if two:
            av2[side][m_] = _f(av2[side][m_] + _f(c2[:, None] * sg_f)[m_])

    def rescale(g_, rs):
        for dd in (0, 1):
            av1[dd] = np.where(g_[:, None], _f(av1[dd] * rs[:, None]), av1[dd])
            av2[dd] = np.where(g_[:, None], _f(av2[dd] * rs[:, None]), av2[dd])

    S, Lw, Zs, m_run = _det_row_protocol(loss, nsc, order, nkeep, eta, alpha, gamma, PF, add_rows, rescale)
    k1, k2, dP, sn, per = _det_finish(loss, P, nsc, S, Lw, Zs, m_run, alpha, gamma, feta)
    k1, k2 = _f(k1 * F32(-1.0)), _f(k2 * F32(-1.0))
    Go = _f(_f(k1[:, None] * av1[0]) + _f(k2[:, None] * av2[0]))
    Gs = _f(_f(k1[:, None] * av1[1]) + _f(k2[:, None] * av2[1]))
    gpos = _f(dP * F32(-1.0))
    sgv = _f(np.sign(d_pos) * gpos[:, None])
    gs = _f(sgv + Go)
    gp = _f(sgv + _f(Go + Gs))
    go = _f(_f(-sgv) - Gs)
    # ---- tile pass, deterministic: a row's entries sorted by (positive, role, bits of g), added from 0 in that order ----
    ent_dest, ent_pos, ent_role, ent_g, ent_vec = [], [], [], [], []
    for j in range(eta):
        g_e = _f(sn[:, j] * F32(-1.0))                          # entry g = dL/dn_j * sgn_scale
        live = ~(np.abs(g_e) < F32(np.finfo(np.float32).tiny))   # (an entry whose coefficient is below the smallest normal fp32 number is no entry; NaN is one)
        role = np.where(keep[:, j], 0, 1)
        gs_d = _f(g_e[:, None] * sgn[:, j])                     # g sign(d)
        vec = np.where(keep[:, j][:, None], _f(-gs_d), gs_d).astype(F32)   # role 0: dd = -(g sign d); role 1: ds = g sign d
        ent_dest.append(repl[live, j]); ent_pos.append(ar[live]); ent_role.append(role[live]); ent_g.append(g_e[live]); ent_vec.append(vec[live])
    one = np.ones(B, dtype=F32)
    ent_dest += [pos[:, 0], pos[:, 2]]; ent_pos += [ar, ar]; ent_role += [np.full(B, 2), np.full(B, 3)]; ent_g += [one, one]; ent_vec += [gs, go]
    Ge = _sorted_row_sums(ent.shape, ent_dest, ent_pos, ent_role, ent_g, ent_vec)
    # ---- relation gradient: the positives' staged rows added per relation in batch order ----
    Gr = _batch_order_row_sums(rel.shape, pos[:, 1], gp)
    total = float(per.astype(np.float64).sum())
    if return_grads:
        return total, Ge, Gr
    state.apply(Ge, Gr)
    return total


def _det_row_protocol(loss, nsc, order, nkeep, eta, alpha, gamma, PF, add_rows, rescale):
    """The single-pass forward kernel's row loop (kge_train_kernel.h onepass_coeff): per positive and side, groups of PF rows,
    lane f of a group evaluating row f's loss terms and holding its share of the running statistics; self_adversarial's online
    softmax.  `add_rows(side, mask, j, c1, c2)` lets the rows join the side's sums in order, `rescale(mask, rs)` rescales what
    has been accumulated when the running maximum grew.  Returns the wave sums (S, Lw, Zs) and the final running maximum."""
    B = nsc.shape[0]
    ar = np.arange(B)
    S_l = np.zeros((B, 64), dtype=F32)      # per-lane partial sums of the running statistics
    Lw_l = np.zeros((B, 64), dtype=F32)
    Zs_l = np.zeros((B, 64), dtype=F32)
    m_run = np.full(B, -np.inf, dtype=F32)  # self_adversarial: running maximum of alpha * n (wave-uniform)
    for side in (0, 1):
        cnt = nkeep if side == 0 else eta - nkeep
        start = np.zeros(B, dtype=np.int64) if side == 0 else nkeep
        for g0 in range(0, eta, PF):
            act = g0 < cnt                                       # positives that have this group at all
            if not act.any():
                continue
            jf = np.zeros((B, PF), dtype=np.int64)
            ok = np.zeros((B, PF), dtype=bool)
            for f in range(PF):
                ok[:, f] = (g0 + f < cnt)
                jf[:, f] = order[ar, np.minimum(start + g0 + f, eta - 1)]
            nv = nsc[ar[:, None], jf]                            # (B, PF) scores of the group's rows (garbage where not ok)
            c1 = np.zeros((B, PF), dtype=F32)
            c2 = np.zeros((B, PF), dtype=F32)
            if loss == "nll":
                inr = ok & (nv >= F32(-75.0)) & (nv <= F32(75.0))
                sg, lsn = det_sig_logsig(np.clip(nv, F32(-75.0), F32(75.0)))
                Lw_l[:, :PF] = np.where(ok, _f(Lw_l[:, :PF] + _f(-lsn)), Lw_l[:, :PF])
                c1 = np.where(inr, sg, F32(0.0)).astype(F32)
            elif loss == "multiclass_nll":
                inr = ok & (nv >= F32(-75.0)) & (nv <= F32(75.0))
                ex = np.where(ok, det_exp(np.clip(nv, F32(-75.0), F32(75.0))), F32(0.0)).astype(F32)
                Zs_l[:, :PF] = _f(Zs_l[:, :PF] + ex)             # (adds 0 for rows that do not exist)
                c1 = np.where(inr, ex, F32(0.0)).astype(F32)
            else:
                x = _f(alpha * nv)
                gm = np.max(np.where(ok, x, F32(-np.inf)), axis=1).astype(F32)
                grow = act & (gm > m_run)
                with np.errstate(invalid="ignore"):
                    resc = np.where(np.isinf(m_run), F32(0.0), det_exp(np.where(grow, _f(m_run - gm), F32(0.0)))).astype(F32)
                rs = np.where(grow, resc, F32(1.0)).astype(F32)
                S_l = np.where(grow[:, None], _f(S_l * rs[:, None]), S_l)
                Lw_l = np.where(grow[:, None], _f(Lw_l * rs[:, None]), Lw_l)
                m_run = np.where(grow, gm, m_run).astype(F32)
                u = np.where(ok, det_exp(_f(x - m_run[:, None])), F32(0.0)).astype(F32)
                sg, ell = det_sig_logsig(_f(nv + gamma))
                S_l[:, :PF] = np.where(act[:, None], _f(S_l[:, :PF] + u), S_l[:, :PF])
                Lw_l[:, :PF] = np.where(ok, _f(Lw_l[:, :PF] + _f(u * ell)), Lw_l[:, :PF])
                c1 = np.where(ok, _f(u * _f(sg - _f(alpha * ell))), F32(0.0)).astype(F32)
                c2 = u
                # the running maximum grew: everything accumulated so far is rescaled (all four accumulators of both sides)
                rescale(grow & (rs != 1), rs)
            for f in range(PF):                                   # the rows join the side's sums in order
                m_ = ok[:, f]
                if m_.any():
                    add_rows(side, m_, jf[:, f], c1[:, f], c2[:, f])
    return wave_sum(S_l), wave_sum(Lw_l), wave_sum(Zs_l), m_run


def _det_finish(loss, P, nsc, S, Lw, Zs, m_run, alpha, gamma, feta):
    """kge_train_kernel.h onepass_kappa / onepass_finish with the declared transcendentals: (k1, k2) of E_side = k1 av1 + k2 av2
    (before the score scale), the positive's dL/dP, every corruption's dL/dn_j and the per-positive loss."""
    B = P.shape[0]
    Pc = np.clip(P, F32(-75.0), F32(75.0))
    inP = (P >= F32(-75.0)) & (P <= F32(75.0))
    inr_all = (nsc >= F32(-75.0)) & (nsc <= F32(75.0))
    if loss == "nll":
        k1, k2 = np.full(B, F32(1.0)), np.zeros(B, dtype=F32)
        sgP, lsP = det_sig_logsig(-Pc)
        dP = np.where(inP, _f(_f(-feta * sgP) / F32(1.0)), F32(0.0)).astype(F32)
        sg_all, _ = det_sig_logsig(np.clip(nsc, F32(-75.0), F32(75.0)))
        sn = np.where(inr_all, _f(sg_all / F32(1.0)), F32(0.0)).astype(F32)
        per = _f(_f(_f(feta * _f(-lsP)) + Lw) / F32(1.0))
    elif loss == "multiclass_nll":
        eP = det_exp(Pc)
        Z = _f(_f(Zs / F32(1.0)) + eP)
        k1, k2 = _f(F32(1.0) / _f(Z * F32(1.0))), np.zeros(B, dtype=F32)
        dP = np.where(inP, _f(F32(-1.0) + _f(eP / Z)), F32(0.0)).astype(F32)
        sn = np.where(inr_all, _f(_f(det_exp(np.clip(nsc, F32(-75.0), F32(75.0))) / Z[:, None]) / F32(1.0)), F32(0.0)).astype(F32)
        per = _f(np.log(Z.astype(np.float64)).astype(F32) - Pc)   # (libm logf on the device: the loss VALUE only, nothing feeds back)
    else:
        k1 = _f(F32(1.0) / _f(S * F32(1.0)))
        k2 = _f(_f(alpha * _f(Lw / S)) / _f(S * F32(1.0)))
        lbar = _f(Lw / S)
        w = _f(det_exp(_f(_f(alpha * nsc) - m_run[:, None])) / S[:, None])
        sg_all, ell_all = det_sig_logsig(_f(nsc + gamma))
        sn = _f(_f(_f(w * sg_all) - _f(_f(alpha * w) * _f(ell_all - lbar[:, None]))) / F32(1.0))
        sgP, lsP = det_sig_logsig(_f(-_f(gamma + P)))
        dP = _f(-sgP)
        per = _f(_f(-lsP) - _f(lbar / F32(1.0)))
    return k1, k2, dP, sn, per


def _sorted_row_sums(shape, ent_dest, ent_pos, ent_role, ent_g, ent_vec):
    """The deterministic tile pass: a row's entries sorted by (positive, role, bits of g) and added from 0 in that order."""
    dest = np.concatenate(ent_dest); epos = np.concatenate(ent_pos); role = np.concatenate(ent_role)
    gbits = np.concatenate(ent_g).astype(F32).view(np.uint32).astype(np.int64)
    vec = np.concatenate(ent_vec).astype(F32)
    srt = np.lexsort((gbits, role, epos, dest))
    dest, vec = dest[srt], vec[srt]
    G = np.zeros(shape, dtype=F32)
    if not len(dest):
        return G
    first = np.r_[True, dest[1:] != dest[:-1]]
    start_of = np.maximum.accumulate(np.where(first, np.arange(len(dest)), 0))
    rank_in_row = np.arange(len(dest)) - start_of
    for r in range(int(rank_in_row.max()) + 1):
        m = rank_in_row == r
        G[dest[m]] = _f(G[dest[m]] + vec[m])
    return G


def _batch_order_row_sums(shape, rows, vecs):
    """rel_backward_det_kernel: the positives' staged relation-gradient rows added per relation in batch order."""
    G = np.zeros(shape, dtype=F32)
    B = len(rows)
    if not B:
        return G
    srt_r = np.argsort(rows, kind="stable")
    rs_, gpv = rows[srt_r], vecs[srt_r]
    first = np.r_[True, rs_[1:] != rs_[:-1]]
    start_of = np.maximum.accumulate(np.where(first, np.arange(B), 0))
    rk = np.arange(B) - start_of
    for r in range(int(rk.max()) + 1):
        m = rk == r
        G[rs_[m]] = _f(G[rs_[m]] + gpv[m])
    return G


def fmaf32(a, b, c):
    """fl32(a * b + c) with ONE rounding, element-wise on fp32 arrays (numpy has no fma).  a * b is exact in fp64 (48-bit product);
    the fp64 sum is turned into its round-to-odd value with the exact residual of the addition (TwoSum), and a round-to-odd
    53-bit value rounds to the nearest fp32 exactly as the unrounded sum does (53 >= 2 * 24 + 2).  Pinned against libm's fmaf
    (tests/test_oracle_train_ordered.py)."""
    a, b, c = np.broadcast_arrays(_f(a).astype(np.float64), _f(b).astype(np.float64), _f(c).astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    si = np.ascontiguousarray(s).view(np.int64).copy()
    fin = np.isfinite(s) & np.isfinite(err)
    odd_fix = fin & (err != 0) & ((si & 1) == 0)
    up = (err > 0) == (s > 0)                       # the exact sum lies beyond s in magnitude
    si = np.where(odd_fix, np.where(up, si + 1, si - 1), si)
    return si.view(np.float64).astype(F32)


def _pf_of(model, nq):
    """Rows in flight per group of the forward kernel (kge_train_kernel.h: PF) for a row of nq quads per component: the launch
    geometry is one wave per positive with 1 (nq <= 64) or 2 (<= 128) quads per component and lane, or four waves per positive
    with 1 (<= 256) or 2 quads (kge_train_stage.hip forward_by_width)."""
    ch = 1 if nq <= 64 else (2 if nq <= 128 else (1 if nq <= 256 else 2))
    nc = 1 if model in ("DistMult", "TransE") else 2
    return (3 if model == "RotatE" else 6) if ch * nc * 4 <= 8 else 2


def _reduce_quads(tq):
    """[n, nq] per-QUAD partial sums -> [n] row sums in the forward kernel's declared order.  Up to 128 quads: ONE wave, lane l
    holds quads l and l + 64 (added from 0 in that order), the wave64 DPP tree.  More (four waves per positive, 256 threads):
    thread t holds quads t and t + 256, every wave reduces its 64 threads by the tree, the four wave sums are added in wave
    order from 0 (they meet in LDS)."""
    tq = _f(tq)
    n, nq = tq.shape
    assert nq <= 512
    width = 64 if nq <= 128 else 256
    thr = np.zeros((n, width), dtype=F32)
    for c0 in range(0, nq, width):
        blk = tq[:, c0:c0 + width]
        thr[:, :blk.shape[1]] = _f(thr[:, :blk.shape[1]] + blk)
    if width == 64:
        return wave_sum(thr)
    tot = np.zeros(n, dtype=F32)
    for w in range(4):
        tot = _f(tot + wave_sum(thr[:, 64 * w:64 * w + 64]))
    return tot


def _unit_chain(vals):
    """[n, k] per-unit values -> [n] row sums: a quad's four units added in order from 0, then _reduce_quads."""
    vals = _f(vals)
    n, k = vals.shape
    q = vals.reshape(n, k // 4, 4)
    acc = np.zeros((n, k // 4), dtype=F32)
    for u in range(4):
        acc = _f(acc + q[:, :, u])
    return _reduce_quads(acc)


def trilinear_step_det(model, state, pos, eta, seed, step, loss="self_adversarial", margin=None, alpha=0.5, n_ents=None,
                       return_grads=False):
    """One step of DistMult / ComplEx / HolE with "nll", "self_adversarial" or "multiclass_nll" (reduction "sum") as the
    owner-computes pair carries it out in DETERMINISTIC mode, in every launch geometry of the forward kernel (one wave per
    positive with one or two quads per component and lane, four waves per positive for stored k > 512: _reduce_quads, _pf_of).
    What differs from transe_step_det is the model arithmetic (kge_train_kernel.h, ONEPASS branch; kge_device.h
    score_unit / grad_unit -- plain products and sums, each rounded where it is written, -ffp-contract=off):
      * the positive's score: score_unit per unit (DistMult.py:48, ComplEx.py:58-62), a quad's units added in order, wave tree;
      * a corruption's score as a dot product with the side row A = d/do (s, p) or B = d/ds (p, o) (the query-vector form of
        ComplEx.py:93-107,138-150): per lane ONE fmaf chain over (unit, component), then the wave tree;
      * sum_j c_j e_j per side by fmaf(c_j, e_j, acc) in the side-ordered row sequence, rescaled when the running softmax
        maximum grows; E_side = fl(fl(k1 av1) + fl(k2 av2)); the row gradients follow from grad_unit on (s, p, E_obj) and
        (E_subj, p, o);
      * tile pass: an entry adds fl(g A) or fl(g B) (own rows: 1 * staged gradient), a row's entries in sorted order.
    State rows are the STORED rows: [re | im] halves for the complex models."""
    assert model in ("DistMult", "ComplEx", "HolE") and loss in ("nll", "self_adversarial", "multiclass_nll")
    pos = np.asarray(pos, dtype=np.int64)
    B = pos.shape[0]
    ent, rel = state.ent, state.rel
    K = ent.shape[1]
    NC = 1 if model == "DistMult" else 2
    k = K // NC
    assert k % 4 == 0 and k <= 2048
    PF = _pf_of(model, k // 4)
    N = ent.shape[0] if n_ents is None else int(n_ents)
    gamma = F32(3.0 if margin is None else margin)
    alpha = F32(alpha)
    feta = F32(float(eta))
    sgn_scale = F32(1.0)
    if model == "HolE":
        sgn_scale = F32(2.0 / float(getattr(state, "k_live", k)))   # (float)(2.0 / k), kge_host.h model_const (HolE.py:45)
    comp = (lambda t: [t[:, h * k:(h + 1) * k] for h in range(NC)])
    s, p, o = comp(ent[pos[:, 0]]), comp(rel[pos[:, 1]]), comp(ent[pos[:, 2]])

    def grad_unit(s_, p_, o_, g):
        """kge_device.h grad_unit: g d(score)/d(s, p, o) per unit; g [n] or [n, 1]-broadcastable."""
        g = _f(g)
        if g.ndim == 1:
            g = g[:, None]
        if NC == 1:
            return ([_f(g * _f(p_[0] * o_[0]))], [_f(g * _f(s_[0] * o_[0]))], [_f(g * _f(s_[0] * p_[0]))])
        ds = [_f(g * _f(_f(p_[0] * o_[0]) + _f(p_[1] * o_[1]))), _f(g * _f(_f(p_[0] * o_[1]) - _f(p_[1] * o_[0])))]
        dp = [_f(g * _f(_f(s_[0] * o_[0]) + _f(s_[1] * o_[1]))), _f(g * _f(_f(s_[0] * o_[1]) - _f(s_[1] * o_[0])))]
        dd = [_f(g * _f(_f(s_[0] * p_[0]) - _f(s_[1] * p_[1]))), _f(g * _f(_f(s_[0] * p_[1]) + _f(s_[1] * p_[0])))]
        return ds, dp, dd

    one = np.ones(B, dtype=F32)
    dsA, _, ddA = grad_unit(s, p, o, one)
    A, Bq = ddA, dsA                                             # A = d/do (s, p), B = d/ds (p, o)
    if NC == 1:
        su = _f(_f(s[0] * p[0]) * o[0])
    else:
        su = _f(_f(s[0] * _f(_f(p[0] * o[0]) + _f(p[1] * o[1]))) + _f(s[1] * _f(_f(p[0] * o[1]) - _f(p[1] * o[0]))))
    P = _f(sgn_scale * _unit_chain(su))

    def row_score(q, e):
        """per quad: t = fmaf(q[u][h], e[u][h], t) over u = 0..3, h = 0..NC-1 from 0; quads by _reduce_quads."""
        n = q[0].shape[0]
        t = np.zeros((n, k // 4), dtype=F32)
        for u in range(4):
            for h in range(NC):
                t = fmaf32(q[h][:, u::4], e[h][:, u::4], t)
        return _f(sgn_scale * _reduce_quads(t))

    keep = np.zeros((B, eta), dtype=bool)
    repl = np.zeros((B, eta), dtype=np.int64)
    nsc = np.zeros((B, eta), dtype=F32)
    for j in range(eta):
        rows = np.uint64(j) * np.uint64(B) + np.arange(B, dtype=np.uint64)
        kj, rj = sample_corruption_draws(rows, step, seed, N)
        keep[:, j], repl[:, j] = kj.astype(bool), rj
        e = comp(ent[rj])
        nsc[:, j] = np.where(keep[:, j], row_score(A, e), row_score(Bq, e))
    ar = np.arange(B)
    order = np.argsort(~keep, axis=1, kind="stable")
    nkeep = keep.sum(1)
    av1 = np.zeros((2, B, K), dtype=F32)
    av2 = np.zeros((2, B, K), dtype=F32)
    two = loss == "self_adversarial"

    def add_rows(side, m_, jcol, c1, c2):
        e = ent[repl[ar, jcol]]
        av1[side][m_] = fmaf32(c1[:, None], e, av1[side])[m_]
        if two:
            av2[side][m_] = fmaf32(c2[:, None], e, av2[side])[m_]

    def rescale(g_, rs):
        for dd in (0, 1):
            av1[dd] = np.where(g_[:, None], _f(av1[dd] * rs[:, None]), av1[dd])
            av2[dd] = np.where(g_[:, None], _f(av2[dd] * rs[:, None]), av2[dd])

    S, Lw, Zs, m_run = _det_row_protocol(loss, nsc, order, nkeep, eta, alpha, gamma, PF, add_rows, rescale)
    k1, k2, dP, sn, per = _det_finish(loss, P, nsc, S, Lw, Zs, m_run, alpha, gamma, feta)
    k1, k2 = _f(k1 * sgn_scale), _f(k2 * sgn_scale)
    Eo = comp(_f(_f(k1[:, None] * av1[0]) + _f(k2[:, None] * av2[0])))
    Es = comp(_f(_f(k1[:, None] * av1[1]) + _f(k2[:, None] * av2[1])))
    gs, gp, go = grad_unit(s, p, o, _f(dP * sgn_scale))
    ds1, dp1, _ = grad_unit(s, p, Eo, one)                        # corruptions (s, p, e_j)
    gs = [_f(gs[h] + ds1[h]) for h in range(NC)]
    gp = [_f(gp[h] + dp1[h]) for h in range(NC)]
    _, dp2, dd2 = grad_unit(Es, p, o, one)                        # corruptions (e_j, p, o)
    go = [_f(go[h] + dd2[h]) for h in range(NC)]
    gp = [_f(gp[h] + dp2[h]) for h in range(NC)]
    gs, gp, go = np.concatenate(gs, 1), np.concatenate(gp, 1), np.concatenate(go, 1)
    Arow, Brow = np.concatenate(A, 1), np.concatenate(Bq, 1)
    ent_dest, ent_pos, ent_role, ent_g, ent_vec = [], [], [], [], []
    for j in range(eta):
        g_e = _f(sn[:, j] * sgn_scale)
        live = ~(np.abs(g_e) < F32(np.finfo(np.float32).tiny))   # (an entry whose coefficient is below the smallest normal fp32 number is no entry; NaN is one)
        role = np.where(keep[:, j], 0, 1)
        vec = _f(g_e[:, None] * np.where(keep[:, j][:, None], Arow, Brow))
        ent_dest.append(repl[live, j]); ent_pos.append(ar[live]); ent_role.append(role[live]); ent_g.append(g_e[live]); ent_vec.append(vec[live])
    ent_dest += [pos[:, 0], pos[:, 2]]; ent_pos += [ar, ar]; ent_role += [np.full(B, 2), np.full(B, 3)]; ent_g += [one, one]; ent_vec += [gs, go]
    Ge = _sorted_row_sums(ent.shape, ent_dest, ent_pos, ent_role, ent_g, ent_vec)
    Gr = _batch_order_row_sums(rel.shape, pos[:, 1], gp)
    total = float(per.astype(np.float64).sum())
    if return_grads:
        return total, Ge, Gr
    state.apply(Ge, Gr)
    return total


def rotate_step_det(state, pos, eta, seed, step, loss="self_adversarial", margin=None, alpha=0.5, n_ents=None, max_rel_size=None,
                    return_grads=False, debug=None):
    """One step of RotatE (RotatE.py:62-105) with "nll", "self_adversarial" or "multiclass_nll" as the owner-computes pair carries
    it out in DETERMINISTIC mode (stored k a multiple of 4, i.e. no padding units; every launch geometry: _reduce_quads, _pf_of):
      * the relation as (cos, sin) of the fp32 phase theta / fl32(embedding_range / pi), each correctly rounded (fp64 libm,
        rounded once: rel_phase_kernel / prep_rel_exact);
      * z = s o r - o with the reference's operations on both sides (object side: A - e with A = s o r; subject side:
        e o r - o), |z| = sqrtf(fl(fl(zr zr) + fl(zi zi))) (IEEE square root), a lane adds its quad's moduli in order, wave tree,
        score = -sum;
      * per corruption the UNIT VECTOR z / |z| (one IEEE division 1 / |z|, two products), sum_j c_j z_j/|z_j| per side by fmaf in
        corruption order, groups of THREE rows (two with two quads per lane), online-softmax rescale;
      * row gradients: d/ds = conj(r) o Z_obj, d/do = -Z_subj, d/dphase = Im(conj(A) Z_obj) + Im(conj(o) Z_subj), on top of
        grad_unit's gradient of the positive; d/dtheta = d/dphase * fl(1 / phase_div);
      * tile pass: an entry adds g (e - S) / |e - S| with S the staged side row (A, or B = o o conj(r)) and e the owner's live row."""
    assert loss in ("nll", "self_adversarial", "multiclass_nll")
    pos = np.asarray(pos, dtype=np.int64)
    B = pos.shape[0]
    ent, rel = state.ent, state.rel
    K = ent.shape[1]
    k = K // 2
    assert k % 4 == 0 and k <= 2048
    PF = _pf_of("RotatE", k // 4)
    N = ent.shape[0] if n_ents is None else int(n_ents)
    gamma = F32(3.0 if margin is None else margin)
    alpha = F32(alpha)
    feta = F32(float(eta))
    sgn_scale = F32(-1.0)
    div = O.rotate_phase_divisor(k, rel.shape[0] if max_rel_size is None else max_rel_size)
    m = lambda a, b: _f(a * b)   # noqa: E731
    comp = lambda t: (t[:, :k], t[:, k:])   # noqa: E731
    s0, s1 = comp(ent[pos[:, 0]])
    o0, o1 = comp(ent[pos[:, 2]])
    phi = _f(rel[pos[:, 1], :k] / div)
    cs, sn_ = np.cos(phi.astype(np.float64)).astype(F32), np.sin(phi.astype(np.float64)).astype(F32)
    A0, A1 = _f(m(s0, cs) - m(s1, sn_)), _f(m(s0, sn_) + m(s1, cs))      # A = s o r
    B0, B1 = _f(m(o0, cs) + m(o1, sn_)), _f(m(o1, cs) - m(o0, sn_))      # B = o o conj(r)

    def modulus(zr, zi):
        return np.sqrt(_f(m(zr, zr) + m(zi, zi))).astype(F32)

    re, im = _f(A0 - o0), _f(A1 - o1)
    mp = modulus(re, im)
    P = _f(sgn_scale * _unit_chain(mp))
    keep = np.zeros((B, eta), dtype=bool)
    repl = np.zeros((B, eta), dtype=np.int64)
    nsc = np.zeros((B, eta), dtype=F32)
    unit = np.zeros((B, eta, K), dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(eta):
            rows = np.uint64(j) * np.uint64(B) + np.arange(B, dtype=np.uint64)
            kj, rj = sample_corruption_draws(rows, step, seed, N)
            keep[:, j], repl[:, j] = kj.astype(bool), rj
            e0, e1 = comp(ent[rj])
            kk = keep[:, j][:, None]
            zr = np.where(kk, _f(A0 - e0), _f(_f(m(e0, cs) - m(e1, sn_)) - o0))
            zi = np.where(kk, _f(A1 - e1), _f(_f(m(e0, sn_) + m(e1, cs)) - o1))
            mj = modulus(zr, zi)
            nsc[:, j] = _f(sgn_scale * _unit_chain(mj))
            inv = _f(F32(1.0) / mj)
            unit[:, j, :k], unit[:, j, k:] = m(zr, inv), m(zi, inv)
    ar = np.arange(B)
    order = np.argsort(~keep, axis=1, kind="stable")
    nkeep = keep.sum(1)
    av1 = np.zeros((2, B, K), dtype=F32)
    av2 = np.zeros((2, B, K), dtype=F32)
    two = loss == "self_adversarial"

    def add_rows(side, m_, jcol, c1, c2):
        e = unit[ar, jcol]
        av1[side][m_] = fmaf32(c1[:, None], e, av1[side])[m_]
        if two:
            av2[side][m_] = fmaf32(c2[:, None], e, av2[side])[m_]

    def rescale(g_, rs):
        for dd in (0, 1):
            av1[dd] = np.where(g_[:, None], _f(av1[dd] * rs[:, None]), av1[dd])
            av2[dd] = np.where(g_[:, None], _f(av2[dd] * rs[:, None]), av2[dd])

    S, Lw, Zs, m_run = _det_row_protocol(loss, nsc, order, nkeep, eta, alpha, gamma, PF, add_rows, rescale)
    k1, k2, dP, sn, per = _det_finish(loss, P, nsc, S, Lw, Zs, m_run, alpha, gamma, feta)
    k1, k2 = _f(k1 * sgn_scale)[:, None], _f(k2 * sgn_scale)[:, None]
    eo0, eo1 = comp(_f(m(k1, av1[0]) + m(k2, av2[0])))             # Z_obj
    es0, es1 = comp(_f(m(k1, av1[1]) + m(k2, av2[1])))             # Z_subj
    # the positive's own gradient: grad_unit<RotatE>(s, (cos, sin), o, dP * sgn_scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        gm = _f(_f(dP * sgn_scale)[:, None] / mp)
    gs0 = m(gm, _f(m(re, cs) + m(im, sn_)))
    gs1 = m(gm, _f(m(-re, sn_) + m(im, cs)))
    gp0 = m(gm, _f(m(re, _f(m(-s0, sn_) - m(s1, cs))) + m(im, _f(m(s0, cs) - m(s1, sn_)))))
    go0, go1 = m(-gm, re), m(-gm, im)
    # + the corruptions' parts
    gs0 = _f(gs0 + _f(m(eo0, cs) + m(eo1, sn_)))
    gs1 = _f(gs1 + _f(m(eo1, cs) - m(eo0, sn_)))
    go0, go1 = _f(go0 - es0), _f(go1 - es1)
    gp0 = _f(gp0 + _f(_f(m(eo1, A0) - m(eo0, A1)) + _f(m(es1, o0) - m(es0, o1))))
    gs, go = np.concatenate([gs0, gs1], 1), np.concatenate([go0, go1], 1)
    if debug is not None:
        debug.update(P=P, nsc=nsc, keep=keep, repl=repl, gs=gs, go=go, sn=sn, dP=dP, per=per)
    mul = _f(F32(1.0) / div)
    gp = np.concatenate([m(gp0, mul), np.zeros((B, k), dtype=F32)], 1)     # d/dtheta; the second half of a relation row gets nothing
    # ---- tile pass: g (e - S) / |e - S| per corruption entry, the owner's live row e ----
    ent_dest, ent_pos, ent_role, ent_g, ent_vec = [], [], [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(eta):
            g_e = _f(sn[:, j] * sgn_scale)
            live = ~(np.abs(g_e) < F32(np.finfo(np.float32).tiny))   # (an entry whose coefficient is below the smallest normal fp32 number is no entry; NaN is one)
            role = np.where(keep[:, j], 0, 1)
            e0, e1 = comp(ent[repl[:, j]])
            kk = keep[:, j][:, None]
            dr, di = _f(e0 - np.where(kk, A0, B0)), _f(e1 - np.where(kk, A1, B1))
            gmj = _f(g_e[:, None] / modulus(dr, di))
            vec = np.concatenate([m(gmj, dr), m(gmj, di)], 1)
            ent_dest.append(repl[live, j]); ent_pos.append(ar[live]); ent_role.append(role[live]); ent_g.append(g_e[live]); ent_vec.append(vec[live])
    one = np.ones(B, dtype=F32)
    ent_dest += [pos[:, 0], pos[:, 2]]; ent_pos += [ar, ar]; ent_role += [np.full(B, 2), np.full(B, 3)]; ent_g += [one, one]; ent_vec += [gs, go]
    Ge = _sorted_row_sums(ent.shape, ent_dest, ent_pos, ent_role, ent_g, ent_vec)
    Gr = _batch_order_row_sums(rel.shape, pos[:, 1], gp)
    total = float(per.astype(np.float64).sum())
    if return_grads:
        return total, Ge, Gr
    state.apply(Ge, Gr)
    return total


def transe_nll_step_det(state, pos, eta, seed, step, n_ents=None, return_grads=False):
    """TransE / nll in deterministic mode (the first of the transcendental losses to be restated; kept under its own name)."""
    return transe_step_det(state, pos, eta, seed, step, "nll", n_ents=n_ents, return_grads=return_grads)
