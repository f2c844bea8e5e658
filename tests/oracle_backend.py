"""CPU stand-in for KgeEngine built on the oracle -- TEST INFRASTRUCTURE: lets the host-side
data-parallel logic of ampligraph_amd.trainer.StepLoop (batch sharding, global RNG rows, gradient
all-reduce, loss aggregation) run under gloo on a GPU-less box."""
import numpy as np
import torch

from oracle import kge_oracle as O

LOSS_BY_ID = {0: "pairwise", 1: "nll", 2: "absolute_margin", 3: "self_adversarial", 4: "multiclass_nll"}
OPT_BY_ID = {0: "sgd", 1: "adagrad", 2: "adam"}



def _terms(reg, default_p):
    """regulariser argument of the engine surface (a bare lambda, or an object with .terms) -> [(p, lambda), ...]"""
    if reg is None:
        return []
    if isinstance(reg, (int, float)):
        return [(int(default_p), float(reg))] if reg else []
    return list(reg.terms)


class OracleEngine:
    def __init__(self, model, k, ent, rel, tiled=False, flat=False, cols=None):
        """cols = (k_full, world, rank): this engine holds a COLUMN SLICE (k = k_full / world units of every row, ent / rel given as
        the slice) -- the calling convention of KgeEngine(..., k_full=...): cols_partial_scores, cols_loss, train_step_tiled(given=)."""
        self.model, self.k = model, k
        self.cols = cols
        self.flat = flat   # flat parameter / gradient / slot buffers like KgeEngine (sharded-optimizer merge)
        self.flat_sweeps = 0
        if flat:
            self.opt_step_flat = self._opt_step_flat
        if tiled:   # expose the owner-computes entry points of KgeEngine (same calling convention)
            self.train_step_tiled = self._train_step_tiled
            self.tiled_supported = lambda B, eta: True
        self.ent0, self.rel0 = ent.copy(), rel.copy()
        self.n_ents, self.n_rels = ent.shape[0], rel.shape[0]
        self.loss_acc = torch.zeros(3, dtype=torch.float64)
        self.state = None
        self.calls = []

    @property
    def ent(self):
        """The entity table as a torch tensor sharing memory with the oracle state (row-sharded plumbing writes
        fetched rows into it)."""
        return torch.from_numpy(self.state.ent if self.state is not None else self.ent0)

    @property
    def rel(self):
        return torch.from_numpy(self.state.rel if self.state is not None else self.rel0)

    # ---- multi-GPU data path of KgeEngine (kge_shard.hip), restated with torch CPU ops -------------------------------
    def _buf(self, name, shape, dtype):
        return torch.empty(*shape, dtype=dtype)

    def zero_(self, t):
        t.zero_()

    def shard_route(self, spec, triples, negs, cap):
        """amdkge_shard_route: local index space + per-peer request lists (-1 padded), distinct ids share a scratch row."""
        W = spec.world
        cols = [triples[:, 0], triples[:, 2]] + ([negs[:, 0], negs[:, 2]] if negs is not None else [])
        ids = torch.cat(cols).to(torch.int64)
        remote = (ids < spec.lo) | (ids >= spec.hi)
        rid, rinv = torch.unique(ids[remote], return_inverse=True)
        owner = torch.div(rid, spec.rows_per, rounding_mode="floor")
        send_ids = torch.full((W * cap,), -1, dtype=torch.int32)
        counts = torch.zeros(W + 1, dtype=torch.int32)
        slot = torch.zeros_like(rid)
        for q in range(W):
            m = owner == q
            n = int(m.sum())
            counts[q] = n
            if n > cap:
                counts[W] = 1
                n = cap
            pos = torch.arange(int(m.sum())).clamp(max=cap - 1)
            slot[m] = q * cap + pos
            send_ids[q * cap:q * cap + n] = (rid[m][:n] - q * spec.rows_per).to(torch.int32)
        loc = ids - spec.lo
        loc[remote] = spec.n_local + slot[rinv]
        b = int(triples.shape[0])
        xl = torch.stack([loc[:b], triples[:, 1].to(torch.int64), loc[b:2 * b]], 1).to(torch.int32).contiguous()
        nl = None
        if negs is not None:
            nn = int(negs.shape[0])
            nl = torch.stack([loc[2 * b:2 * b + nn], negs[:, 1].to(torch.int64), loc[2 * b + nn:]], 1).to(torch.int32).contiguous()
        if not hasattr(self, "_route_counts"):
            self._route_counts = counts
        else:
            self._route_counts[:W] = counts[:W]
            self._route_counts[W] |= counts[W]
        return xl, nl, send_ids, self._route_counts

    def zero_route_overflow(self):
        if hasattr(self, "_route_counts"):
            self._route_counts[-1] = 0

    def gather_rows(self, table, idx, name="gathered"):
        i = idx.to(torch.int64)
        out = table[i.clamp(min=0)].clone()
        out[i < 0] = 0
        return out

    def scatter_add_rows(self, table, idx, src):
        i = idx.to(torch.int64)
        table.index_add_(0, i[i >= 0], src[i >= 0])

    def sample_corruptions(self, triples, eta, seed, step, sample_base=0, sample_range=None, row_offset=0, b_global=0):
        X = triples.numpy()
        negs = O.generate_corruptions(X, int(sample_range or self.n_ents), eta, seed, step, row_offset,
                                      b_global or X.shape[0])
        assert sample_base == 0
        return torch.as_tensor(negs.astype(np.int32))

    def rank_side(self, triples, side, strategy="worst", flt=None, ent_ids=None, subset_pos=None, ent_lo=0,
                  ent_hi=None, out=None, out_stride=1, flt_range=None):
        """(None, counts (n,2) [greater, equal], sub (n,) or None) like KgeEngine.rank_side, on rows [ent_lo, ent_hi)."""
        X = triples.numpy().astype(np.int64)
        ent, rel = self.ent.numpy(), self.rel.numpy()
        s, p, o = O.lookup(ent, rel, X)
        tq = O.quantise(O.compute_scores(self.model, s, p, o, max_rel_size=self.n_rels))
        cand = ent[ent_lo:ent_hi] if ent_ids is None else ent[ent_ids.numpy().astype(np.int64)[ent_lo:ent_hi]]
        cq = O.quantise(O.corruption_scores(self.model, "s" if side == 1 else "o", s, p, o, cand, self.n_rels))
        counts = np.stack([(tq[:, None] < cq).sum(1), (tq[:, None] == cq).sum(1)], 1).astype(np.int32)
        sub = None
        if flt is not None:
            lo, hi, ids = (t.numpy() for t in flt)
            sub = np.zeros(len(X), dtype=np.int32)
            for i in range(len(X)):
                f = ids[lo[i]:hi[i]].astype(np.int64)
                if flt_range is None:
                    f = f[(f >= ent_lo) & (f < ent_hi)] - ent_lo
                    sub[i] = int((tq[i] <= cq[i, f]).sum())
                else:   # filter ids are table rows in flt_range, scored directly (candidates are a subset list)
                    f = f[(f >= flt_range[0]) & (f < flt_range[1])]
                    fq = O.quantise(O.corruption_scores(self.model, "s" if side == 1 else "o", s[i:i + 1], p[i:i + 1],
                                                        o[i:i + 1], ent[f], self.n_rels))[0] if len(f) else np.zeros(0)
                    sub[i] = int((tq[i] <= fq).sum())
            sub = torch.as_tensor(sub)
        return None, torch.as_tensor(counts), sub

    def prepare_training(self, optimizer):
        self.state = O.TrainState(self.ent0, self.rel0, optimizer, 0.0)
        ne, nr = self.ent0.size, self.rel0.size
        if not self.flat:
            self.g_flat = torch.zeros(ne + nr, dtype=torch.float32)
            self.g_ent = self.g_flat[:ne].view(self.ent0.shape)
            self.g_rel = self.g_flat[ne:].view(self.rel0.shape)
            return
        # KgeEngine layout: [entity | pad to 64 | relation | pad to 1024]
        self._ne, self._nr, self._off = ne, nr, (ne + 63) // 64 * 64
        n = (self._off + nr + 1023) // 1024 * 1024

        def flat_of(a_e, a_r, fill=0.0):
            f = np.full(n, fill, dtype=np.float32)
            f[:ne] = a_e.reshape(-1)
            f[self._off:self._off + nr] = a_r.reshape(-1)
            return f

        self._p = flat_of(self.state.ent, self.state.rel)
        self.state.ent = self._p[:ne].reshape(self.ent0.shape)          # numpy views: the oracle updates in place
        self.state.rel = self._p[self._off:self._off + nr].reshape(self.rel0.shape)
        self._slot_flat = {}
        for key in sorted({k.rsplit("_", 1)[0] for k in self.state.slots}):
            f = flat_of(self.state.slots[key + "_e"], self.state.slots[key + "_r"], fill=0.1 if key == "a" else 0.0)
            self._slot_flat[key] = f
            self.state.slots[key + "_e"] = f[:ne].reshape(self.ent0.shape)
            self.state.slots[key + "_r"] = f[self._off:self._off + nr].reshape(self.rel0.shape)
        self.p_flat = torch.from_numpy(self._p)
        self.g_flat = torch.zeros(n, dtype=torch.float32)
        self.g_ent = self.g_flat[:ne].view(self.ent0.shape)
        self.g_rel = self.g_flat[self._off:self._off + nr].view(self.rel0.shape)

    def _opt_step_flat(self, opt, lo, hi, reg_e=0.0, reg_r=0.0, reg_slot=1):
        """Sweep elements [lo, hi) of the flat vector only: run the whole-table oracle sweep, then put everything outside
        the slice back."""
        self.flat_sweeps += 1
        keep_p = self._p.copy()
        keep_s = {k: v.copy() for k, v in self._slot_flat.items()}
        reg_before = self.loss_acc.clone()
        self._sweep(opt, reg_e, reg_r, (reg_slot, reg_slot), None)
        self.loss_acc.copy_(reg_before)
        for reg, a, b in ((reg_e, max(lo, 0), min(hi, self._ne)), (reg_r, max(lo, self._off), min(hi, self._off + self._nr))):
            for pw, lam in _terms(reg, opt.reg_p):
                if b > a:
                    self.loss_acc[reg_slot] += lam * float((np.abs(keep_p[a:b].astype(np.float64)) ** pw).sum())
        mask = np.ones(self._p.shape, dtype=bool)
        mask[lo:hi] = False
        self._p[mask] = keep_p[mask]
        for k, v in self._slot_flat.items():
            v[mask] = keep_s[k][mask]

    @property
    def slot_flat(self):
        return {k: torch.from_numpy(v) for k, v in self._slot_flat.items()}

    def grad_tensors(self):
        return [self.g_flat]

    def train_fwdbwd(self, triples, eta, loss, seed, step, row_offset=0, b_global=0, sample_base=0,
                     sample_range=None, neg_override=None, **kw):
        X = triples.numpy()
        self.calls.append((int(X.shape[0]), int(row_offset), int(b_global), int(step)))
        if neg_override is not None:
            negs = neg_override.numpy()
        else:
            assert sample_base == 0
            negs = O.generate_corruptions(X, int(sample_range or self.n_ents), eta, seed, step, row_offset,
                                          b_global or X.shape[0])
        total, Ge, Gr, _ = O.dense_gradients(self.model, self.state.ent, self.state.rel, X, negs, eta,
                                             LOSS_BY_ID[loss.kind], {"margin": loss.margin, "alpha": loss.alpha},
                                             "mean" if loss.reduction_mean else "sum", self.n_rels)
        self.g_ent += torch.as_tensor(Ge.astype(np.float32))
        self.g_rel += torch.as_tensor(Gr.astype(np.float32))
        self.loss_acc[0] += float(total)

    # ---- column-sharded step (kge_train_cols.hip): the slice embedded in zero columns of the whole width scores and differentiates
    #      like the slice of the whole model (every score is a sum over units; HolE's 2 / k and RotatE's phase normaliser are the
    #      whole model's) ----
    def _embed(self, a):
        k_full, W, r = self.cols
        kp = k_full // W
        cx = self.model in ("ComplEx", "HolE", "RotatE")
        out = np.zeros((a.shape[0], (2 if cx else 1) * k_full), dtype=np.float32)
        out[:, r * kp:(r + 1) * kp] = a[:, :kp]
        if cx:
            out[:, k_full + r * kp:k_full + (r + 1) * kp] = a[:, kp:]
        return out

    def _unembed(self, a):
        k_full, W, r = self.cols
        kp = k_full // W
        cx = self.model in ("ComplEx", "HolE", "RotatE")
        parts = [a[:, r * kp:(r + 1) * kp]] + ([a[:, k_full + r * kp:k_full + (r + 1) * kp]] if cx else [])
        return np.concatenate(parts, 1)

    def _sgn_scale(self):
        return -1.0 if self.model in ("TransE", "RotatE") else (2.0 / self.cols[0] if self.model == "HolE" else 1.0)

    def cols_partial_scores(self, triples, eta, seed, step, sample_base=0, sample_range=None, row_offset=0, b_global=0, neg_override=None, out=None):
        X = triples.numpy()
        negs = O.generate_corruptions(X, int(sample_range or self.n_ents), eta, seed, step, row_offset, b_global or X.shape[0])
        E, Rl = self._embed(self.state.ent), self._embed(self.state.rel)
        sp = O.compute_scores(self.model, *O.lookup(E, Rl, X.astype(np.int64)), max_rel_size=self.n_rels)
        sn = O.compute_scores(self.model, *O.lookup(E, Rl, negs.astype(np.int64)), max_rel_size=self.n_rels)
        self._negs = negs
        return torch.as_tensor((np.concatenate([sp, sn]).astype(np.float64) / self._sgn_scale()).astype(np.float32))

    def cols_loss(self, loss, scores, B, eta):
        sc = scores.numpy().astype(np.float64) * self._sgn_scale()
        total, per, dP, dN = O.loss_and_grads(LOSS_BY_ID[loss.kind], sc[:B].astype(np.float32), sc[B:].astype(np.float32), eta,
                                              {"margin": loss.margin, "alpha": loss.alpha}, "mean" if loss.reduction_mean else "sum")
        self.loss_acc[0] += float(total)
        scores.copy_(torch.as_tensor(np.concatenate([dP, dN]).astype(np.float32)))
        return scores

    def _given_grads(self, triples, eta, given):
        X = triples.numpy().astype(np.int64)
        B = X.shape[0]
        coef = given.numpy().astype(np.float64)
        E, Rl = self._embed(self.state.ent), self._embed(self.state.rel)
        Ge, Gr = np.zeros(E.shape), np.zeros(Rl.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            for tri, g in ((X, coef[:B]), (self._negs.astype(np.int64), coef[B:])):
                gs, gp, go = O.score_grads(self.model, *O.lookup(E, Rl, tri), self.n_rels)
                np.add.at(Ge, tri[:, 0], g[:, None] * gs)
                np.add.at(Gr, tri[:, 1], g[:, None] * gp)
                np.add.at(Ge, tri[:, 2], g[:, None] * go)
        self.g_ent += torch.as_tensor(self._unembed(Ge).astype(np.float32))
        self.g_rel += torch.as_tensor(self._unembed(Gr).astype(np.float32))

    def _train_step_tiled(self, triples, eta, loss, opt, seed, step, reg_e=0.0, reg_r=0.0, row_offset=0,
                          b_global=0, grad_only=False, given=None, **kw):
        """amdkge_train_step_tiled: grad_only stores the entity gradient (overwrite) and adds the relation
        gradient; otherwise it is the complete step (both tables updated, gradients left zero).  given: the column-sharded
        step's coefficient buffer (AMDKGE_TILED_GIVEN_COEFFS)."""
        kw.pop("pos_atomic", None)
        kw.pop("deterministic", None)
        kw.pop("det_wide", None)
        if given is not None:
            self._given_grads(triples, eta, given)
            if not grad_only:
                self.opt_step(opt, reg_e, reg_r)
            return
        if grad_only:
            self.g_ent.zero_()   # staged positives: the entity gradient is stored, not added
        self.train_fwdbwd(triples, eta, loss, seed, step, row_offset=row_offset, b_global=b_global, **kw)
        if not grad_only:
            self.opt_step(opt, reg_e, reg_r)

    def opt_step(self, opt, lam_e=0.0, lam_r=0.0, rows_e=None, reg_slots=(1, 1)):
        if rows_e is not None:   # row-sharded mode: only the first rows_e rows are this rank's
            keep = self.state.ent[rows_e:].copy()
            keep_slots = {k: v[rows_e:].copy() for k, v in self.state.slots.items() if k.endswith("_e")}
            self.g_ent[rows_e:].zero_()
            self._sweep(opt, lam_e, lam_r, reg_slots, rows_e)
            self.state.ent[rows_e:] = keep
            for k, v in keep_slots.items():
                self.state.slots[k][rows_e:] = v
            return
        self._sweep(opt, lam_e, lam_r, reg_slots, None)

    def _sweep(self, opt, lam_e, lam_r, reg_slots, rows_e):
        self.state.lr = opt.lr
        self.state.iterations = opt.iteration - 1
        Ge, Gr = self.g_ent.numpy().astype(np.float64), self.g_rel.numpy().astype(np.float64)
        for x, G, lam, slot, rows in ((self.state.ent, Ge, lam_e, reg_slots[0], rows_e), (self.state.rel, Gr, lam_r, reg_slots[1], None)):
            for pw, lm in _terms(lam, opt.reg_p):
                xx = x.astype(np.float64)
                if rows is not None:
                    xx = xx.copy()
                    xx[rows:] = 0.0   # scratch rows carry no regulariser
                self.loss_acc[slot] += lm * float((np.abs(xx) ** pw).sum())
                G += lm * pw * np.abs(xx) ** (pw - 1) * np.sign(xx)
        kind = self.state.optimizer   # the descriptor's beta1 / beta2 carry other hyper-parameters for the non-Adam rules
        if kind in ("adam", "adamax", "adagrad", "sgd"):
            O.apply_optimizer(self.state, Ge, Gr, opt.beta1, opt.beta2, opt.epsilon)
        else:
            self.state.hp = {"momentum": {"momentum": opt.beta1, "nesterov": opt.beta2 != 0.0},
                             "rmsprop": {"rho": opt.beta1}, "rmsprop_mom": {"rho": opt.beta1, "momentum": opt.beta2},
                             "adadelta": {"rho": opt.beta1}}[kind]
            self.state.hp["epsilon"] = opt.epsilon
            O.apply_optimizer(self.state, Ge, Gr)
        self.g_ent.zero_()
        self.g_rel.zero_()
