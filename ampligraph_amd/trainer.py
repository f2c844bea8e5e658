"""The training step loop shared by ScoringBasedEmbeddingModel.fit() and bench.py.

One process drives one GPU (one `KgeEngine`).  With torch.distributed initialised the loop is data
parallel over the positives of each *global* batch: tables and optimizer state are replicated, rank r
takes the contiguous share [lo_r, hi_r) of the batch, the dense gradient buffers are summed with an
all-reduce (RCCL over xGMI on GPUs; gloo in the CPU tests) and every rank applies the same dense
optimizer sweep.  Negatives are drawn from a counter-based RNG indexed by the GLOBAL corruption row,
so N ranks at batch B/N reproduce exactly the corruptions (and, up to fp32 summation order, the
update) of one rank at batch B.  The reference has no multi-device path at all
(/root/reference: no tf.distribute / NCCL / Horovod call sites); its step is
ScoringBasedEmbeddingModel.train_step :370-429.
"""
import os


def shard_bounds(n, world, rank):
    """Contiguous, balanced split of n rows over `world` ranks (first n % world ranks get one more)."""
    lo = (n * rank) // world
    hi = (n * (rank + 1)) // world
    return lo, hi


# The three features that own a part of the step -- each a (message prefix, reason clause) -- and the modes they were not built for.
# Whoever can see a mode asks refuse_modes: compile() (latent_features/models.py, negatives.py, relation_prediction.py), bind() /
# fit() through fit_modes(model), and StepLoop.step.
SHARED_STEP = ("negatives", "a shared-list step (SharedNegatives, SharedDistanceNegatives, KvsAll) accumulates its gradients in no fixed "
                            "order and ends in one rank's dense sweep")
BATCH_REG = ("batch regularizer", "its gradient rows are added with atomics, in no fixed order, into one rank's dense gradient")
RELATION_TERM = ("relation_prediction", "its gradient rows are added with atomics, in no fixed order, into one rank's dense gradient")


def refuse_modes(prefix, reason, focus=False, multi=False, deterministic=False, lazy=False, sharding="replicated"):
    """Raise NotImplementedError("<prefix>: <reason>; not offered with <the modes that are on>") when any of the given modes is on:
    focus (FocusE), multi (more than one rank), deterministic, lazy (optimizer_mode='lazy'), sharding (entity_sharding other than
    "replicated").  A caller passes the modes it can see and the feature does not run under."""
    if not (focus or multi or deterministic or lazy or sharding != "replicated"):
        return
    on = [name for flag, name in ((focus, "FocusE"), (multi, "more than one rank"), (deterministic, "deterministic mode"),
                                  (lazy, "optimizer_mode='lazy'"), (sharding != "replicated", "entity_sharding='{}' (sharded tables)".format(sharding)))
          if flag]
    raise NotImplementedError("{}: {}; not offered with {}".format(prefix, reason, ", ".join(on)))


# optimizer_mode="sparse" (include/ext/amdkge_sparse.h): the closing sweep visits the step's candidate rows and nothing else
SPARSE_MODE = "optimizer_mode='sparse'"


def refuse_sparse(negatives):
    """Raise NotImplementedError unless `negatives` (a sampler or a bound sampler) names the rows its step can touch: a sampler that
    owns its step (`shared`) and draws FINITE lists (`names_rows`).  Whoever can see the sampler asks: compile() and StepLoop.step."""
    if not getattr(negatives, "shared", False):
        raise NotImplementedError("{}: the sweep visits the rows the step's sampler names, and a step {} names no rows; per-corruption steps "
                                  "have optimizer_mode='lazy'".format(SPARSE_MODE, "without a sampler" if negatives is None else "on override rows"))
    if not getattr(negatives, "names_rows", False):
        raise NotImplementedError("{}: with a list of every entity (num_negs='all' without an `entities` pool, KvsAll) every row is a candidate: "
                                  "the dense sweep is that step's sweep".format(SPARSE_MODE))


def fit_modes(model):
    """The modes refuse_modes can be asked about once fit() has a loop: what bind() of a sampler or of the relation term, and fit()
    itself for a batch regulariser, pass on."""
    loop = getattr(model, "_loop", None)
    return dict(focus=bool(getattr(model, "use_focusE", False)), multi=bool(getattr(loop, "multi", False)),
                deterministic=bool(getattr(loop, "deterministic", False)))


def prefer_tiled(engine):
    """Which fused train path a loop should use when the shape allows both.  Owner-computes (kge_train_tiled.hip)
    wins 2.2x for the trilinear models (single pass over the rows, no global atomics).  TransE / RotatE read the rows
    twice AND re-read side + own rows in the tile pass; measured at the C2 shape (ms/step, atomic vs tiled): TransE
    k=52 0.059 vs 0.089, TransE k=200 0.214 vs 0.161, RotatE k=200 0.358 vs 0.340, RotatE k=1000 eta=64 B=65536
    52.0 vs 37.1 -- so only narrow TransE rows (k < 128) stay on kge_train.hip.  AMDKGE_TRAIN_PATH=atomic|tiled forces."""
    if not hasattr(engine, "train_step_tiled"):
        return False
    force = os.environ.get("AMDKGE_TRAIN_PATH", "")
    if force == "atomic":
        return False
    if force == "tiled":
        return True
    model = getattr(engine, "scoring_type", "ComplEx")
    if model == "TransE":
        return getattr(engine, "k", 0) >= 128
    return True


def hot_rows(triples, batch_size, threshold, limit=64):
    """Entity ids expected to receive more than `threshold` own-row gradients (as s or o of a positive) per batch of
    `batch_size` positives, most frequent first, at most `limit` -- and the expected count of the first entity beyond them."""
    import numpy as np

    t = np.asarray(triples)
    if t.shape[0] == 0:
        return np.zeros(0, dtype=np.int32), 0.0
    cnt = np.bincount(np.concatenate([t[:, 0], t[:, 2]]).astype(np.int64)).astype(np.float64) * (float(batch_size) / float(t.shape[0]))
    order = np.argsort(-cnt, kind="stable")
    n = int((cnt[order] > threshold).sum())
    rest = float(cnt[order[limit]]) if n > limit and len(order) > limit else 0.0
    return order[:min(n, limit)].astype(np.int32), rest


def hot_row_entries(triples, batch_size):
    """Expected number of gradient rows ONE entity receives from the positives of one batch, for the most frequent
    entity of `triples` (numpy (n,3) ids): (count as subject + count as object) / n * batch_size."""
    import numpy as np

    t = np.asarray(triples)
    if t.shape[0] == 0:
        return 0.0
    cnt = np.bincount(np.concatenate([t[:, 0], t[:, 2]]).astype(np.int64))
    return float(cnt.max()) / float(t.shape[0]) * float(batch_size)


HOT_ROW_THRESHOLD = 256.0   # expected entries on one row per batch beyond which the positives' rows go atomic
HOT_ROW_REPLICA_THRESHOLD = 48.0   # expected own-row gradients per batch beyond which an entity gets replica rows


class StepLoop:
    PHASES = ("kernels", "merge+sweep")   # what kernel_hook(i) / kernel_hook(i + 1) bracket

    def __init__(self, engine, eta, loss, optimizer, regularizer=None, seed=0, dist=None, merge=None):
        """engine: KgeEngine-like backend; loss/optimizer: objects with .to_ffi(); dist: None or the
        torch.distributed module (already initialised); merge: how N > 1 ranks merge gradients --
          "sharded"   (default when the backend has flat parameter buffers): reduce-scatter by all_to_all (every rank
                      receives the W partial sums of ITS 1/W slice of the flat gradient over all xGMI links at once and
                      adds them), sharded optimizer sweep (each rank sweeps only its slice: 1/W of the optimizer traffic,
                      m / v effectively sharded), all_to_all of the updated parameter slices (every rank's slice to every
                      peer).  Same bytes on the wire as an all-reduce, but point-to-point on every link at once instead of
                      a ring that is bound by one link.
          "allreduce": one all-reduce of the flat gradient, every rank sweeps everything (AMDKGE_DP_MERGE=allreduce);
          "auto"     : measured on the first steps (tune_merge; AMDKGE_DP_MERGE=auto)."""
        self.engine = engine
        self.eta = int(eta)
        # loss_functions.BCELoss has no amdkge_loss descriptor: it is the loss step of the labelled shared step (KvsAll), which takes
        # its two hyper-parameters as arguments
        self.label_loss = loss if getattr(loss, "labelled", False) else None
        self.loss_ffi = None if self.label_loss is not None else loss.to_ffi()
        self.optimizer = optimizer
        # regulariser of the entity table; the relation table takes `reg_rel` -- "same" (the default: one regulariser for both,
        # EmbeddingLookupLayer.py:153-155), None, or its own object (an [entity, relation] pair, :147-152)
        self.reg = regularizer
        self.reg_rel = "same"
        self.seed = int(seed)
        self.dist = dist
        self.world = dist.get_world_size() if dist is not None else 1
        self.rank = dist.get_rank() if dist is not None else 0
        # the multi-rank form of the step (gradient-only kernels + merge through the collectives).  AMDKGE_FORCE_DIST=1 takes it
        # with a process group of ONE rank too: every collective of the merge then really goes through the backend (RCCL on a GPU)
        # -- the first-contact run a one-GPU box allows (bench.py AMDKGE_BENCH_FORCE_DIST, tests/test_dp_gloo.py)
        self.multi = self.world > 1 or (dist is not None and os.environ.get("AMDKGE_FORCE_DIST", "0") == "1")
        if merge is None:
            merge = os.environ.get("AMDKGE_DP_MERGE", "sharded")
        # "auto": start with the sharded merge and let the caller run tune_merge() on the first steps (fit() does)
        self.auto_tune = merge == "auto"
        if self.auto_tune:
            merge = "sharded"
        if merge not in ("sharded", "allreduce"):
            raise ValueError("merge must be 'sharded', 'allreduce' or 'auto'")
        self.merge = merge if hasattr(engine, "opt_step_flat") else "allreduce"
        if getattr(optimizer, "lazy", False):
            # touched-rows optimizer: rows are the unit of work, the slice-wise sharded sweep would cut them
            self.merge, self.auto_tune = "allreduce", False
        self.merge_report = None
        self.collectives = os.environ.get("AMDKGE_DP_GATHER", "alltoall")   # sharded merge: "alltoall" | "native"
        if self.collectives == "allgather":   # older spelling: all_to_all reduce-scatter + native all_gather
            self.collectives = "alltoall+allgather"
        self.n_steps = 0
        self.use_tiled = prefer_tiled(engine)
        self.pos_atomic = False   # see configure_for_data
        # bitwise reproducible tables (AMDKGE_TILED_DETERMINISTIC): compile(deterministic=True) or AMDKGE_DETERMINISTIC=1,
        # read once here.  Needs the owner-computes path (any k <= 2048); the merged DP sweep already sums in rank order.
        self.deterministic = os.environ.get("AMDKGE_DETERMINISTIC", "0") == "1"
        self.kernel_hook = None   # bench.py: callable(i) recording HIP events at the phase boundaries (PHASES)
        # compile(negatives=...) bound by fit(): None (the train kernels draw their own corruptions) or one of two kinds of bound sampler
        # (latent_features/negatives.py; DESIGN.md "What a bound sampler provides"):
        #   an OVERRIDE sampler (BoundNegatives, BoundTypedNegatives): a callable(global_batch, lo, hi, eta, seed, rng_step) -> int32 device
        #     rows [(hi - lo) * eta, 3], the corruptions of rows [lo, hi) of the global batch drawn by GLOBAL row, which the step hands to
        #     the train kernels as their neg_override; the loop reads nothing else of it;
        #   a sampler that OWNS the backward call (`shared` set: BoundSharedNegatives, BoundMaskedSharedNegatives, BoundKvsAll):
        #     step(global_batch, loss, seed, rng_step) draws and runs its own engine.train_shared*_fwdbwd; the loop reads `shared` and,
        #     for the loss <-> sampler pairing (BCELoss exists only with KvsAll), `labelled`.
        self.negatives = None
        # compile(relation_prediction=...): None or an object with .step(batch) (latent_features/relation_prediction.py:
        # BoundRelationPrediction), the relation-prediction term -- engine.train_relation_fwdbwd on the batch, between the backward call
        # and the dense sweep, before the batch regulariser
        self.relation = None
        engine.prepare_training(optimizer.name)
        if hasattr(optimizer, "bind"):
            optimizer.bind(engine)   # get_weights() / set_weights() of the wrapper read and write the engine's state tensors
        if self.merge == "sharded" and self.multi and int(engine.g_flat.numel()) % self.world != 0:
            self.merge = "allreduce"   # the flat buffers split evenly over 1, 2, 4, 8, 16 ranks; other counts all-reduce

    def configure_for_data(self, triples, batch_size):
        """Pick the owner-computes variant for this training set (host-side, once per fit): skewed graphs route the
        positives' own s / o gradient rows through atomics (AMDKGE_TILED_POS_ATOMIC)."""
        per_rank = -(-int(batch_size) // self.world)
        self.pos_atomic = False
        # deterministic mode on a skewed graph: a hub's tile receives many times a bucket -- ask for the wide sort buffer
        # (AMDKGE_TILED_DET_WIDE_SORT: smaller tiles; uniform graphs keep the default mode's geometry)
        self.det_wide = bool(self.deterministic) and hot_row_entries(triples, per_rank) > HOT_ROW_REPLICA_THRESHOLD
        if self.deterministic or not hasattr(self.engine, "set_hot_rows"):
            self.pos_atomic = (not self.deterministic) and hot_row_entries(triples, per_rank) > HOT_ROW_THRESHOLD
            return self.pos_atomic
        # skewed graphs: the (up to 64) entities that are the s / o of many positives of a batch get replica rows
        # (AMDKGE_TILED_HOT_ROWS); only if even the 65th entity is that hot do ALL positives' rows go through atomics
        ids, rest = hot_rows(triples, per_rank, HOT_ROW_REPLICA_THRESHOLD)
        self.engine.set_hot_rows(ids)
        self.pos_atomic = rest > HOT_ROW_THRESHOLD
        return self.pos_atomic

    def step(self, global_batch, rng_step, focus=None):
        """global_batch: (Bg,3) int32 device tensor holding the WHOLE batch (same on every rank);
        rng_step: the step counter the negatives are keyed by; focus: None or (w fp32 device tensor [Bg], beta,
        non-linearity name) for FocusE (ScoringBasedEmbeddingModel.py:396-406).

        Pairing check and refusals -> the optimizer's clock and the descriptors -> hook 0 -> ONE backward call (the sampler's own
        step, the owner-computes step, or train_fwdbwd) -> the dense extras (relation term, batch regulariser) -> hook 1 -> merge
        and / or sweep (optimizer_mode="sparse": engine.opt_step_rows on the sampler's candidate_rows) -> hook 2.  Everything that can
        refuse a step does so before anything is touched."""
        eng, neg, relation = self.engine, self.negatives, self.relation
        bg = int(global_batch.shape[0])
        lo, hi = shard_bounds(bg, self.world, self.rank)
        labelled = getattr(neg, "labelled", False)
        if self.label_loss is not None:
            if focus is not None or not labelled:
                raise NotImplementedError("BCELoss is the loss of the labelled shared step: it needs compile(negatives=KvsAll(...)) and takes no FocusE")
        elif labelled:
            raise NotImplementedError("KvsAll labels every entity for a binary cross-entropy: it needs loss=BCELoss(...)")
        lam = self.reg    # LPRegularizer objects (or None): the engine turns them into the descriptor's (p, lambda) terms
        lam_r = self.reg if isinstance(self.reg_rel, str) else self.reg_rel
        # BatchLPRegularizer members (N3, per-occurrence Lp: include/amdkge_batch_reg.h) act on the rows of this step's positives:
        # engine.batch_reg_fwdbwd between the backward call and the dense sweep, which then takes only the whole-table members
        breg_e = lam if getattr(lam, "batch", False) else None
        breg_r = lam_r if getattr(lam_r, "batch", False) else None
        batch_reg = breg_e is not None or breg_r is not None
        if batch_reg:
            refuse_modes(*BATCH_REG, focus is not None, self.multi, self.deterministic, getattr(self.optimizer, "lazy", False))
            lam = None if breg_e is not None else lam
            lam_r = None if breg_r is not None else lam_r
        if relation is not None:
            refuse_modes(*RELATION_TERM, focus is not None, self.multi, self.deterministic, getattr(self.optimizer, "lazy", False))
        owns = getattr(neg, "shared", False)   # the sampler runs the backward call itself (kge_train_shared*.hip), on the whole batch
        sparse = getattr(self.optimizer, "sparse", False)   # the sweep visits the sampler's candidate rows (include/ext/amdkge_sparse.h)
        if sparse:
            refuse_sparse(neg)
        if owns:
            refuse_modes(*SHARED_STEP, focus is not None, self.multi, self.deterministic)
        # owner-computes path (kge_train_tiled.hip) whenever the shape allows it: no global atomics, no dense
        # entity gradient; data-parallel runs take its gradient-only form and keep the dense sweep
        # (a batch regulariser and the relation-prediction term need the dense entity gradient, which the owner-computes step never
        # materialises)
        tiled = (not owns and (self.use_tiled or self.deterministic) and not batch_reg and relation is None and hi > lo
                 and eng.tiled_supported(hi - lo, self.eta))
        if self.deterministic and hi > lo and not tiled:
            raise ValueError("deterministic mode needs the owner-computes train path (k <= 2048)")
        self.optimizer.iterations += 1
        if focus is not None:
            from . import _ffi

            fw = focus[0][lo:hi].contiguous()   # kept alive until the launches below are enqueued
            self.loss_ffi.focus_nonlinearity = _ffi.FOCUS_NONLINEARITY[focus[2]]
            self.loss_ffi.focus_beta = float(focus[1])
            self.loss_ffi.d_focus_w = fw.data_ptr()
        elif self.loss_ffi is not None:
            self.loss_ffi.focus_nonlinearity = 0
            self.loss_ffi.d_focus_w = None
        opt_ffi = self.optimizer.to_ffi(self.optimizer.iterations, 2)
        if self.kernel_hook is not None:
            self.kernel_hook(0)
        rows, n_rows = (global_batch, bg) if owns else (global_batch[lo:hi], hi - lo)   # what this rank's backward call and extras work on
        if owns and n_rows > 0:
            neg.step(rows, self.label_loss if labelled else self.loss_ffi, self.seed, rng_step)
        elif n_rows > 0:
            # (the override keyword is only passed when a sampler is set: backends without it keep working)
            over = {"neg_override": neg(global_batch, lo, hi, self.eta, self.seed, rng_step)} if neg is not None else {}
            if tiled:
                eng.train_step_tiled(rows, self.eta, self.loss_ffi, opt_ffi, self.seed, rng_step,
                                     reg_e=lam, reg_r=lam_r, row_offset=lo, b_global=bg, grad_only=self.multi,
                                     pos_atomic=self.pos_atomic, **over,
                                     **({"deterministic": True, **({"det_wide": True} if getattr(self, "det_wide", False) else {})} if self.deterministic else {}))
            else:
                eng.train_fwdbwd(rows, self.eta, self.loss_ffi, self.seed, rng_step, row_offset=lo, b_global=bg, **over)
        # the dense extras (never next to the owner-computes step: tiled is off with either)
        if relation is not None and n_rows > 0:
            relation.step(rows)
        if batch_reg and n_rows > 0:
            eng.batch_reg_fwdbwd(rows, breg_e, breg_r)
        if self.kernel_hook is not None:
            self.kernel_hook(1)
        if self.multi and self.merge == "sharded":
            self._merge_sharded(opt_ffi, lam, lam_r)
        else:
            if self.multi:
                for g in eng.grad_tensors():
                    self.dist.all_reduce(g)
            if sparse:   # (one rank, a sampler that owns its step: refused above otherwise)
                cand, n_cand = neg.candidate_rows(rows)
                eng.opt_step_rows(opt_ffi, lam, lam_r, cand, n_cand, int(cand.numel()))
            elif not (tiled and not self.multi):   # the single-GPU owner-computes call is the complete step
                eng.opt_step(opt_ffi, lam, lam_r)
        if self.kernel_hook is not None:
            self.kernel_hook(2)
        self.n_steps += 1

    def _merge_sharded(self, opt_ffi, lam, lam_r):
        """Reduce-scatter (all_to_all of the partial slices), sharded sweep that sums the W partials on the fly
        (amdkge_opt_step_merged), parameters back to everyone.  Only collectives and libamdkge calls: no torch compute op,
        no host synchronisation."""
        eng, W, r = self.engine, self.world, self.rank
        g, p = eng.g_flat, eng.p_flat
        chunk = g.numel() // W                      # the flat buffers are padded to a multiple of 16 * 64 floats
        lo, hi = r * chunk, (r + 1) * chunk
        merged = hasattr(eng, "opt_step_merged")
        if self.collectives == "native":            # the library's own reduce-scatter / all-gather schedules
            red = eng._buf("dp_red", (chunk,), g.dtype) if merged else g.new_empty(chunk)
            self.dist.reduce_scatter_tensor(red, g)
            parts, n_parts = red, 1
        else:
            parts = eng._buf("dp_recv", (g.numel(),), g.dtype) if merged else g.new_empty(g.numel())
            self.dist.all_to_all_single(parts, g)   # parts[q*chunk:(q+1)*chunk] = rank q's partial sums of MY slice
            n_parts = W
        if merged:
            # the spent gradient buffer is cleared on the stream (the tile kernel stores the entity part anyway; the
            # relation part and, with atomic positives, everything must start at zero)
            eng.zero_(g)
            eng.opt_step_merged(opt_ffi, lo, hi, parts, n_parts, chunk, lam, lam_r, reg_slot=1)
        else:   # backends without the fused kernel (CPU test double): explicit sum + slice sweep
            import torch

            g.zero_()
            torch.sum(parts.view(n_parts, chunk), dim=0, out=g[lo:hi])
            eng.opt_step_flat(opt_ffi, lo, hi, lam, lam_r, reg_slot=1)   # leaves my gradient slice zero
        self._gather_slices(p)   # parameters back to everyone

    def _gather_slices(self, flat):
        """Every rank's slice of `flat` to every peer, in place.  "alltoall": W - 1 point-to-point sends of MY slice and
        W - 1 receives into the peers' slices, batched into one group -- every xGMI link carries one slice at once, where a
        ring all-gather pushes W - 1 hops through each link in turn; the other schedules use the library's all-gather."""
        W, r = self.world, self.rank
        chunk = flat.numel() // W
        mine = flat[r * chunk:(r + 1) * chunk]
        if self.collectives == "alltoall" and hasattr(self.dist, "batch_isend_irecv"):
            ops = []
            for q in range(W):
                if q != r:
                    ops.append(self.dist.P2POp(self.dist.isend, mine, q))
                    ops.append(self.dist.P2POp(self.dist.irecv, flat[q * chunk:(q + 1) * chunk], q))
            for req in (self.dist.batch_isend_irecv(ops) if ops else ()):   # (a group of one rank has nobody to send to)
                req.wait()
        else:
            self.dist.all_gather_into_tensor(flat, mine)

    def tune_merge(self, batch_of, first_step=0, trials=4, pick=None):
        """Measure the merge schedules on THIS machine's fabric and keep the fastest (collective: call on every rank).

        Every schedule computes the same update (up to fp32 summation order), so the 1 + `trials` steps spent on each
        candidate are ordinary training steps: batch_of(step) -> global batch, steps first_step, first_step + 1, ...
        Which schedule wins depends on the RCCL version and the xGMI topology (ring all-reduce vs. point-to-point
        all_to_all vs. the library's reduce-scatter/all-gather), which is why it is measured rather than assumed.
        Resets the loss accumulators (the schedules book the regulariser term differently).  Returns the number of
        steps consumed; the choice is left in self.merge / self.collectives and described by self.merge_report.
        pick: optional callable(candidates, seconds) -> index overriding "fastest" (must agree on every rank)."""
        import time

        import torch

        self.merge_report = None
        if not self.multi or not hasattr(self.engine, "opt_step_flat") or int(self.engine.g_flat.numel()) % self.world:
            return 0
        backend = getattr(self.dist, "get_backend", lambda: "")()
        cands = [("allreduce", self.collectives), ("sharded", "alltoall"), ("sharded", "alltoall+allgather")]
        if backend == "nccl":   # gloo has no reduce_scatter_tensor
            cands.append(("sharded", "native"))
        cuda = torch.cuda.is_available()
        step, times = int(first_step), []
        dev = self.engine.g_flat.device

        def usable(coll):
            """Probe the collectives of a schedule on scratch tensors first: a backend build that rejects one (raised at
            call time, identically on every rank) drops the candidate before any training state is touched."""
            W = self.world
            a, b = torch.zeros(W * 4, device=dev), torch.zeros(W * 4, device=dev)
            try:
                if coll.startswith("alltoall"):
                    self.dist.all_to_all_single(b, a)
                if coll == "native":
                    self.dist.reduce_scatter_tensor(b[:4], a)
                if coll != "alltoall" or not hasattr(self.dist, "batch_isend_irecv"):
                    self.dist.all_gather_into_tensor(b, b[self.rank * 4:(self.rank + 1) * 4])
                else:   # the point-to-point return of _gather_slices, on the scratch tensor
                    ops = []
                    for q in range(W):
                        if q != self.rank:
                            ops.append(self.dist.P2POp(self.dist.isend, b[self.rank * 4:(self.rank + 1) * 4], q))
                            ops.append(self.dist.P2POp(self.dist.irecv, b[q * 4:(q + 1) * 4], q))
                    for req in (self.dist.batch_isend_irecv(ops) if ops else ()):
                        req.wait()
            except RuntimeError:
                return False
            return True

        for merge, coll in cands:   # all-reduce first: it needs complete optimizer slots on every rank
            if merge == "sharded" and not usable(coll):
                times.append(float("inf"))
                continue
            self.merge, self.collectives = merge, coll
            self.step(batch_of(step), step)
            step += 1
            if cuda:
                torch.cuda.synchronize()
            self.dist.barrier()
            t0 = time.perf_counter()
            for _ in range(int(trials)):
                self.step(batch_of(step), step)
                step += 1
            if cuda:
                torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / max(1, int(trials)))
        t = torch.tensor(times, dtype=torch.float64, device=self.engine.g_flat.device)
        self.dist.all_reduce(t, op=torch.distributed.ReduceOp.MAX)   # slowest rank decides, same choice everywhere
        best = int(torch.argmin(t).item()) if pick is None else int(pick(cands, t.tolist()))
        if cands[best][0] == "allreduce":
            self.sync_optimizer_slots()   # the sharded candidates left every rank with only ITS slice up to date
        self.merge, self.collectives = cands[best]
        self.merge_report = {f"{m}/{c}" if m == "sharded" else m: (float(x) * 1e3 if x != float("inf") else None)
                             for (m, c), x in zip(cands, t.tolist())}
        self.reset_loss()
        return step - int(first_step)

    def sync_optimizer_slots(self):
        """Sharded merge: every rank only maintains ITS slice of the optimizer slots.  Before a checkpoint is written
        the slices are exchanged so that any rank holds the complete m / v / accumulator tables."""
        if not self.multi or self.merge != "sharded":
            return
        W, r = self.world, self.rank
        for fl in self.engine.slot_flat.values():
            self._gather_slices(fl)

    def reset_loss(self):
        self.engine.loss_acc.zero_()
        self.n_steps = 0

    def mean_batch_loss(self):
        """Keras Mean('loss') of the per-batch total loss (loss_functions.py:224): (sum over batches of
        data loss + regulariser loss) / #batches.  The data loss is summed over ranks; the regulariser
        term is identical on every rank (replicated tables, all-reduce merge: counted once) or split over the
        ranks' slices (sharded merge: summed)."""
        st = self.engine.tiled_status() if hasattr(self.engine, "tiled_status") else 0   # (0 without a sync unless it can be set)
        if self.deterministic and st:
            raise RuntimeError("deterministic mode: a tile received more entries than its sort buffer holds (very hot rows); "
                               "this epoch's sums were not all added in canonical order")
        acc = self.engine.loss_acc.clone()
        if self.multi and self.merge == "sharded":
            both = acc[0:2].clone()
            self.dist.all_reduce(both)
            acc[0], acc[1] = both[0], both[1]
        elif self.multi:
            data = acc[0:1].clone()
            self.dist.all_reduce(data)
            acc[0] = data[0]
        tot = float(acc[0].item()) + float(acc[1].item()) + float(acc[2].item())
        return tot / max(1, self.n_steps)
