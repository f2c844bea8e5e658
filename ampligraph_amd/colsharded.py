"""COLUMN-SHARDED tables (`compile(entity_sharding="columns")`, `bench.py --parallelism columns`).

For tables that FIT every GPU (BASELINE.json configs[1] - [3]) the data-parallel modes of trainer.py / sharded.py move about one
table per step and direction (dense Adam touches every row of a 14 505-row table every step), which bounds 8-GPU scaling near 3-4x.
All five scoring functions are SUMS OVER UNITS (TransE.py:51-53, DistMult.py:48, ComplEx.py:58-62, HolE.py:45, RotatE.py:100-104),
so the tables can instead be cut by COLUMNS: rank r holds units [r k / W, (r + 1) k / W) of every entity and relation row (the re
and im slices of the same units for the complex models) with the optimizer state of those columns, EVERY rank processes the WHOLE
global batch on its slice, and the one exchange of a step is the all-reduce of the B (1 + eta) partial score sums -- 6.7 MB at
B = 80 000, eta = 20, whatever the table size.  Loss, backward, gradient merge, regulariser and optimizer are element-wise in the
columns and stay local (kge_train_cols.hip).  What a step replaces is ScoringBasedEmbeddingModel.train_step
(ScoringBasedEmbeddingModel.py:370-429) on one global batch; the reference has no multi-device path.  W ranks compute one GPU's
step up to fp32 summation order: every rank draws the same Philox corruptions for the whole batch.
"""
import numpy as np

COMPLEX = ("ComplEx", "HolE", "RotatE")


def column_slice(dense, scoring_type, k, world, rank):
    """Whole dense rows [n, internal_k(k)] -> rank's slice [n, internal_k(k / world)]."""
    a = np.asarray(dense)
    kp = int(k) // int(world)
    lo, hi = rank * kp, (rank + 1) * kp
    if scoring_type in COMPLEX:
        return np.ascontiguousarray(np.concatenate([a[:, lo:hi], a[:, k + lo:k + hi]], axis=1))
    return np.ascontiguousarray(a[:, lo:hi])


def column_merge(slices, scoring_type):
    """The slices of all ranks (rank order) -> whole dense rows."""
    parts = [np.asarray(p) for p in slices]
    if scoring_type in COMPLEX:
        kp = parts[0].shape[1] // 2
        return np.concatenate([p[:, :kp] for p in parts] + [p[:, kp:] for p in parts], axis=1)
    return np.concatenate(parts, axis=1)


def check_columns(scoring_type, k, world, padded_k=None):
    if int(k) % int(world) != 0:
        raise ValueError(f"entity_sharding='columns' needs k ({k}) to be a multiple of the number of ranks ({world})")
    kp = int(k) // int(world)
    if (padded_k(kp) if padded_k else (kp + 3) // 4 * 4) > 256:
        raise ValueError("entity_sharding='columns': a rank's slice may hold up to 256 units per half (use more ranks, or rows / replicated tables)")
    return kp


class ColumnStepLoop:
    """The step loop of a rank that holds a column slice (engine: KgeEngine(scoring_type, k / W, N, R, k_full=k)).  Same interface as
    trainer.StepLoop (step / reset_loss / mean_batch_loss / kernel_hook), so fit() and bench.py drive either."""
    PHASES = ("partial scores", "score all-reduce", "loss + stage + tiles")

    def __init__(self, engine, eta, loss, optimizer, regularizer=None, seed=0, dist=None):
        self.engine = engine
        self.eta = int(eta)
        self.loss_ffi = loss.to_ffi()
        self.optimizer = optimizer
        self.reg = regularizer
        self.reg_rel = "same"
        self.seed = int(seed)
        self.dist = dist
        self.world = dist.get_world_size() if dist is not None else 1
        self.rank = dist.get_rank() if dist is not None else 0
        self.multi = dist is not None
        if getattr(optimizer, "lazy", False):
            raise ValueError("entity_sharding='columns' keeps the reference's dense optimizer (optimizer_mode='lazy' is not offered)")
        self.deterministic = False
        self.use_tiled = True
        self.pos_atomic = False
        self.merge, self.collectives, self.merge_report = "score all-reduce", None, None
        self.n_steps = 0
        self.kernel_hook = None
        engine.prepare_training(optimizer.name)
        if hasattr(optimizer, "bind"):
            optimizer.bind(engine)

    def step(self, global_batch, rng_step, focus=None):
        """global_batch: (Bg, 3) int32 device tensor, the WHOLE batch, the same on every rank."""
        if focus is not None:
            raise ValueError("entity_sharding='columns': FocusE is not offered")
        if self.deterministic:
            raise ValueError("entity_sharding='columns': deterministic mode is not offered")
        eng = self.engine
        bg = int(global_batch.shape[0])
        self.optimizer.iterations += 1
        opt_ffi = self.optimizer.to_ffi(self.optimizer.iterations, 2)
        lam = self.reg
        lam_r = self.reg if isinstance(self.reg_rel, str) else self.reg_rel
        hook = self.kernel_hook
        if hook is not None:
            hook(0)
        scores = eng.cols_partial_scores(global_batch, self.eta, self.seed, rng_step)
        if hook is not None:
            hook(1)
        if self.dist is not None:
            self.dist.all_reduce(scores)   # the ONE exchange of the step: B (1 + eta) floats
        if hook is not None:
            hook(2)
        eng.cols_loss(self.loss_ffi, scores, bg, self.eta)
        eng.train_step_tiled(global_batch, self.eta, self.loss_ffi, opt_ffi, self.seed, rng_step, reg_e=lam, reg_r=lam_r, given=scores)
        if hook is not None:
            hook(3)
        self.n_steps += 1

    def configure_for_data(self, triples, batch_size):
        return False   # (hot-row replicas / atomic positives belong to the row forms of the step)

    def tune_merge(self, *a, **k):
        return 0

    def sync_optimizer_slots(self):
        pass

    def reset_loss(self):
        self.engine.loss_acc.zero_()
        self.n_steps = 0

    def mean_batch_loss(self):
        """Data loss: every rank evaluated the same loss on the same complete scores (counted once); the regulariser is a sum over
        elements, i.e. over the ranks' slices."""
        acc = self.engine.loss_acc.clone()
        if self.dist is not None:
            reg = acc[1:2].clone()
            self.dist.all_reduce(reg)
            acc[1] = reg[0]
        return (float(acc[0].item()) + float(acc[1].item())) / max(1, self.n_steps)
