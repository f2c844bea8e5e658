"""Where ScoringBasedEmbeddingModel's tables live across the ranks of a torch.distributed run: one object per
`compile(entity_sharding=...)` mode, held by the model as `_placement`.  The model calls it without branching on the mode.

  Replicated  every rank holds the whole tables (data-parallel training, trainer.StepLoop).  A single-rank run always uses it.
  Rows        rank r holds rows [lo, hi) of the entity table with scratch rows behind them (sharded.py).
  Columns     rank r trains on a column slice of every row (colsharded.py) and also keeps the whole tables, which everything
              but the step reads; publish() refreshes them from the slices.

Rule: every method that runs a collective is called on every rank, at the same point, whatever each rank's own arguments
are.  The model calls them unconditionally; a decision that depends on one rank's arguments (Columns.begin_fit: has any
rank got callbacks?) is reduced over the ranks before it steers a collective.
"""
import numpy as np
import torch

from . import _ffi
from .colsharded import ColumnStepLoop, check_columns, column_merge, column_slice
from .engine import KgeEngine, subset_positions
from .sharded import RowExchange, ShardedStepLoop, ShardSpec, sharded_rank_counts
from .trainer import StepLoop, shard_bounds


_LISTS_NEED_WHOLE_TABLE = ("evaluate_candidates gathers each triple's candidate rows from the whole entity table on one GPU: row- and "
                           "column-sharded tables (entity_sharding) are out of its scope; evaluate(entities_subset=...) works there")


def shard_file(filepath, rank, world):
    return "{}.shard{:03d}-of-{:03d}.npz".format(filepath, rank, world)


class Replicated:
    """The whole tables on every rank; evaluate() on several ranks splits the queries."""

    lists_supported = True   # evaluate_candidates / evaluate_typed gather candidate rows from the whole table

    def __init__(self, m, dist, n_ents, n_rels, ent_rows, rel, batch_size=None):
        """ent_rows(lo, hi): dense rows [lo, hi) of the whole initial entity table; rel: the relation table."""
        self.m, self.dist, self.n_rels = m, dist, int(n_rels)
        self.lo, self.hi = 0, int(n_ents)
        self.engine = self._new_engine(n_ents)
        self._upload(ent_rows, rel)

    def _new_engine(self, rows):
        return KgeEngine(self.m.scoring_type, self.m.k, rows, self.n_rels, max_rel_size=self.n_rels)

    def _upload(self, ent_rows, rel):
        self.upload_rows(self.engine.ent, ent_rows)
        self.engine.pack(rel, out=self.engine.rel)

    def upload_rows(self, dst, rows, chunk_elems=1 << 24):
        """dst[0 : hi-lo] <- rows(lo, hi) (dense rows, packed into the engine's stored layout), in host chunks of
        <= chunk_elems floats (C5 shards do not fit host RAM twice)."""
        eng = self.engine
        step = max(1, chunk_elems // eng.K)
        for r0 in range(self.lo, self.hi, step):
            r1 = min(self.hi, r0 + step)
            blk = np.ascontiguousarray(rows(r0, r1), dtype=np.float32)
            if blk.shape != (r1 - r0, eng.K):
                raise ValueError(f"table rows have shape {blk.shape}, expected {(r1 - r0, eng.K)}")
            eng.pack(blk, out=dst[r0 - self.lo:r1 - self.lo])

    def ensure_capacity(self, batch_size):
        pass

    # ---- training
    def make_loop(self):
        m = self.m
        return self._configure(StepLoop(self.engine, m.eta, m.loss, m.optimizer, m._regularizers[0], m.seed, self.dist))

    def _configure(self, loop):
        loop.reg_rel = self.m._regularizers[1]   # the relation table's own regulariser (or None)
        if self.m._deterministic:
            loop.deterministic = True   # AMDKGE_TILED_DETERMINISTIC: bitwise reproducible tables (include/amdkge.h)
        return loop

    def begin_fit(self, has_callbacks):
        """fit() starts (collective); has_callbacks: whether THIS rank's fit() got callbacks."""

    def publish(self):
        """Make the tables predict / evaluate / checkpoints / callbacks read current with training (collective)."""

    def before_callbacks(self):
        """An epoch's callbacks are about to run on the ranks that have them (collective)."""

    def tables_written(self):
        """Someone outside the step loop wrote self.engine's tables (EarlyStopping restoring the best ones)."""

    # ---- reading tables
    def entity_table(self):
        """(N, Ks) entity table in the engine's STORED layout as a device tensor; engine.unpack() gives dense rows."""
        return self.engine.ent

    def localise(self, Xd):
        """int32 device triples (global ids) -> the same triples in this rank's row index space of self.engine."""
        return Xd

    def score(self, Xd):
        """Scores of the int32 device triples Xd (global ids) as a device tensor, the same on every rank."""
        return self.engine.score(Xd)

    def select(self, pick, cand, nq, k, largest=True):
        """Top k of nq queries over the candidate entities (int64 global ids, or None for all of them): pick(ent_ids, ent_hi, kk)
        runs the engine's selection over candidate rows of self.engine.  Returns (global ids int64 [nq, k], values [nq, k])."""
        ids = None if cand is None else torch.as_tensor(cand.astype(np.int32)).to(self.engine.device)
        pos, val = pick(ids, None, k)
        pos = pos.cpu().numpy().astype(np.int64)
        return (pos if cand is None else cand[pos]), val.cpu().numpy()

    def rank(self, Xi, sides, fi, subset, strategy):
        """int32 device ranks (n, len(sides)) of the test triples Xi (global ids); fi: FilterIndex or None; subset: global
        ids of entities_subset or None."""
        return self._over_ranks(Xi.shape[0], len(sides), lambda a, b: self._rank(Xi[a:b], sides, fi, subset, strategy))

    def _over_ranks(self, n, ncols, ranks_of):
        """ranks_of(a, b) -> int32 device ranks (b - a, ncols) of the test triples [a, b).  One rank computes them all; several
        ranks: every rank ranks its contiguous share of the test triples (the filters hold the whole data, so the ranks are
        those of the single-GPU run) and the shares are gathered."""
        d = self.dist
        if d is None or n < d.get_world_size():
            return ranks_of(0, n)
        W = d.get_world_size()
        bounds = [shard_bounds(n, W, q) for q in range(W)]
        lo, hi = bounds[d.get_rank()]
        buf = torch.zeros(-(-n // W), ncols, dtype=torch.int32, device=self.engine.device)
        buf[:hi - lo] = ranks_of(lo, hi)
        parts = [torch.empty_like(buf) for _ in range(W)]
        d.all_gather(parts, buf)
        return torch.cat([p[:b - a] for p, (a, b) in zip(parts, bounds)])

    def _rank(self, Xi, sides, fi, subset, strategy):
        eng = self.engine
        dev = eng.device
        ent_ids = subset_pos = None
        if subset is not None:
            sub = np.asarray(subset, dtype=np.int32)
            ent_ids, subset_pos = torch.as_tensor(sub).to(dev), subset_positions(sub, eng.n_ents, dev)
        n = Xi.shape[0]
        Xd = torch.as_tensor(Xi).to(dev)
        ranks = torch.empty(n, len(sides), dtype=torch.int32, device=dev)
        CH = 1 << 16
        for c0 in range(0, n, CH):
            xs = Xd[c0:c0 + CH]
            jobs = []
            for col, sd in enumerate(sides):
                flt = fi.device_filter(eng, xs, sd) if fi is not None else None   # range lookup on the device
                jobs.append((_ffi.SIDE_S if sd == "s" else _ffi.SIDE_O, flt, ranks[c0:c0 + CH, col], len(sides)))
            eng.rank_sides(xs, jobs, strategy, ent_ids, subset_pos)   # the sides run beside each other
        return ranks

    # ---- ranks against per-triple candidate lists (evaluate_candidates)
    LIST_CHUNK_BYTES = 256 << 20   # bound of the candidate ids of one side that are on the device at a time

    def rank_candidates(self, Xi, sides_with_lists, fi, strategy):
        """int32 device ranks (n, len(sides_with_lists)) of the test triples Xi (global ids), each against its own candidates:
        sides_with_lists = [(side "s" | "o", (offsets int64 [n + 1], ids int32, max_len)), ...] (evaluation.candidates.as_csr, host
        arrays of global ids); fi: FilterIndex or None.  Several ranks share the triples exactly as rank() does."""
        return self._over_ranks(Xi.shape[0], len(sides_with_lists), lambda a, b: self._rank_candidates(Xi, sides_with_lists, fi, strategy, a, b))

    def _rank_candidates(self, Xi, sides_with_lists, fi, strategy, a, b):
        """rank_candidates for the triples [a, b): chunks of at most 65 536 queries (as _rank) whose id lists stay under
        LIST_CHUNK_BYTES per side (a single longer list is a chunk of its own)."""
        eng = self.engine
        dev = eng.device
        Xd = torch.as_tensor(Xi[a:b]).to(dev)
        ranks = torch.empty(b - a, len(sides_with_lists), dtype=torch.int32, device=dev)
        CH, cap = 1 << 16, self.LIST_CHUNK_BYTES // 4
        c0 = a
        while c0 < b:
            c1 = min(b, c0 + CH)
            for _, (off, _, _) in sides_with_lists:
                c1 = min(c1, max(c0 + 1, int(np.searchsorted(off, off[c0] + cap, side="right")) - 1))
            xs = Xd[c0 - a:c1 - a]
            for col, (sd, (off, ids, _)) in enumerate(sides_with_lists):
                rel_off = off[c0:c1 + 1] - off[c0]
                lens = np.diff(rel_off)
                cand = (torch.as_tensor(rel_off[:-1].copy()).to(dev), torch.as_tensor(rel_off[1:].copy()).to(dev),
                        torch.as_tensor(ids[off[c0]:off[c1]]).to(dev), int(lens.max()) if lens.size else 0)
                flt = fi.device_filter(eng, xs, sd) if fi is not None else None   # range lookup on the device
                eng.rank_lists(xs, _ffi.SIDE_S if sd == "s" else _ffi.SIDE_O, cand, strategy, flt,
                               out=ranks[c0 - a:c1 - a, col], out_stride=len(sides_with_lists))
            c0 = c1
        return ranks

    # ---- ranks against the relation's domain / range set (evaluate_typed)
    def rank_typed(self, Xi, sides, types, fi, strategy, min_size):
        """int32 device ranks (n, len(sides)) of the test triples Xi (global ids), each against the set of its relation on that
        side: types = a datasets.types.BoundRelationTypes, whose range lookup runs on the device (a set smaller than min_size, or
        none: every entity).  Several ranks share the triples exactly as rank() does."""
        return self._over_ranks(Xi.shape[0], len(sides), lambda a, b: self._rank_typed(Xi[a:b], sides, types, fi, strategy, min_size))

    def _rank_typed(self, Xi, sides, types, fi, strategy, min_size):
        eng = self.engine
        Xd = torch.as_tensor(Xi).to(eng.device)
        n = Xi.shape[0]
        ranks = torch.empty(n, len(sides), dtype=torch.int32, device=eng.device)
        CH = 1 << 16
        for c0 in range(0, n, CH):
            xs = Xd[c0:c0 + CH]
            for col, sd in enumerate(sides):
                cand = (*types.ranges(xs, sd, min_size, "all"), types.max_len)
                flt = fi.device_filter(eng, xs, sd) if fi is not None else None
                eng.rank_lists(xs, _ffi.SIDE_S if sd == "s" else _ffi.SIDE_O, cand, strategy, flt, out=ranks[c0:c0 + CH, col], out_stride=len(sides))
        return ranks

    # ---- relation prediction: the relation table is whole in every placement, so every rank computes every query
    def _relation_chunks(self, Xd):
        """(c0, c1, the triples Xd[c0:c1] in self.engine's row index space) -- collective where localise() is."""
        yield 0, int(Xd.shape[0]), Xd

    def _relation_subset(self, cand):
        """candidate relation ids (or None) -> (rel_ids, subset_pos) device tensors; a repeated id keeps its last position"""
        if cand is None:
            return None, None
        eng = self.engine
        ids = np.asarray(cand, dtype=np.int32)
        return torch.as_tensor(ids).to(eng.device), subset_positions(ids, eng.n_rels, eng.device)

    def rank_relations(self, Xi, pfi, subset, strategy):
        """int32 device ranks (n,) of each test triple's relation among the candidate relations (all, or the ids `subset`), the
        same on every rank; pfi: PairFilterIndex or None."""
        eng = self.engine
        rel_ids, subset_pos = self._relation_subset(subset)
        Xd = torch.as_tensor(Xi).to(eng.device)
        ranks = torch.empty(int(Xd.shape[0]), dtype=torch.int32, device=eng.device)
        for c0, c1, xl in self._relation_chunks(Xd):
            flt = pfi.device_filter(eng, Xd[c0:c1]) if pfi is not None else None   # (on the GLOBAL ids)
            ranks[c0:c1] = eng.relation_rank(xl, strategy, flt, rel_ids, subset_pos)[0]
        return ranks

    def select_relations(self, Xd, k, cand, pfi):
        """The k best candidate relations of every (s, o) pair of the int32 device triples Xd (global ids): (positions int64
        [n, k] into `cand` / the relation table, -1 = missing; scores [n, k]) as numpy arrays, the same on every rank."""
        eng = self.engine
        rel_ids = self._relation_subset(cand)[0]
        n = int(Xd.shape[0])
        pos = torch.empty(n, int(k), dtype=torch.int32, device=eng.device)
        val = torch.empty(n, int(k), dtype=torch.float32, device=eng.device)
        for c0, c1, xl in self._relation_chunks(Xd):
            flt = pfi.device_filter(eng, Xd[c0:c1]) if pfi is not None else None
            pos[c0:c1], val[c0:c1] = eng.relation_topk(xl, k, rel_ids, flt)
        return pos.cpu().numpy().astype(np.int64), val.cpu().numpy()

    # ---- checkpoints
    def save(self, filepath, loop):
        """The arrays of <filepath>.npz on the rank that writes it, None on the others (collective).  Replicated tables:
        every rank holds the same bytes, rank 0 writes them."""
        if loop is not None and hasattr(loop, "sync_optimizer_slots"):
            loop.sync_optimizer_slots()   # data-parallel sharded merge: collective
        if self.dist is not None and self.dist.get_rank() != 0:
            return None
        eng = self.engine
        ent, rel = eng.get_tables()
        arrays = {"ent": ent, "rel": rel}
        for kname, t in getattr(eng, "slots", {}).items():
            arrays["slot_" + kname] = eng.unpack(t).cpu().numpy()
        return arrays


class Rows(Replicated):
    """The entity table row-sharded over the ranks (sharded.py); the relation table is replicated."""

    def __init__(self, m, dist, n_ents, n_rels, ent_rows, rel, batch_size=None):
        self.m, self.dist, self.n_rels = m, dist, int(n_rels)
        self.spec = sp = ShardSpec(n_ents, dist.get_world_size(), dist.get_rank())
        self.lo, self.hi = sp.lo, sp.hi   # same initial values as one GPU: rows [lo, hi) of the whole-table draw
        self._gathered = None             # entity_table()'s cache
        self.engine = self._new_engine(sp.n_local + self._scratch(batch_size or 1000))
        self._upload(ent_rows, rel)

    def _scratch(self, batch_size):
        """Scratch rows behind the shard: a training step's fetched rows, or two evaluation chunks' s / o rows."""
        sp = self.spec
        per_rank = -(-int(batch_size) // sp.world)
        return max(ShardedStepLoop.rows_needed(per_rank, self.m.eta, self.m._sharded_negatives, sp.world, sp.n_ents),
                   2 * self.m.EVAL_CHUNK_SHARDED)

    def ensure_capacity(self, batch_size):
        """Continued training: the scratch rows were sized for the first fit()'s batch (or for the default batch by
        load_weights); a larger batch gets a larger engine, tables and optimizer state carried over."""
        sp, old = self.spec, self.engine
        need = self._scratch(batch_size)
        if need <= int(old.ent.shape[0]) - sp.n_local:
            return
        new = self._new_engine(sp.n_local + need)
        new.ent[:sp.n_local].copy_(old.ent[:sp.n_local])
        new.rel.copy_(old.rel)
        self.engine, self._gathered = new, None
        self.m._loop = self.m._make_loop()   # allocates fresh slots on the new engine
        for name, t in getattr(old, "slots", {}).items():
            if name in new.slots:
                (new.slots[name][:sp.n_local] if name.endswith("_e") else new.slots[name]).copy_(
                    t[:sp.n_local] if name.endswith("_e") else t)

    def make_loop(self):
        m = self.m
        return self._configure(ShardedStepLoop(self.engine, self.spec, m.eta, m.loss, m.optimizer, m._regularizers[0], m.seed,
                                               self.dist, negatives=m._sharded_negatives))

    def begin_fit(self, has_callbacks):
        self._gathered = None

    def tables_written(self):
        self._gathered = None

    def entity_table(self):
        """Gathered once (collective) and cached until the next fit."""
        if self._gathered is None:
            sp, eng = self.spec, self.engine
            mine = torch.zeros(sp.rows_per, eng.Ks, dtype=eng.ent.dtype, device=eng.ent.device)
            mine[:sp.n_local] = eng.ent[:sp.n_local]
            parts = [torch.empty_like(mine) for _ in range(sp.world)]
            self.dist.all_gather(parts, mine)
            self._gathered = torch.cat(parts)[:sp.n_ents]
        return self._gathered

    def localise(self, Xd):
        """Fetches the remote s / o rows of Xd behind the shard (collective)."""
        sp = self.spec
        x = Xd.to(torch.int64)
        n = int(x.shape[0])
        ids = torch.cat([x[:, 0], x[:, 2]])
        remote = (ids < sp.lo) | (ids >= sp.hi)
        rid, rinv = torch.unique(ids[remote], return_inverse=True)
        ex = RowExchange(sp, self.dist, rid)
        ex.fetch(self.engine.ent, sp.n_local)
        loc = ids - sp.lo
        loc[remote] = sp.n_local + ex.slots()[rinv]
        return torch.stack([loc[:n], x[:, 1], loc[n:]], 1).to(torch.int32).contiguous()

    def score(self, Xd):
        CH = self.m.EVAL_CHUNK_SHARDED   # every rank fetches the rows it lacks and scores all triples
        outs = [self.engine.score(self.localise(Xd[c0:c0 + CH])) for c0 in range(0, int(Xd.shape[0]), CH)]
        return torch.cat(outs) if outs else torch.zeros(0, dtype=torch.float32, device=Xd.device)

    def _relation_chunks(self, Xd):
        CH = self.m.EVAL_CHUNK_SHARDED   # as score(): every rank fetches the s / o rows it lacks behind its shard, chunk by chunk
        for c0 in range(0, int(Xd.shape[0]), CH):
            c1 = min(int(Xd.shape[0]), c0 + CH)
            yield c0, c1, self.localise(Xd[c0:c1])

    def select(self, pick, cand, nq, k, largest=True):
        """Every rank selects among ITS rows, the W partial lists (global ids, values) are gathered and merged by a second
        selection (collective)."""
        sp, eng = self.spec, self.engine
        dev = eng.device
        if cand is None:
            loc, n_loc = None, sp.n_local
        else:
            loc = sp.local_subset(torch.as_tensor(cand).to(dev))[0]
            n_loc = int(loc.shape[0])
        gid = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
        gval = torch.full((nq, k), float("-inf") if largest else float("inf"), dtype=torch.float32, device=dev)
        if n_loc > 0:
            kk = min(k, n_loc)
            pos, val = pick(loc, n_loc, kk)
            rows = pos.to(torch.int64) if loc is None else loc[pos.to(torch.int64)].to(torch.int64)
            gid[:, :kk] = (rows + sp.lo).to(torch.int32)
            gval[:, :kk] = val
        parts_i = [torch.empty_like(gid) for _ in range(sp.world)]
        parts_v = [torch.empty_like(gval) for _ in range(sp.world)]
        self.dist.all_gather(parts_i, gid)
        self.dist.all_gather(parts_v, gval)
        ids, val = eng.topk_rows(torch.cat(parts_v, 1).contiguous(), k, largest=largest, payload=torch.cat(parts_i, 1).contiguous())
        return ids.cpu().numpy().astype(np.int64), val.cpu().numpy()

    def rank(self, Xi, sides, fi, subset, strategy):
        """Every rank counts against ITS rows, counts are summed over ranks (the reference's loop over entity partitions,
        :1431-1452, across GPUs); the same ranks on every rank."""
        eng = self.engine
        dev = eng.device
        if subset is not None:
            subset = self.spec.local_subset(torch.as_tensor(np.asarray(subset, dtype=np.int64)).to(dev))
        n = Xi.shape[0]
        ranks = torch.empty(n, len(sides), dtype=torch.int32, device=dev)
        CH = self.m.EVAL_CHUNK_SHARDED
        Xd = torch.as_tensor(Xi).to(dev)
        for c0 in range(0, n, CH):
            for col, sd in enumerate(sides):
                flt = fi.device_filter(eng, Xd[c0:c0 + CH], sd) if fi is not None else None
                counts, sub = sharded_rank_counts(eng, self.spec, self.dist, Xd[c0:c0 + CH],
                                                  _ffi.SIDE_S if sd == "s" else _ffi.SIDE_O, flt, subset)
                eng.compose_ranks(counts, sub, strategy, out=ranks[c0:c0 + CH, col], out_stride=len(sides))
        return ranks

    lists_supported = False

    def rank_candidates(self, Xi, sides_with_lists, fi, strategy):
        raise NotImplementedError(_LISTS_NEED_WHOLE_TABLE)

    def rank_typed(self, Xi, sides, types, fi, strategy, min_size):
        raise NotImplementedError(_LISTS_NEED_WHOLE_TABLE.replace("evaluate_candidates", "evaluate_typed"))

    def save(self, filepath, loop):
        """Rank r writes ITS rows of the entity table and of the optimizer slots to <filepath>.shardRRR-of-WWW.npz; rank 0
        gets the replicated part (relation table + slots, `shard_world`).  Nothing is gathered, so it works at C5 scale."""
        sp, eng = self.spec, self.engine
        dense = lambda t: eng.unpack(t).cpu().numpy()   # noqa: E731  checkpoints hold dense rows, whatever the engine stores
        mine = {"ent": dense(eng.ent[:sp.n_local]), "lo": np.int64(sp.lo), "hi": np.int64(sp.hi)}
        for kname, t in getattr(eng, "slots", {}).items():
            if kname.endswith("_e"):
                mine["slot_" + kname] = dense(t[:sp.n_local])
        np.savez(shard_file(filepath, sp.rank, sp.world), **mine)
        arrays = {"rel": dense(eng.rel), "shard_world": np.int64(sp.world), "n_ents": np.int64(sp.n_ents)}
        for kname, t in getattr(eng, "slots", {}).items():
            if kname.endswith("_r"):
                arrays["slot_" + kname] = dense(t)
        self.dist.barrier()   # every shard file is complete before rank 0 writes the file that names them
        return arrays if sp.rank == 0 else None


class Columns(Replicated):
    """Rank r trains on the column slice self.cols; self.engine keeps the whole tables (and their optimizer slots), which
    predict / evaluate / checkpoints / callbacks read.  They are refreshed from the slices through host numpy (all_gather +
    column merge) by publish()."""

    def __init__(self, m, dist, n_ents, n_rels, ent_rows, rel, batch_size=None):
        super().__init__(m, dist, n_ents, n_rels, ent_rows, rel)
        W = dist.get_world_size()
        check_columns(m.scoring_type, m.k, W, lambda kk: int(self.engine.lib.amdkge_padded_k(kk)))
        # the slice this rank trains on; filled from the whole tables (and optimizer slots) when fit() starts
        self.cols = KgeEngine(m.scoring_type, m.k // W, n_ents, n_rels, max_rel_size=n_rels, k_full=m.k)
        self.synced = None                # the optimizer's iteration count when the whole tables last matched the slices
        self.callbacks_anywhere = False

    def make_loop(self):
        m = self.m
        if m._deterministic:
            raise ValueError("entity_sharding='columns': deterministic mode is not offered")
        loop = ColumnStepLoop(self.cols, m.eta, m.loss, m.optimizer, m._regularizers[0], m.seed, self.dist)
        loop.reg_rel = m._regularizers[1]
        self.engine.prepare_training(m.optimizer.name)   # the whole tables' optimizer slots: what checkpoints hold
        self.optimizer = m.optimizer   # every step counts one iteration: publish() compares the count
        return loop

    def begin_fit(self, has_callbacks):
        """Whole tables (+ optimizer slots) -> this rank's slice (a fresh model, a checkpoint just loaded, or the tables the
        previous fit() or its callbacks left); then whether ANY rank has callbacks, which decides the per-epoch publish()."""
        if self.m.use_focusE:
            raise ValueError("entity_sharding='columns': FocusE is not offered")
        W, r, st, k = self.dist.get_world_size(), self.dist.get_rank(), self.m.scoring_type, self.m.k
        eng, col = self.engine, self.cols
        ent, rel = eng.get_tables()
        col.set_tables(column_slice(ent, st, k, W, r), column_slice(rel, st, k, W, r))
        for name, t in getattr(col, "slots", {}).items():
            if name in getattr(eng, "slots", {}):
                col.pack(column_slice(eng.unpack(eng.slots[name]).cpu().numpy(), st, k, W, r), out=t)
        self.synced = self.optimizer.iterations
        flag = torch.tensor([int(bool(has_callbacks))], dtype=torch.int32, device=col.device)   # (NCCL: a device tensor)
        self.dist.all_reduce(flag)
        self.callbacks_anywhere = int(flag.item()) > 0

    def publish(self):
        """The ranks' column slices (+ optimizer slots) -> the whole tables every rank keeps, if a step ran since they last
        matched: never over what a callback restored after the last step."""
        if self.optimizer.iterations == self.synced:
            return
        W, col, eng = self.dist.get_world_size(), self.cols, self.engine

        def gathered(stored):
            mine = col.unpack(stored).contiguous()
            parts = [torch.empty_like(mine) for _ in range(W)]
            self.dist.all_gather(parts, mine)
            return column_merge([p_.cpu().numpy() for p_ in parts], self.m.scoring_type)

        eng.set_tables(gathered(col.ent), gathered(col.rel))
        for name, t in getattr(col, "slots", {}).items():
            if name in getattr(eng, "slots", {}):
                eng.pack(gathered(t), out=eng.slots[name])
        self.synced = self.optimizer.iterations

    def before_callbacks(self):
        # callbacks read AND write the whole tables: they must see this epoch's.  Every rank publishes when any rank has
        # callbacks (publish() is a collective); callback-free fits skip the host round trip.
        if self.callbacks_anywhere:
            self.publish()

    lists_supported = False

    def rank_candidates(self, Xi, sides_with_lists, fi, strategy):
        raise NotImplementedError(_LISTS_NEED_WHOLE_TABLE)

    def rank_typed(self, Xi, sides, types, fi, strategy, min_size):
        raise NotImplementedError(_LISTS_NEED_WHOLE_TABLE.replace("evaluate_candidates", "evaluate_typed"))
