"""Thin Python layer over the C ABI: torch tensors supply device memory and the HIP stream
(plumbing only); every computation is a libamdkge entry point.

`KgeEngine` owns the HBM-resident state of one model replica on one GPU: the two embedding tables,
their dense gradient buffers and optimizer slots, and the scratch used by evaluation.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _ffi
from ._ffi import check


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def reg_fields(reg, default_p):
    """Regulariser argument of the engine's step / sweep calls -> (p1, lambda1, p2, lambda2) for the amdkge_opt descriptor.
    `reg`: None / a number (lambda of ONE LP term whose p the descriptor already carries: the form the kernel tests and
    older callers use) or an object with `.terms` = [(p, lambda), ...] (latent_features.regularizers.LPRegularizer: one
    term, or two for Keras' l1_l2)."""
    if reg is None:
        return int(default_p), 0.0, int(default_p), 0.0
    if isinstance(reg, (int, float)):
        return int(default_p), float(reg), int(default_p), 0.0
    if getattr(reg, "batch", False):
        raise NotImplementedError("a batch regularizer (BatchLPRegularizer) is no term of the optimizer sweep: it goes to "
                                  "KgeEngine.batch_reg_fwdbwd (trainer.StepLoop.step does); the session layer does not offer it")
    t = list(reg.terms)[:2]
    while len(t) < 2:
        t.append((int(default_p), 0.0))
    return int(t[0][0]), float(t[0][1]), int(t[1][0]), float(t[1][1])


def _same_reg(a, b, default_p):
    return reg_fields(a, default_p) == reg_fields(b, default_p)


def _set_reg(opt_desc, reg, default_p):
    opt_desc.reg_p, opt_desc.reg_lambda, opt_desc.reg2_p, opt_desc.reg2_lambda = reg_fields(reg, default_p)


def subset_positions(ids, n_rows, device):
    """Candidate subset (int array of row ids) -> int32 device tensor [n_rows]: a row's column in the subset, -1 = not a candidate.
    A repeated id keeps its LAST column (the reference's DenseHashTable.insert: last wins, :1639-1643)."""
    ids = np.asarray(ids)
    pos = np.full(int(n_rows), -1, dtype=np.int32)
    pos[ids] = np.arange(ids.shape[0], dtype=np.int32)
    return torch.as_tensor(pos).to(device)


class KgeEngine:
    def __init__(self, scoring_type, k, n_ents, n_rels, max_rel_size=None, device=None, pad=True, k_full=None):
        """k_full: this engine holds a COLUMN SLICE -- k of the k_full units of every row -- of a k_full-unit model (column-sharded
        tables, amdkge_cols_*; HolE's scale and RotatE's phase normaliser are then those of the whole model).
        pad=True (the product's setting): tables are STORED with each half padded to a multiple of 4 units
        (include/amdkge.h "STORED row layout"), which gives every k the 16-byte kernels; `ent`, `rel`, the gradient
        buffers and the optimizer slots then have `Ks` floats per row, of which the dense `K` are live.  pack() /
        unpack() convert; set_tables() / get_tables() speak the dense layout.  pad=False keeps dense rows (tests)."""
        if scoring_type not in _ffi.SCORING_TYPES:
            raise ValueError(f"unknown scoring_type {scoring_type!r}")
        self.lib = _ffi.lib()  # raises when the HIP library is absent: no fallback path exists
        if not torch.cuda.is_available():
            raise RuntimeError("ampligraph_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.scoring_type = scoring_type
        self.k = int(k)
        self.n_ents = int(n_ents)
        self.n_rels = int(n_rels)
        self.K = int(self.lib.amdkge_internal_k(_ffi.SCORING_TYPES[scoring_type], self.k))
        self.ks = int(self.lib.amdkge_padded_k(self.k)) if pad else self.k
        self.model = _ffi.Model(_ffi.SCORING_TYPES[scoring_type], self.k, self.n_ents, self.n_rels,
                                int(max_rel_size) if max_rel_size else 0, self.ks, int(k_full) if k_full else 0, 0)
        self.k_full = int(k_full) if k_full else self.k
        self.Ks = int(self.lib.amdkge_row_floats(C.byref(self.model)))
        # Both tables live in ONE flat allocation (entity rows first, relation rows on a 256-byte boundary behind them),
        # and so do their gradients and every optimizer slot: the multi-GPU step can then treat "all parameters" as one
        # vector (single all-reduce, or slice-wise reduce-scatter / sharded sweep / all-gather).
        ne, nr = self.n_ents * self.Ks, self.n_rels * self.Ks
        self._ne, self._nr = ne, nr
        self._off = (ne + 63) // 64 * 64
        self.p_flat = self._flat()
        self.ent = self.p_flat[:ne].view(self.n_ents, self.Ks)
        self.rel = self.p_flat[self._off:self._off + nr].view(self.n_rels, self.Ks)
        self.g_flat = None
        self.slot_flat = {}
        self.g_ent = None
        self.g_rel = None
        self.slots = {}
        self.opt_kind = None
        # [data loss, regulariser loss, second regulariser slot (row-sharded mode: relation-table part)]
        self.loss_acc = torch.zeros(3, dtype=torch.float64, device=self.device)
        self._work = None
        self._twork = None
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        """Reusable scratch tensor (grown on demand, never shrunk): the step loops allocate nothing per step."""
        n = 1
        for d_ in shape:
            n *= int(d_)
        t = self._bufs.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.empty(max(n, 1), dtype=dtype, device=self.device)
            self._bufs[name] = t
        return t[:n].view(*shape)

    def _flat(self, pad_to=64 * 16, fill=0.0):
        """Flat fp32 buffer [entity part | pad | relation part | pad]; total length a multiple of `pad_to` floats so that
        it splits evenly over up to 16 ranks in 256-byte-aligned slices."""
        n = (self._off + self._nr + pad_to - 1) // pad_to * pad_to
        return torch.full((n,), float(fill), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ tables
    def pack(self, dense, out=None):
        """dense rows [n, K] (device tensor or anything np.asarray takes) -> stored rows [n, Ks] (amdkge_pack_rows)."""
        if not torch.is_tensor(dense):
            dense = torch.as_tensor(np.ascontiguousarray(dense, dtype=np.float32))
        dense = dense.to(self.device, torch.float32).contiguous()
        if dense.ndim != 2 or int(dense.shape[1]) != self.K:
            raise ValueError(f"rows must have {self.K} floats, got shape {tuple(dense.shape)}")
        n = int(dense.shape[0])
        if out is None:
            out = torch.empty(n, self.Ks, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != (n, self.Ks) or not out.is_contiguous():
            raise ValueError("pack: output must be a contiguous [n, Ks] tensor")
        check(self.lib.amdkge_pack_rows(C.byref(self.model), _ptr(dense), n, _ptr(out), _stream()))
        return out

    def unpack(self, stored):
        """stored rows [n, Ks] (device tensor) -> dense rows [n, K] (amdkge_unpack_rows)."""
        stored = stored.contiguous()
        n = int(stored.shape[0])
        out = torch.empty(n, self.K, dtype=torch.float32, device=self.device)
        check(self.lib.amdkge_unpack_rows(C.byref(self.model), _ptr(stored), n, _ptr(out), _stream()))
        return out

    def set_tables(self, ent, rel):
        """Dense [n_ents, K] / [n_rels, K] tables (the reference's layout) -> HBM."""
        ent, rel = np.asarray(ent), np.asarray(rel)
        if tuple(ent.shape) != (self.n_ents, self.K) or tuple(rel.shape) != (self.n_rels, self.K):
            raise ValueError(f"table shapes must be {(self.n_ents, self.K)} and {(self.n_rels, self.K)}")
        self.pack(ent, out=self.ent)
        self.pack(rel, out=self.rel)

    def get_tables(self):
        return self.unpack(self.ent).cpu().numpy(), self.unpack(self.rel).cpu().numpy()

    # ------------------------------------------------------------------ training
    def prepare_training(self, optimizer="adam"):
        if optimizer not in _ffi.OPTIMIZERS:
            raise ValueError(f"unknown optimizer {optimizer!r}")
        self.opt_kind = optimizer
        ne, nr, off = self._ne, self._nr, self._off
        self.g_flat = self._flat()
        self.g_ent = self.g_flat[:ne].view_as(self.ent)
        self.g_rel = self.g_flat[off:off + nr].view_as(self.rel)
        self.slots, self.slot_flat = {}, {}
        for nme in _ffi.OPT_SLOTS[optimizer]:   # Keras legacy Adagrad initial_accumulator_value = 0.1
            fl = self._flat(fill=0.1 if nme == "a" else 0.0)
            self.slot_flat[nme] = fl
            self.slots[nme + "_e"] = fl[:ne].view_as(self.ent)
            self.slots[nme + "_r"] = fl[off:off + nr].view_as(self.rel)

    def grad_tensors(self):
        return [self.g_flat]

    def train_fwdbwd(self, triples, eta, loss, seed, step, sample_base=0, sample_range=None,
                     row_offset=0, b_global=0, neg_override=None, pos_scores=None, neg_scores=None):
        """triples: int32 cuda tensor (B,3).  Accumulates into g_ent/g_rel and loss_acc[0]."""
        B = int(triples.shape[0])
        if sample_range is None:
            sample_range = self.n_ents
        check(self.lib.amdkge_train_fwdbwd(
            C.byref(self.model), C.byref(loss), _ptr(self.ent), _ptr(self.rel), _ptr(triples), B, int(eta),
            int(sample_base), int(sample_range), int(seed), int(step), int(row_offset), int(b_global),
            _ptr(neg_override), _ptr(self.g_ent), _ptr(self.g_rel), C.c_void_p(self.loss_acc.data_ptr()),
            _ptr(pos_scores), _ptr(neg_scores), _stream()))

    def _slots_of(self, table):
        """(slot0, slot1) tensors of table "e" | "r" in the ABI's slot order (None where the optimizer has none)."""
        names = _ffi.OPT_SLOTS[self.opt_kind]
        got = [self.slots[f"{nme}_{table}"] for nme in names]
        return (got + [None, None])[:2]

    def tiled_supported(self, B, eta):
        """True when the owner-computes step (amdkge_train_step_tiled) covers this shape."""
        return int(self.lib.amdkge_train_tiled_workspace_bytes(C.byref(self.model), int(B), int(eta))) > 0

    def train_step_tiled(self, triples, eta, loss, opt_desc, seed, step, reg_e=0.0, reg_r=0.0, sample_base=0,
                         sample_range=None, row_offset=0, b_global=0, neg_override=None, pos_scores=None,
                         neg_scores=None, grad_only=False, pos_atomic=False, deterministic=False, given=None, det_wide=False):
        """Owner-computes step (kge_train_tiled.hip).  given: the coefficient buffer of the column-sharded step (cols_loss left
        dL/dscore in it: [B] positives then [eta][B] corruptions) -- AMDKGE_TILED_GIVEN_COEFFS, phase C of that step.  grad_only=False: the COMPLETE step -- entity table
        from the LDS tiles, relation table by the fused sweep; g_ent / g_rel (zero on entry) are left zero.
        grad_only=True (data-parallel): g_ent / g_rel (zero on entry) receive the gradients; nothing is updated.
        pos_atomic: skewed graphs, see AMDKGE_TILED_POS_ATOMIC in include/amdkge.h; deterministic: AMDKGE_TILED_DETERMINISTIC
        (bitwise reproducible tables: sorted tile accumulation, staged relation gradient; excludes pos_atomic)."""
        B = int(triples.shape[0])
        hot = getattr(self, "_hot_ids", None) is not None and not pos_atomic and not deterministic
        flags = ((_ffi.TILED_POS_ATOMIC if pos_atomic else 0) | (_ffi.TILED_DETERMINISTIC if deterministic else 0) | (_ffi.TILED_HOT_ROWS if hot else 0)
                 | (_ffi.TILED_DET_WIDE_SORT if deterministic and det_wide else 0))
        if given is not None:
            if pos_atomic or deterministic or int(given.numel()) != B * (1 + int(eta)) or given.dtype != torch.float32:
                raise ValueError("given: one float32 buffer of B (1 + eta) coefficients; excludes pos_atomic / deterministic")
            flags = _ffi.TILED_GIVEN_COEFFS
            pos_scores, neg_scores = given, given.view(-1)[B:]
        if getattr(self, "_twork_flags", flags) & _ffi.TILED_DETERMINISTIC != flags & _ffi.TILED_DETERMINISTIC:
            self._twork = None   # the two modes lay out the bookkeeping differently: a workspace serves one of them
        self._twork_flags = flags
        self._last_tiled = (B, int(eta), flags)
        need = int(self.lib.amdkge_train_tiled_workspace_bytes(C.byref(self.model), B, int(eta)))
        if need <= 0:
            raise ValueError("shape not supported by the owner-computes path")
        if self._twork is None or self._twork.numel() < need:
            # zero-filled once; the library keeps its bookkeeping region zero between steps
            self._twork = torch.zeros(need, dtype=torch.uint8, device=self.device)
            self._hot_applied = False
        if hot and not getattr(self, "_hot_applied", False):
            check(self.lib.amdkge_train_tiled_set_hot_rows(C.byref(self.model), _ptr(self._twork), _ptr(self._hot_ids),
                                                           int(self._hot_ids.shape[0]), _stream()))
            self._hot_applied = True
        if sample_range is None:
            sample_range = self.n_ents
        s0, s1 = self._slots_of("e")
        r0, r1 = self._slots_of("r")
        p0 = int(opt_desc.reg_p)   # the descriptor's own p: what a bare lambda refers to
        _set_reg(opt_desc, reg_e, p0)
        rp1, rl1, rp2, rl2 = reg_fields(reg_r, p0)
        if rl1 == 0.0 and rl2 != 0.0:
            rp1, rl1, rl2 = rp2, rl2, 0.0
        opt_desc.rel_reg_p, opt_desc.rel_reg2_p, opt_desc.rel_reg2_lambda = rp1, rp2, rl2
        opt_desc.row_floats = self.Ks
        try:
            check(self.lib.amdkge_train_step_tiled(
                C.byref(self.model), C.byref(loss), C.byref(opt_desc), _ptr(self.ent), _ptr(self.rel), _ptr(s0), _ptr(s1),
                _ptr(r0), _ptr(r1), float(rl1), _ptr(triples), B, int(eta), int(sample_base), int(sample_range),
                int(seed), int(step), int(row_offset), int(b_global), _ptr(neg_override),
                _ptr(self.g_ent), _ptr(self.g_rel), 0 if grad_only else 1, flags,
                C.c_void_p(self.loss_acc.data_ptr()), C.c_void_p(self.loss_acc.data_ptr() + 8),
                _ptr(pos_scores), _ptr(neg_scores), _ptr(self._twork), _stream()))
        except Exception:
            self._twork = None   # bookkeeping may be dirty after a failed launch: start from a fresh zeroed buffer
            raise
        finally:
            opt_desc.reg_p = p0

    # ------------------------------------------------------------------ column-sharded step (amdkge_cols_*, kge_train_cols.hip)
    def cols_partial_scores(self, triples, eta, seed, step, sample_base=0, sample_range=None, row_offset=0, b_global=0,
                            neg_override=None, out=None):
        """Phase A: this slice's partial score sums of B positives and their eta corruptions -> float32 [B (1 + eta)] (positives,
        then corruptions at j * B + i); the caller all-reduces it over the ranks."""
        B = int(triples.shape[0])
        if out is None:
            out = self._buf("cols_scores", (B * (1 + int(eta)),), torch.float32)
        check(self.lib.amdkge_cols_partial_scores(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples), B, int(eta), int(sample_base),
                                                  int(self.n_ents if sample_range is None else sample_range), int(seed), int(step), int(row_offset),
                                                  int(b_global), _ptr(neg_override), _ptr(out), _stream()))
        return out

    def cols_loss(self, loss, scores, B, eta):
        """Phase B: Loss.__call__ on the complete (summed) scores: loss_acc[0] += the data loss, scores <- dL/dscore in place."""
        check(self.lib.amdkge_cols_loss(C.byref(self.model), C.byref(loss), _ptr(scores), int(B), int(eta), C.c_void_p(self.loss_acc.data_ptr()), _stream()))
        return scores

    def set_hot_rows(self, ids):
        """Declare up to 64 hot entity rows (AMDKGE_TILED_HOT_ROWS: skewed graphs); None / empty switches the feature off."""
        if ids is None or len(ids) == 0:
            self._hot_ids = None
        else:
            self._hot_ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32)[:64]).to(self.device)
        self._hot_applied = False
        if self._hot_ids is None and self._twork is not None:   # clear a map an earlier fit left in the workspace
            check(self.lib.amdkge_train_tiled_set_hot_rows(C.byref(self.model), _ptr(self._twork), None, 0, _stream()))

    def tiled_status(self):
        """Sticky status of the owner-computes steps since the last query: 1 = a DETERMINISTIC step fell back to unsorted
        accumulation in some tile.  Only a deterministic step can set it, so only then is the stream synchronised to read it (the
        row-direct pass of long rows handles an overflowing LDS list by rescanning the spill: complete sums, no status)."""
        if self._twork is None or not hasattr(self, "_last_tiled") or not (self._last_tiled[2] & _ffi.TILED_DETERMINISTIC):
            return 0
        st = C.c_int32(0)
        B, eta, flags = self._last_tiled
        check(self.lib.amdkge_train_tiled_status(C.byref(self.model), B, eta, flags, _ptr(self._twork), C.byref(st), _stream()))
        return int(st.value)

    def opt_step(self, opt_desc, reg_e=0.0, reg_r=0.0, rows_e=None, reg_slots=(1, 1)):
        """Dense sweep over both tables (optimizer + regulariser + gradient reset).  rows_e limits the entity
        sweep to the first rows_e rows (row-sharded mode: the rows behind them are fetched copies of remote
        rows); reg_slots = loss_acc slots receiving the entity / relation regulariser values."""
        n_e = self.ent.numel() if rows_e is None else int(rows_e) * self.Ks
        opt_desc.row_floats = self.Ks
        p0 = int(opt_desc.reg_p)
        if rows_e is None and _same_reg(reg_e, reg_r, p0) and reg_slots[0] == reg_slots[1] and not opt_desc.lazy:
            # both tables in ONE launch: they live in one flat allocation (the padding between / behind them holds zero
            # parameters and zero gradients, which every rule maps to zero) -- one launch less on launch-bound shapes (C1)
            _set_reg(opt_desc, reg_e, p0)
            names = _ffi.OPT_SLOTS[self.opt_kind]
            sl = [self.slot_flat[n] for n in names] + [None, None]
            n_all = self._off + self._nr
            check(self.lib.amdkge_opt_step(C.byref(opt_desc), _ptr(self.p_flat), _ptr(self.g_flat), _ptr(sl[0]), _ptr(sl[1]), n_all,
                                           C.c_void_p(self.loss_acc.data_ptr() + 8 * int(reg_slots[0])), _stream()))
            opt_desc.reg_p = p0
            return
        for x, g, table, lam, n_el, slot in ((self.ent, self.g_ent, "e", reg_e, n_e, reg_slots[0]),
                                             (self.rel, self.g_rel, "r", reg_r, self.rel.numel(), reg_slots[1])):
            reg_ptr = C.c_void_p(self.loss_acc.data_ptr() + 8 * int(slot))
            _set_reg(opt_desc, lam, p0)
            s0, s1 = self._slots_of(table)
            check(self.lib.amdkge_opt_step(C.byref(opt_desc), _ptr(x), _ptr(g), _ptr(s0), _ptr(s1),
                                           n_el, reg_ptr, _stream()))
        opt_desc.reg_p = p0

    def step_rows(self, triples, ids):
        """amdkge_step_rows (include/ext/amdkge_sparse.h): the candidate rows of a step -- the ascending unique union of the s and o
        of the int32 device triples [B, 3] and the int32 device ids (any shape, contiguous; None: no list) -> (rows int32 [cap],
        n_rows int64 [1]), cap = min(2 B + ids.numel(), n_ents) being what the count can reach.  The count stays on the device.
        Both live in the engine's buffer cache (and so does the workspace): the next call overwrites them."""
        B, n_ids = int(triples.shape[0]), 0 if ids is None else int(ids.numel())
        if ids is not None and not ids.is_contiguous():
            raise ValueError("step_rows: the id tensor must be contiguous")
        cap = min(2 * B + n_ids, self.n_ents)
        rows = self._buf("step_rows", (cap,), torch.int32)
        n_rows = self._buf("step_n_rows", (1,), torch.int64)
        need = int(self.lib.amdkge_step_rows_workspace_bytes(self.n_ents, 2 * B + n_ids))
        if need < 0:
            raise ValueError("step_rows: batch and list too large for one call")
        work = self._buf("step_rows_work", (need,), torch.uint8)
        check(self.lib.amdkge_step_rows(self.n_ents, _ptr(triples), B, _ptr(ids), n_ids, _ptr(rows), cap, _ptr(n_rows), _ptr(work), _stream()))
        return rows, n_rows

    def opt_step_rows(self, opt_desc, reg_e, reg_r, rows, n_rows, cap, reg_slots=(1, 1)):
        """The sweep of the sparse optimizer mode: the entity table through amdkge_opt_step_rows on the listed rows (rows int32 [cap],
        strictly ascending in [0, n_rows[0]); n_rows int64 [1] on the device), then the relation table through the row-wise lazy
        sweep of amdkge_opt_step (the descriptor's lazy = 1 for that call, restored afterwards).  On a list that holds every entity
        row with a non-zero gradient the result is opt_step's with lazy = 1; nothing of size n_ents * Ks is walked."""
        opt_desc.row_floats = self.Ks
        p0, lazy0 = int(opt_desc.reg_p), int(opt_desc.lazy)
        _set_reg(opt_desc, reg_e, p0)
        s0, s1 = self._slots_of("e")
        check(self.lib.amdkge_opt_step_rows(C.byref(opt_desc), _ptr(self.ent), _ptr(self.g_ent), _ptr(s0), _ptr(s1), self.n_ents, _ptr(rows),
                                            _ptr(n_rows), int(cap), C.c_void_p(self.loss_acc.data_ptr() + 8 * int(reg_slots[0])), _stream()))
        _set_reg(opt_desc, reg_r, p0)
        opt_desc.lazy = 1
        s0, s1 = self._slots_of("r")
        check(self.lib.amdkge_opt_step(C.byref(opt_desc), _ptr(self.rel), _ptr(self.g_rel), _ptr(s0), _ptr(s1), self.rel.numel(),
                                       C.c_void_p(self.loss_acc.data_ptr() + 8 * int(reg_slots[1])), _stream()))
        opt_desc.lazy, opt_desc.reg_p = lazy0, p0

    def _flat_segments(self, lo, hi, reg_e, reg_r):
        """[lo, hi) of the flat parameter vector -> [(a, b, regulariser)]: its entity part and its relation part (the padding
        between / behind the tables holds zero parameters and zero gradients: nothing to sweep)"""
        parts = ((max(lo, 0), min(hi, self._ne), reg_e), (max(lo, self._off), min(hi, self._off + self._nr), reg_r))
        return [(a, b, lam) for a, b, lam in parts if b > a]

    def opt_step_flat(self, opt_desc, lo, hi, reg_e=0.0, reg_r=0.0, reg_slot=1):
        """Dense sweep over elements [lo, hi) of the flat parameter vector (sharded-optimizer data parallelism: a rank
        sweeps only its slice).  The slice may straddle the entity / relation boundary; the regulariser lambda follows."""
        segs = self._flat_segments(lo, hi, reg_e, reg_r)
        reg_ptr = C.c_void_p(self.loss_acc.data_ptr() + 8 * int(reg_slot))
        names = _ffi.OPT_SLOTS[self.opt_kind]
        if opt_desc.lazy:
            raise ValueError("the touched-rows optimizer mode sweeps whole rows: use the all-reduce gradient merge")
        p0 = int(opt_desc.reg_p)
        for a, b, lam in segs:
            _set_reg(opt_desc, lam, p0)
            sl = [self.slot_flat[n][a:b] for n in names] + [None, None]
            check(self.lib.amdkge_opt_step(C.byref(opt_desc), _ptr(self.p_flat[a:b]), _ptr(self.g_flat[a:b]), _ptr(sl[0]),
                                           _ptr(sl[1]), b - a, reg_ptr, _stream()))
        opt_desc.reg_p = p0

    # ------------------------------------------------------------------ multi-GPU data path (kge_shard.hip)
    def shard_route(self, spec, triples, negs, cap):
        """amdkge_shard_route: int32 device triples [b,3] (+ corruptions [nneg,3] or None) with GLOBAL ids -> the same in this
        rank's local index space, plus the per-peer request lists.  Returns (xl, nl, send_ids [world*cap], counts [world+1]);
        counts[world] is a sticky overflow flag (zeroed by zero_route_overflow)."""
        b = int(triples.shape[0])
        nneg = 0 if negs is None else int(negs.shape[0])
        xl = self._buf("route_xl", (b, 3), torch.int32)
        nl = self._buf("route_nl", (nneg, 3), torch.int32) if negs is not None else None
        send_ids = self._buf("route_send", (spec.world * int(cap),), torch.int32)
        counts = self._bufs.get("route_counts")
        if counts is None or counts.numel() != spec.world + 1:
            counts = self._bufs["route_counts"] = torch.zeros(spec.world + 1, dtype=torch.int32, device=self.device)
        need = int(self.lib.amdkge_shard_route_workspace_bytes(b, nneg))
        if need < 0:
            raise ValueError("batch too large for one shard_route call")
        work = self._buf("route_work", (need,), torch.uint8)
        check(self.lib.amdkge_shard_route(spec.n_ents, spec.world, spec.rank, _ptr(triples), b, _ptr(negs), nneg, int(cap),
                                          _ptr(xl), _ptr(nl), _ptr(send_ids), _ptr(counts), _ptr(work), _stream()))
        return xl, nl, send_ids, counts

    def zero_route_overflow(self):
        """Clear the sticky overflow flag of shard_route (counts[world]); stream-ordered."""
        counts = self._bufs.get("route_counts")
        if counts is not None:
            self.zero_(counts[-1:])

    def gather_rows(self, table, idx, name="gathered"):
        """rows table[idx] (idx < 0: zero rows) into a reusable [n, Ks] buffer (amdkge_gather_rows)."""
        n = int(idx.shape[0])
        out = self._buf(name, (n, int(table.shape[1])), torch.float32)
        check(self.lib.amdkge_gather_rows(_ptr(table), int(table.shape[1]), _ptr(idx), n, _ptr(out), _stream()))
        return out

    def scatter_add_rows(self, table, idx, src):
        """table[idx[j]] += src[j] (idx < 0 skipped) (amdkge_scatter_add_rows)."""
        check(self.lib.amdkge_scatter_add_rows(_ptr(table), int(table.shape[1]), _ptr(idx), int(idx.shape[0]), _ptr(src), _stream()))

    def zero_(self, t):
        """hipMemsetAsync on the launch stream (no torch op in the step loops)."""
        if t.numel():
            check(self.lib.amdkge_dev_memset(_ptr(t), 0, t.numel() * t.element_size(), _stream()))

    def opt_step_merged(self, opt_desc, lo, hi, parts, n_parts, part_stride, reg_e=0.0, reg_r=0.0, reg_slot=1):
        """Sharded-optimizer data parallelism: sweep elements [lo, hi) of the flat parameter vector with the gradient
        sum_q parts[q * part_stride + (i - lo)] (amdkge_opt_step_merged: the W partial slices are summed inside the sweep)."""
        segs = self._flat_segments(lo, hi, reg_e, reg_r)
        reg_ptr = C.c_void_p(self.loss_acc.data_ptr() + 8 * int(reg_slot))
        names = _ffi.OPT_SLOTS[self.opt_kind]
        p0 = int(opt_desc.reg_p)
        for a, b, lam in segs:
            _set_reg(opt_desc, lam, p0)
            sl = [self.slot_flat[n][a:b] for n in names] + [None, None]
            check(self.lib.amdkge_opt_step_merged(C.byref(opt_desc), _ptr(self.p_flat[a:b]), _ptr(parts[a - lo:]), int(n_parts),
                                                  int(part_stride), _ptr(sl[0]), _ptr(sl[1]), b - a, reg_ptr, _stream()))
        opt_desc.reg_p = p0

    def synth_triples(self, seed, first_row, n, n_ents, n_rels, out=None):
        """int32 [n,3] triples number first_row .. of the counter-based synthetic stream (amdkge_synth_triples)."""
        if out is None:
            out = torch.empty(int(n), 3, dtype=torch.int32, device=self.device)
        check(self.lib.amdkge_synth_triples(int(seed), int(first_row), int(n), int(n_ents), int(n_rels), _ptr(out), _stream()))
        return out

    def sample_corruptions(self, triples, eta, seed, step, sample_base=0, sample_range=None,
                           row_offset=0, b_global=0):
        B = int(triples.shape[0])
        out = torch.empty(B * eta, 3, dtype=torch.int32, device=self.device)
        check(self.lib.amdkge_sample_corruptions(
            _ptr(triples), B, int(eta), int(sample_base), int(sample_range or self.n_ents), int(seed),
            int(step), int(row_offset), int(b_global), _ptr(out), _stream()))
        return out

    def sample_negatives(self, triples, eta, seed, step, sample_base=0, sample_range=None, row_offset=0, b_global=0,
                         side="uniform", side_thr=None, pool=None, s_filter=None, o_filter=None, max_tries=8, stats=None):
        """amdkge_sample_negatives (include/amdkge_negatives.h has the draw): int32 [(B * eta), 3] corruptions of the int32 device
        triples [B, 3], row j * B + i -- the neg_override of train_fwdbwd / train_step_tiled / cols_partial_scores.  side: "uniform" |
        "bernoulli" (side_thr: uint32 thresholds per relation, held as an int32 tensor) | "s" | "o"; pool: int32 device ids the
        replacements come from (validated by the caller) or None; s_filter / o_filter: (lo, hi, ids) of the B positives, both or
        neither (FilterIndex.device_filter's form); stats: int64 [2] device tensor, += (redraws, exhausted).  The result lives in
        the engine's buffer cache: the next call overwrites it."""
        B = int(triples.shape[0])
        if (s_filter is None) != (o_filter is None):
            raise ValueError("sample_negatives: s_filter and o_filter are given together or not at all")
        out = self._buf("negatives", (B * int(eta), 3), torch.int32)
        sf, of = s_filter or (None, None, None), o_filter or (None, None, None)
        check(self.lib.amdkge_sample_negatives(
            _ptr(triples), B, int(eta), int(sample_base), int(sample_range or self.n_ents), int(seed), int(step), int(row_offset),
            int(b_global), _ffi.NEG_SIDE_MODES[side], _ptr(side_thr), _ptr(pool), 0 if pool is None else int(pool.numel()),
            _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(of[0]), _ptr(of[1]), _ptr(of[2]), int(max_tries), _ptr(stats), _ptr(out), _stream()))
        return out

    def sample_negatives_typed(self, triples, eta, seed, step, sample_base=0, sample_range=None, row_offset=0, b_global=0,
                               side="uniform", side_thr=None, pool=None, s_filter=None, o_filter=None, max_tries=8, stats=None,
                               s_cand=None, o_cand=None):
        """amdkge_sample_negatives_typed (include/amdkge_types.h has the draw): sample_negatives with every try's replacement taken from
        the positive's own candidate range -- s_cand / o_cand: (lo, hi, ids) of the B positives, both or neither (what
        relation_sets_ranges gives on a relation-set CSR); a positive whose range is empty is corrupted by sample_negatives' rule.
        stats: int64 [3] device tensor, += (redraws, exhausted, untyped).  The result shares sample_negatives' buffer."""
        B = int(triples.shape[0])
        if (s_filter is None) != (o_filter is None):
            raise ValueError("sample_negatives_typed: s_filter and o_filter are given together or not at all")
        if (s_cand is None) != (o_cand is None):
            raise ValueError("sample_negatives_typed: s_cand and o_cand are given together or not at all")
        out = self._buf("negatives", (B * int(eta), 3), torch.int32)
        none = (None, None, None)
        sf, of, sc, oc = s_filter or none, o_filter or none, s_cand or none, o_cand or none
        check(self.lib.amdkge_sample_negatives_typed(
            _ptr(triples), B, int(eta), int(sample_base), int(sample_range or self.n_ents), int(seed), int(step), int(row_offset),
            int(b_global), _ffi.NEG_SIDE_MODES[side], _ptr(side_thr), _ptr(pool), 0 if pool is None else int(pool.numel()),
            _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(of[0]), _ptr(of[1]), _ptr(of[2]), int(max_tries), _ptr(stats), _ptr(out),
            _ptr(sc[0]), _ptr(sc[1]), _ptr(sc[2]), _ptr(oc[0]), _ptr(oc[1]), _ptr(oc[2]), _stream()))
        return out

    def sample_shared(self, triples, group_size, num_negs, seed, step, sample_base=0, sample_range=None, side="uniform",
                      side_thr=None, pool=None):
        """amdkge_sample_shared (include/amdkge_shared.h has the draw): for the int32 device triples [B, 3] of a whole batch ->
        (ids int32 [ceil(B / group_size), num_negs], side int32 [B]; 1 = the subject is replaced).  Both live in the engine's
        buffer cache: the next call overwrites them."""
        B, G, M = int(triples.shape[0]), int(group_size), int(num_negs)
        n_groups = -(-B // min(G, B)) if B > 0 and G > 0 else 0
        ids = self._buf("shared_ids", (n_groups, M), torch.int32)
        sd = self._buf("shared_side", (B,), torch.int32)
        check(self.lib.amdkge_sample_shared(_ptr(triples), B, G, M, int(sample_base), int(sample_range or self.n_ents), int(seed), int(step),
                                            _ffi.NEG_SIDE_MODES[side], _ptr(side_thr), _ptr(pool), 0 if pool is None else int(pool.numel()),
                                            _ptr(ids), _ptr(sd), _stream()))
        return ids, sd

    def shared_supported(self, B, group_size, num_negs):
        """True when the shared-negative step (amdkge_train_shared_fwdbwd) covers this model and shape."""
        return int(self.lib.amdkge_train_shared_workspace_bytes(C.byref(self.model), int(B), int(group_size), int(num_negs))) > 0

    def _shared_step(self, fn, ws_fn, refusal, head, triples, group_size, num_negs, ids, side, pos_scores, neg_scores, *tail):
        """One shared-list train step, whichever entry point `fn` is: its family's workspace bytes (ws_fn) -> refuse a model /
        shape it does not cover -> the "shared_work" buffer -> the call.  head: the arguments between the model and the tables
        (the loss; label_smoothing and the reduction); tail: those between the workspace and the stream (_shared_lists, ...)."""
        B, G, M = int(triples.shape[0]), int(group_size), int(num_negs)
        need = int(ws_fn(C.byref(self.model), B, G, M)) if B > 0 else 0
        if B > 0 and need <= 0:
            raise ValueError(f"{refusal} for this model / shape ({self.scoring_type}, B={B}, group_size={G}, num_negs={M})")
        work = self._buf("shared_work", (need,), torch.uint8)
        check(fn(C.byref(self.model), *head, _ptr(self.ent), _ptr(self.rel), _ptr(triples), B, G, M, _ptr(ids), _ptr(side), _ptr(self.g_ent), _ptr(self.g_rel),
                 C.c_void_p(self.loss_acc.data_ptr()), _ptr(pos_scores), _ptr(neg_scores), _ptr(work), *tail, _stream()))

    @staticmethod
    def _shared_lists(s_filter, o_filter, identity):
        """the six range arrays ((lo, hi, ids) per side, or None) and the list mode, as the masked and labelled entry points take them"""
        sf, of = s_filter or (None, None, None), o_filter or (None, None, None)
        return (_ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(of[0]), _ptr(of[1]), _ptr(of[2]), _ffi.SHARED_LIST_MODES["identity" if identity else "given"])

    def train_shared_fwdbwd(self, triples, group_size, num_negs, ids, side, loss, pos_scores=None, neg_scores=None):
        """amdkge_train_shared_fwdbwd: the train step of train_fwdbwd with eta = num_negs on the corruptions 'positive i with its
        side[i] entity replaced by ids[i // group_size][j]', as matrix products.  Accumulates into g_ent / g_rel and loss_acc[0];
        neg_scores (optional) has row j * B + i."""
        self._shared_step(self.lib.amdkge_train_shared_fwdbwd, self.lib.amdkge_train_shared_workspace_bytes,
                          "train_shared_fwdbwd: shared negatives are not offered", (C.byref(loss),), triples, group_size, num_negs, ids, side,
                          pos_scores, neg_scores)

    @staticmethod
    def _score_window(who, scores, row0, side, group_size):
        """(rows, M, the group size clamped to the batch) of a score buffer [rows, M] whose row r is batch row row0 + r of side [B]"""
        rows, M = int(scores.shape[0]), int(scores.shape[1])
        B = int(side.shape[0])
        if int(row0) < 0 or int(row0) + rows > B or not scores.is_contiguous():
            raise ValueError(who + ": rows [row0, row0 + rows) must lie inside the batch and the buffer be contiguous")
        return rows, M, max(1, min(int(group_size), B)) if int(group_size) >= 1 else int(group_size)

    def shared_mask_scores(self, scores, row0, group_size, ids, side, s_filter, o_filter, identity=False, stats=None):
        """amdkge_shared_mask_scores (include/amdkge_shared_mask.h): the mask of the masked shared step alone, in place on the fp32
        device tensor scores [rows, M] whose row r is batch row row0 + r.  side int32 [B]; ids int32 [ceil(B / group_size), M] (may
        be None with identity=True, the promise that ids[g][j] == j); s_filter / o_filter: (lo, hi, ids) of the B positives
        (FilterIndex.device_filter's form); stats: int64 [2] device tensor, += (masked, unmaskable)."""
        rows, M, G = self._score_window("shared_mask_scores", scores, row0, side, group_size)
        check(self.lib.amdkge_shared_mask_scores(
            _ptr(scores), int(row0), rows, G, M, _ptr(ids), _ptr(side), _ptr(s_filter[0]), _ptr(s_filter[1]), _ptr(s_filter[2]),
            _ptr(o_filter[0]), _ptr(o_filter[1]), _ptr(o_filter[2]), _ffi.SHARED_LIST_MODES["identity" if identity else "given"], _ptr(stats), _stream()))
        return scores

    def train_shared_masked_fwdbwd(self, triples, group_size, num_negs, ids, side, loss, s_filter=None, o_filter=None, identity=False, stats=None,
                                   pos_scores=None, neg_scores=None):
        """amdkge_train_shared_masked_fwdbwd: train_shared_fwdbwd in which the score of a corruption whose replacement is in the
        positive's known range -- s_filter / o_filter: (lo, hi, ids) of the B positives, both or neither -- is -inf before the loss;
        a positive whose whole list is known keeps its row.  identity: the promise that ids[g][j] == j (the all-entities list);
        stats: int64 [2] device tensor, += (masked, unmaskable).  Without the filters it is train_shared_fwdbwd."""
        if (s_filter is None) != (o_filter is None):
            raise ValueError("train_shared_masked_fwdbwd: s_filter and o_filter are given together or not at all")
        self._shared_step(self.lib.amdkge_train_shared_masked_fwdbwd, self.lib.amdkge_train_shared_workspace_bytes,
                          "train_shared_masked_fwdbwd: shared negatives are not offered", (C.byref(loss),), triples, group_size, num_negs, ids, side,
                          pos_scores, neg_scores, *self._shared_lists(s_filter, o_filter, identity), _ptr(stats))

    def shared_dist_supported(self, B, group_size, num_negs):
        """True when the distance-tile shared step (amdkge_train_shared_dist_fwdbwd: TransE, RotatE) covers this model and shape."""
        return int(self.lib.amdkge_train_shared_dist_workspace_bytes(C.byref(self.model), int(B), int(group_size), int(num_negs))) > 0

    def train_shared_dist_fwdbwd(self, triples, group_size, num_negs, ids, side, loss, s_filter=None, o_filter=None, identity=False, stats=None,
                                 pos_scores=None, neg_scores=None):
        """amdkge_train_shared_dist_fwdbwd (include/amdkge_shared_dist.h): train_shared_masked_fwdbwd's step for TransE and RotatE, whose
        G x M scores of a group are a tile of distances instead of a matrix product.  The arguments are that method's: s_filter /
        o_filter (both or neither) mask the known statements, identity promises ids[g][j] == j, stats int64 [2] += (masked,
        unmaskable).  Accumulates into g_ent / g_rel and loss_acc[0]; neg_scores (optional) has row j * B + i."""
        if (s_filter is None) != (o_filter is None):
            raise ValueError("train_shared_dist_fwdbwd: s_filter and o_filter are given together or not at all")
        self._shared_step(self.lib.amdkge_train_shared_dist_fwdbwd, self.lib.amdkge_train_shared_dist_workspace_bytes,
                          "train_shared_dist_fwdbwd: distance-tile shared negatives are not offered", (C.byref(loss),), triples, group_size, num_negs, ids,
                          side, pos_scores, neg_scores, *self._shared_lists(s_filter, o_filter, identity), _ptr(stats))

    def shared_label_loss(self, scores, row0, group_size, ids, side, s_filter, o_filter, label_smoothing=0.0, reduction="sum", scale=1.0,
                          weights=None, identity=False, loss_sum=None, stats=None):
        """amdkge_shared_label_loss (include/amdkge_shared_labels.h): the loss step of the labelled (KvsAll) shared step alone, in
        place on the fp32 device tensor scores [rows, M] whose row r is batch row row0 + r: scores in, scale * dL/dscore out.  An
        entry is labelled 1 when its id is in the row's known range -- s_filter / o_filter: (lo, hi, ids) of the B batch rows
        (FilterIndex.device_filter's form) --, the loss is binary cross-entropy with logits on scale * score.  side int32 [B]; ids
        int32 [ceil(B / group_size), M] (may be None with identity=True, the promise that ids[g][j] == j); weights: None or (w_s,
        w_o) fp32 [B] device tensors; loss_sum: float64 [1] device tensor, += the rows' losses (default: loss_acc[0]); stats: int64
        [2] device tensor, += (labelled, unlabelled_rows)."""
        rows, M, G = self._score_window("shared_label_loss", scores, row0, side, group_size)
        ws, wo = weights if weights is not None else (None, None)
        acc = self.loss_acc if loss_sum is None else loss_sum
        check(self.lib.amdkge_shared_label_loss(
            _ptr(scores), int(row0), rows, G, M, _ptr(ids), _ptr(side), _ptr(s_filter[0]), _ptr(s_filter[1]), _ptr(s_filter[2]),
            _ptr(o_filter[0]), _ptr(o_filter[1]), _ptr(o_filter[2]), _ffi.SHARED_LIST_MODES["identity" if identity else "given"],
            float(label_smoothing), 1 if reduction == "mean" else 0, float(scale), _ptr(ws), _ptr(wo), C.c_void_p(acc.data_ptr()), _ptr(stats), _stream()))
        return scores

    def _train_shared_labels(self, fn, ws_fn, who, triples, group_size, num_negs, ids, side, s_filter, o_filter, label_smoothing, reduction, weights,
                             identity, stats, pos_scores, neg_scores):
        if s_filter is None or o_filter is None:
            raise ValueError(who + ": s_filter and o_filter are both required (the labels are the known ranges)")
        ws, wo = weights if weights is not None else (None, None)
        self._shared_step(fn, ws_fn, who + ": the labelled shared step is not offered", (float(label_smoothing), 1 if reduction == "mean" else 0), triples,
                          group_size, num_negs, ids, side, pos_scores, neg_scores, *self._shared_lists(s_filter, o_filter, identity), _ptr(ws), _ptr(wo),
                          _ptr(stats))

    def train_shared_labels_fwdbwd(self, triples, group_size, num_negs, ids, side, s_filter, o_filter, label_smoothing=0.0, reduction="sum",
                                   weights=None, identity=False, stats=None, pos_scores=None, neg_scores=None):
        """amdkge_train_shared_labels_fwdbwd (include/amdkge_shared_labels.h): the KvsAll step of DistMult / ComplEx / HolE -- the
        shared step in which every row is a query, every entry of its list a binary classification labelled 1 when its id is in the
        row's known range (s_filter / o_filter: (lo, hi, ids) of the B positives, both required), and the loss binary
        cross-entropy with logits, label_smoothing in [0, 1), reduction "sum" | "mean" (over the list).  weights: None or (w_s,
        w_o) fp32 [B] row weights by replaced side; identity: the promise that ids[g][j] == j (the all-entities list); stats: int64
        [2] device tensor, += (labelled, unlabelled_rows).  Accumulates into g_ent / g_rel and loss_acc[0]; neg_scores
        (optional) has row j * B + i and shows the plain scores."""
        self._train_shared_labels(self.lib.amdkge_train_shared_labels_fwdbwd, self.lib.amdkge_train_shared_workspace_bytes, "train_shared_labels_fwdbwd",
                                  triples, group_size, num_negs, ids, side, s_filter, o_filter, label_smoothing, reduction, weights, identity, stats,
                                  pos_scores, neg_scores)

    def train_shared_dist_labels_fwdbwd(self, triples, group_size, num_negs, ids, side, s_filter, o_filter, label_smoothing=0.0, reduction="sum",
                                        weights=None, identity=False, stats=None, pos_scores=None, neg_scores=None):
        """amdkge_train_shared_dist_labels_fwdbwd: train_shared_labels_fwdbwd's step for TransE and RotatE, on the distance tiles of
        train_shared_dist_fwdbwd.  The arguments are that method's."""
        self._train_shared_labels(self.lib.amdkge_train_shared_dist_labels_fwdbwd, self.lib.amdkge_train_shared_dist_workspace_bytes,
                                  "train_shared_dist_labels_fwdbwd", triples, group_size, num_negs, ids, side, s_filter, o_filter, label_smoothing,
                                  reduction, weights, identity, stats, pos_scores, neg_scores)

    def batch_reg_fwdbwd(self, triples, reg_e=None, reg_r=None):
        """amdkge_batch_reg_fwdbwd (include/amdkge_batch_reg.h): the batch regularisers reg_e / reg_r (BatchLPRegularizer or None:
        that term is off) on the rows of the int32 device positives [B, 3], once per occurrence.  Runs between a forward / backward
        call that leaves dense gradients and opt_step: the gradient is ADDED to g_ent / g_rel, the penalty to loss_acc[1], the slot
        the whole-table regulariser's value uses."""
        terms = []
        for reg, table in ((reg_e, "ent"), (reg_r, "rel")):
            if reg is None:
                terms += [2, 0.0, _ffi.BATCH_REG_NORMS["float"]]
            else:
                terms += [int(reg.p), float(reg.lam), _ffi.BATCH_REG_NORMS[reg.norm_for(self.scoring_type, table)]]
        check(self.lib.amdkge_batch_reg_fwdbwd(
            C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples), int(triples.shape[0]), *terms,
            _ptr(self.g_ent), _ptr(self.g_rel), C.c_void_p(self.loss_acc.data_ptr() + 8), _stream()))

    def train_relation_fwdbwd(self, triples, loss, weight, flt=None, stats=None, pos_scores=None, rel_scores=None):
        """amdkge_train_relation_fwdbwd (include/amdkge_relation_objective.h): the relation-prediction term on the int32 device
        positives [B, 3] -- the train step of train_fwdbwd with eta = n_rels on the rows (s_i, j, o_i), j = 0 .. n_rels - 1, as matrix
        products over the relation table, times `weight`.  flt: None (nothing is masked) or (lo, hi, ids), each positive's range of
        known relation ids (PairFilterIndex.device_filter's form): those scores are -inf before the loss, a positive whose every
        relation is known keeps its row; stats: int64 [2] device tensor, += (masked, unmaskable).  Runs between a forward / backward
        call that leaves dense gradients and opt_step: accumulates into g_ent / g_rel and weight * loss into loss_acc[0];
        rel_scores (optional, [n_rels * B]) has row j * B + i."""
        B = int(triples.shape[0])
        need = int(self.lib.amdkge_train_relation_workspace_bytes(C.byref(self.model), B)) if B > 0 else 0
        if B > 0 and need <= 0:
            raise ValueError(f"train_relation_fwdbwd: the relation objective is not offered for this model / shape ({self.scoring_type}, B={B})")
        work = self._buf("relation_work", (need,), torch.uint8)
        lo, hi, ids = flt if flt is not None else (None, None, None)
        check(self.lib.amdkge_train_relation_fwdbwd(
            C.byref(self.model), C.byref(loss), float(weight), _ptr(self.ent), _ptr(self.rel), _ptr(triples), B, _ptr(lo), _ptr(hi), _ptr(ids),
            _ptr(self.g_ent), _ptr(self.g_rel), C.c_void_p(self.loss_acc.data_ptr()), _ptr(pos_scores), _ptr(rel_scores), _ptr(work), _ptr(stats),
            _stream()))

    def negatives_side_thresholds(self, po_keys, sp_keys, n_ents=None, n_rels=None):
        """amdkge_negatives_side_thresholds: the Bernoulli thresholds floor(2^32 G_po / (G_sp + G_po)) per relation from a
        FilterIndex's two int64 device key arrays -> int32 device tensor [n_rels] holding the uint32 bit patterns."""
        n_rels = self.n_rels if n_rels is None else int(n_rels)
        thr = torch.empty(n_rels, dtype=torch.int32, device=self.device)
        check(self.lib.amdkge_negatives_side_thresholds(_ptr(po_keys), int(po_keys.numel()), _ptr(sp_keys), int(sp_keys.numel()),
                                                        int(self.n_ents if n_ents is None else n_ents), n_rels, _ptr(thr), _stream()))
        return thr

    def _filter_build(self, triples, side, n_ents, n_rels, name=None):
        """One CSR filter index from the concatenated id triples (int32 [m,3] device tensor) -> (keys int64 [n_groups], start
        int64 [n_groups + 1], ids int32 [n_unique]) device tensors.  side "s" | "o": amdkge_filter_build (or, with
        name="relation_sets_build", the relation sets of include/amdkge_types.h: the same protocol); None: the (s, o) pair
        form, amdkge_pair_filter_build.  One stream synchronisation (the two counts come back to size the views); an index is
        built once per evaluate() and cached."""
        name = name or ("filter_build" if side is not None else "pair_filter_build")
        m = int(triples.shape[0])
        keys = torch.empty(max(m, 1), dtype=torch.int64, device=self.device)
        start = torch.empty(m + 1, dtype=torch.int64, device=self.device)
        ids = torch.empty(max(m, 1), dtype=torch.int32, device=self.device)
        counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        need = int(self.lib.amdkge_filter_build_workspace_bytes(m, int(n_ents), int(n_rels)))
        if need < 0:
            raise ValueError(name + ": bad sizes")
        work = self._buf("filter_build_work", (need,), torch.uint8)
        form = () if side is None else (_ffi.SIDE_S if side == "s" else _ffi.SIDE_O,)
        check(getattr(self.lib, "amdkge_" + name)(_ptr(triples), m, *form, int(n_ents), int(n_rels), _ptr(keys), _ptr(start), _ptr(ids),
                                                  _ptr(counts), _ptr(work), _stream()))
        ng, nu = (int(c) for c in counts.tolist())
        return keys[:ng], start[:ng + 1], ids[:nu]

    def _filter_ranges(self, keys, start, triples, side, n_ents, n_rels=None):
        """(lo, hi) int64 device tensors: each triple's range in the id array of a filter index.  side 1 | 2 (subject / object):
        amdkge_filter_ranges; None: the (s, o) pair form, amdkge_pair_filter_ranges."""
        n = int(triples.shape[0])
        lo = torch.empty(n, dtype=torch.int64, device=self.device)
        hi = torch.empty(n, dtype=torch.int64, device=self.device)
        head, tail = (_ptr(keys), _ptr(start), int(keys.shape[0]), _ptr(triples), n), (_ptr(lo), _ptr(hi), _stream())
        if side is None:
            check(self.lib.amdkge_pair_filter_ranges(*head, int(n_ents), *tail))
        else:
            check(self.lib.amdkge_filter_ranges(*head, int(side), int(n_ents), int(n_rels), *tail))
        return lo, hi

    def filter_build(self, triples, side, n_ents, n_rels):
        """amdkge_filter_build: the CSR filter index of one side ("s" | "o"), see _filter_build."""
        return self._filter_build(triples, "s" if side == "s" else "o", n_ents, n_rels)

    def filter_ranges(self, keys, start, triples, side, n_ents, n_rels):
        """(lo, hi) int64 device tensors: each triple's range in a FilterIndex id array (amdkge_filter_ranges; side 1 | 2)."""
        return self._filter_ranges(keys, start, triples, side, n_ents, n_rels)

    def relation_sets_build(self, triples, side, n_ents, n_rels):
        """amdkge_relation_sets_build: the CSR of the distinct subjects (side "s": the domains) or objects ("o": the ranges) per
        relation of the int32 device triples -> (keys, start, ids), see _filter_build."""
        return self._filter_build(triples, "s" if side == "s" else "o", n_ents, n_rels, name="relation_sets_build")

    def relation_sets_ranges(self, keys, start, triples, min_size=0, fallback=(0, 0)):
        """(lo, hi) int64 device tensors: the range of each triple's RELATION in the id array of a relation-set CSR; `fallback`
        = (lo, hi) for a relation that is absent or whose set has fewer than min_size ids (amdkge_relation_sets_ranges)."""
        n = int(triples.shape[0])
        lo = torch.empty(n, dtype=torch.int64, device=self.device)
        hi = torch.empty(n, dtype=torch.int64, device=self.device)
        check(self.lib.amdkge_relation_sets_ranges(_ptr(keys), _ptr(start), int(keys.shape[0]), _ptr(triples), n, int(min_size),
                                                   int(fallback[0]), int(fallback[1]), _ptr(lo), _ptr(hi), _stream()))
        return lo, hi

    def compose_ranks(self, counts, sub, strategy, out=None, out_stride=1):
        """(greater, equal) counts [+ filter subtraction] -> 1-based ranks (amdkge_rank_compose)."""
        n = int(counts.shape[0])
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
            out_stride = 1
        check(self.lib.amdkge_rank_compose(_ptr(counts), _ptr(sub), n, _ffi.RANK_STRATEGY[strategy], _ptr(out),
                                           int(out_stride), _stream()))
        return out

    # ------------------------------------------------------------------ predict
    def score(self, triples):
        n = int(triples.shape[0])
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        check(self.lib.amdkge_score(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples), n,
                                    _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ discovery (kge_discovery.hip, kge_rank_tile.hip, kge_rank.hip)
    SCORE_CHUNK_BYTES = 256 << 20   # bound of the transient (queries x candidates) score block

    def _score_chunks(self, n, m):
        """Query ranges [(c0, c1), ...] whose (queries x m candidates) fp32 score block stays under SCORE_CHUNK_BYTES."""
        rows = max(1, min(n, self.SCORE_CHUNK_BYTES // max(4 * m, 1)))
        return [(c0, min(n, c0 + rows)) for c0 in range(0, n, rows)]

    def _corruption_blocks(self, triples, side, ent_ids, ent_lo, ent_hi):
        """(c0, c1, block) per chunk of the query triples: block = the 1-vs-all scores fp32 [c1 - c0, ent_hi - ent_lo] of one
        corruption side (amdkge_corruption_scores) in the reused "disc_scores" buffer -- valid until the next chunk."""
        m = int(ent_hi) - int(ent_lo)
        for c0, c1 in self._score_chunks(int(triples.shape[0]), m):
            blk = self._buf("disc_scores", (c1 - c0, m), torch.float32)
            work = self._workspace(c1 - c0)
            check(self.lib.amdkge_corruption_scores(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples[c0:c1]), c1 - c0, int(side),
                                                    _ptr(ent_ids), int(ent_lo), int(ent_hi), _ptr(blk), m, _ptr(work), _stream()))
            yield c0, c1, blk

    def _relation_blocks(self, triples, rel_ids, m):
        """(c0, c1, block) per chunk of the query triples: block = relation_scores fp32 [c1 - c0, m] of the m candidate relations
        (all, or rel_ids) in the reused "rel_scores" buffer -- valid until the next chunk."""
        for c0, c1 in self._score_chunks(int(triples.shape[0]), m):
            blk = self._buf("rel_scores", (c1 - c0, m), torch.float32)
            self._relation_block(triples[c0:c1], rel_ids, 0, m, blk, m)
            yield c0, c1, blk

    @staticmethod
    def _flt_chunk(flt, c0, c1):
        """the filter (lo, hi, ids) of queries [c0, c1); the id array is shared"""
        return None if flt is None else (flt[0][c0:c1], flt[1][c0:c1], flt[2])

    def _idx_val(self, n, k):
        """the (idx int32 [n,k], val fp32 [n,k]) output pair of a selection"""
        return (torch.empty(n, int(k), dtype=torch.int32, device=self.device), torch.empty(n, int(k), dtype=torch.float32, device=self.device))

    def topk_rows(self, vals, k, largest=True, col_scale=None, col_bias=None, payload=None):
        """(idx int32 [n,k], val fp32 [n,k]) of the k best entries per row of vals [n,m] (amdkge_topk_rows); with `payload`
        (int32, same shape and row stride as vals) idx holds the payload entries of the selected columns."""
        n, m = int(vals.shape[0]), int(vals.shape[1])
        if int(k) > 1024:
            # beyond the streaming selection's k: a full stable sort of the (scaled) row on the device, which is what the
            # reference does for every top_n (argsort over all candidates, discovery.py:1150-1160); same order rule as the
            # kernel (best first, equal values by increasing column), missing entries (m < k) as index -1 / -inf
            v = vals.to(torch.float32)
            if col_scale is not None:
                v = v * col_scale[None, :m]
            if col_bias is not None:
                v = v + col_bias[None, :m]
            v = torch.nan_to_num(v, nan=float("-inf") if largest else float("inf"), posinf=float("inf"), neginf=float("-inf"))   # NaN ranks last, as in the kernel
            sv, si = torch.sort(v, dim=1, descending=bool(largest), stable=True)
            kk = min(int(k), m)
            idx = torch.full((n, int(k)), -1, dtype=torch.int32, device=self.device)
            val = torch.full((n, int(k)), float("-inf") if largest else float("inf"), dtype=torch.float32, device=self.device)
            sel = si[:, :kk]
            idx[:, :kk] = (sel if payload is None else torch.gather(payload[:, :m].to(torch.int64), 1, sel)).to(torch.int32)
            val[:, :kk] = sv[:, :kk]
            return idx, val
        idx, val = self._idx_val(n, k)
        check(self.lib.amdkge_topk_rows(_ptr(vals), n, m, int(vals.stride(0)), _ptr(col_scale), _ptr(col_bias), _ptr(payload), int(k), 1 if largest else 0,
                                        _ptr(idx), _ptr(val), _stream()))
        return idx, val

    def topk_rows_excluding(self, vals, k, col_ids=None, id_base=0, flt=None, own=None):
        """(idx int32 [n,k], val fp32 [n,k]) of the k largest entries per row of vals [n,m] among the columns whose entity id
        (col_ids[j], or id_base + j) is neither in the row's range of flt = (lo, hi, ids) nor equal to own[row]
        (amdkge_topk_rows_excluding; 1 <= k <= 1024).  Same order and missing-entry convention as topk_rows."""
        n, m = int(vals.shape[0]), int(vals.shape[1])
        lo, hi, ids = flt if flt is not None else (None, None, None)
        idx, val = self._idx_val(n, k)
        check(self.lib.amdkge_topk_rows_excluding(_ptr(vals), n, m, int(vals.stride(0)) if n else m, _ptr(col_ids), int(id_base), _ptr(lo), _ptr(hi),
                                                  _ptr(ids), _ptr(own), int(k), _ptr(idx), _ptr(val), _stream()))
        return idx, val

    def corruption_topk(self, triples, side, k, ent_ids=None, ent_lo=0, ent_hi=None, flt=None, own=None):
        """Top-k scoring corruptions of one side for every query triple: (positions int32 [n,k] into the candidate list /
        row range, scores fp32 [n,k]).  Queries go through amdkge_corruption_scores in chunks whose score block stays under
        SCORE_CHUNK_BYTES, each chunk straight into amdkge_topk_rows.  With flt = (lo, hi, ids) (FilterIndex.device_filter of
        the queries) and / or own (int32 [n] entity ids) the chunk goes to amdkge_topk_rows_excluding instead: a candidate
        whose entity id is in the query's range, or equals own[query], takes no part in the selection."""
        n = int(triples.shape[0])
        if ent_hi is None:
            ent_hi = self.n_ents if ent_ids is None else int(ent_ids.shape[0])
        out_i, out_v = self._idx_val(n, k)
        excluding = flt is not None or own is not None
        col_ids = None if ent_ids is None else ent_ids[int(ent_lo):int(ent_hi)]
        for c0, c1, blk in self._corruption_blocks(triples, side, ent_ids, ent_lo, ent_hi):
            if excluding:
                out_i[c0:c1], out_v[c0:c1] = self.topk_rows_excluding(blk, k, col_ids, int(ent_lo), self._flt_chunk(flt, c0, c1),
                                                                      None if own is None else own[c0:c1])
            else:
                out_i[c0:c1], out_v[c0:c1] = self.topk_rows(blk, k)
        return out_i, out_v

    # ------------------------------------------------------------------ relation prediction (kge_relation.hip, kge_filter.hip)
    def pair_filter_build(self, triples, n_ents, n_rels):
        """amdkge_pair_filter_build: the CSR of the relations known between every (s, o) pair of the id triples, see _filter_build."""
        return self._filter_build(triples, None, n_ents, n_rels)

    def pair_filter_ranges(self, keys, start, triples, n_ents):
        """(lo, hi) int64 device tensors: each triple's (s, o) range in a PairFilterIndex id array (amdkge_pair_filter_ranges)."""
        return self._filter_ranges(keys, start, triples, None, n_ents)

    def _relation_block(self, triples, rel_ids, lo, hi, out, ld):
        work = None
        need = int(self.lib.amdkge_relation_workspace_bytes(C.byref(self.model), hi - lo))
        if need > 0:
            work = self._buf("relation_work", (need,), torch.uint8)
        check(self.lib.amdkge_relation_scores(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples), int(triples.shape[0]),
                                              _ptr(rel_ids), int(lo), int(hi), _ptr(out), int(ld), _ptr(work), _stream()))

    def relation_scores(self, triples, rel_ids=None, out=None, rel_lo=0, rel_hi=None):
        """Scores fp32 [n, m] of (s_i, r_j, o_i) for every query row of `triples` (int32 [n,3] device tensor; the predicate column is
        ignored) and every candidate relation -- rows [rel_lo, rel_hi) of the relation table, or of the list rel_ids (int32 device
        tensor) --, each with the bits score() gives the materialised triple (amdkge_relation_scores).  out: an fp32 [n, >= m]
        device tensor whose rows may be strided; its columns beyond m are left untouched."""
        n = int(triples.shape[0])
        if rel_hi is None:
            rel_hi = self.n_rels if rel_ids is None else int(rel_ids.shape[0])
        m = int(rel_hi) - int(rel_lo)
        if out is None:
            out = torch.empty(n, m, dtype=torch.float32, device=self.device)
        if out.ndim != 2 or out.dtype != torch.float32 or int(out.shape[0]) != n or int(out.shape[1]) < m or (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError("relation_scores: `out` must be an fp32 [n, >= m] tensor with unit column stride")
        self._relation_block(triples, rel_ids, rel_lo, rel_hi, out, int(out.stride(0)) if n > 1 else max(int(out.shape[1]), m))
        return out[:, :m]

    def relation_rank(self, triples, strategy="worst", flt=None, rel_ids=None, subset_pos=None):
        """1-based ranks (int32 [n]) of each triple's OWN relation among the candidate relations (all, or rel_ids), with the tie
        and filter conventions of the entity sides: the positive's score (score()) against the 1-vs-all block of relation_scores
        in quantised comparisons (amdkge_relation_rank_counts), composed by amdkge_rank_compose.  flt = (lo, hi, ids) of
        PairFilterIndex.device_filter; subset_pos (int32 [n_rels], -1 = not a candidate) maps a relation to its column of rel_ids
        and is derived from rel_ids when not given.  -> (ranks, counts, sub)."""
        n = int(triples.shape[0])
        m = self.n_rels if rel_ids is None else int(rel_ids.shape[0])
        if rel_ids is not None and subset_pos is None:
            subset_pos = subset_positions(rel_ids.cpu().numpy(), self.n_rels, self.device)
        pos = self.score(triples)
        counts = torch.zeros(n, 2, dtype=torch.int32, device=self.device)
        sub = torch.zeros(n, dtype=torch.int32, device=self.device) if flt is not None else None
        for c0, c1, blk in self._relation_blocks(triples, rel_ids, m):
            lo, hi, ids = self._flt_chunk(flt, c0, c1) or (None, None, None)
            check(self.lib.amdkge_relation_rank_counts(_ptr(blk), c1 - c0, m, m, _ptr(pos[c0:c1]), _ptr(rel_ids), 0, _ptr(lo), _ptr(hi), _ptr(ids),
                                                       _ptr(subset_pos), _ptr(counts[c0:c1]), _ptr(None if sub is None else sub[c0:c1]), _stream()))
        return self.compose_ranks(counts, sub, strategy), counts, sub

    def relation_topk(self, triples, k, rel_ids=None, flt=None):
        """The k (<= 1024) best candidate relations of every query pair: (positions int32 [n,k] into the candidate list / the
        relation table, scores fp32 [n,k]), best first, equal scores by increasing position, missing entries -1 / -inf.  With
        flt = (lo, hi, ids) (PairFilterIndex.device_filter of the queries) a relation already known between the pair takes no
        part in the selection (amdkge_topk_rows_excluding over each chunk's relation_scores block)."""
        n = int(triples.shape[0])
        m = self.n_rels if rel_ids is None else int(rel_ids.shape[0])
        out_i, out_v = self._idx_val(n, k)
        for c0, c1, blk in self._relation_blocks(triples, rel_ids, m):
            out_i[c0:c1], out_v[c0:c1] = self.topk_rows_excluding(blk, k, rel_ids, 0, self._flt_chunk(flt, c0, c1), None)
        return out_i, out_v

    def nearest_rows(self, q_rows, k, metric="euclidean", ent_ids=None, ent_lo=0, ent_hi=None, table=None):
        """k nearest table rows of every query row (stored layout, [n, Ks]), nearest first: (positions int32 [n,k],
        distances fp32 [n,k]).  Selection in GEMM form on the tile kernel (amdkge_row_dots) with the norms folded into
        amdkge_topk_rows' column scale / bias (euclidean: v = <q,e> - |e|^2 / 2; cosine: v = <q,e> / |e|) -- the distance matrix
        never exists; the k survivors are then re-measured exactly (amdkge_pair_distances: the GEMM form cancels for near
        neighbours) and put in their final order."""
        table = self.ent if table is None else table
        n = int(q_rows.shape[0])
        if ent_hi is None:
            ent_hi = int(table.shape[0]) if ent_ids is None else int(ent_ids.shape[0])
        m = int(ent_hi) - int(ent_lo)
        Kf = int(table.shape[1])
        q_rows = q_rows.contiguous()
        col = torch.empty(m, dtype=torch.float32, device=self.device)
        cosine = metric == "cosine"
        check(self.lib.amdkge_row_sqnorms(_ptr(table), Kf, _ptr(ent_ids), int(ent_lo), m, -0.5, 1 if cosine else 0, _ptr(col), _stream()))
        out_i, out_v = self._idx_val(n, k)
        for c0, c1 in self._score_chunks(n, m):
            blk = self._buf("disc_scores", (c1 - c0, m), torch.float32)
            check(self.lib.amdkge_row_dots(_ptr(q_rows[c0:c1]), c1 - c0, _ptr(table), Kf, _ptr(ent_ids), int(ent_lo), int(ent_hi), _ptr(blk), m,
                                           _stream()))
            out_i[c0:c1], out_v[c0:c1] = self.topk_rows(blk, k, True, col if cosine else None, None if cosine else col)
        dist = torch.empty(n, int(k), dtype=torch.float32, device=self.device)
        check(self.lib.amdkge_pair_distances(_ptr(q_rows), n, _ptr(table), Kf, _ptr(ent_ids), int(ent_lo), _ptr(out_i), int(k), 1 if cosine else 0,
                                             _ptr(dist), _stream()))
        return self.topk_rows(dist, k, largest=False, payload=out_i)   # final order by the exact distances

    def join_nearest(self, X):
        """Exact self-join of the fp32 device matrix X [n, d] (amdkge_join_nearest): every row's nearest OTHER row in squared
        euclidean distance -> (d2 fp32 [n], idx int32 [n] (equal distances: the lower index; n == 1: +inf / -1), largest
        pair d2 fp32 [1]), all on the device."""
        X = X.to(self.device, torch.float32).contiguous()
        n, d = int(X.shape[0]), int(X.shape[1])
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        idx = torch.empty(n, dtype=torch.int32, device=self.device)
        mx = torch.empty(1, dtype=torch.float32, device=self.device)
        work = self._buf("join_keys", (max(n, 1),), torch.int64)
        check(self.lib.amdkge_join_nearest(_ptr(X), n, d, _ptr(dist), _ptr(idx), _ptr(mx), _ptr(work), _stream()))
        return dist, idx, mx

    def join_radius(self, X, thr):
        """Every unordered pair i < j of rows of the fp32 device matrix X [n, d] with squared euclidean distance <= thr
        (amdkge_join_radius) -> int32 device tensor [m, 2], sorted lexicographically.  One synchronisation reads the count;
        a count beyond the buffer's capacity relaunches with a buffer of that size."""
        X = X.to(self.device, torch.float32).contiguous()
        n, d = int(X.shape[0]), int(X.shape[1])
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        cap = max(4 * n, 4096)
        while True:
            pairs = torch.empty(cap, 2, dtype=torch.int32, device=self.device)
            check(self.lib.amdkge_join_radius(_ptr(X), n, d, float(thr), _ptr(pairs), cap, _ptr(count), _stream()))
            m = int(count.item())
            if m <= cap:
                break
            cap = m
        key = pairs[:m].to(torch.int64)
        order = torch.argsort(key[:, 0] * max(n, 1) + key[:, 1])
        return pairs[:m][order].contiguous()

    def dbscan(self, X, thr, min_samples):
        """DBSCAN over the rows of the fp32 device matrix X [n, d] on the self-join (amdkge_join_dbscan): row j is a neighbour of
        row i when their squared euclidean distance is <= thr (i is its own neighbour), a row with at least min_samples neighbours
        is a core row -> (labels int32 [n] in sklearn's numbering, -1 = noise; core bool [n]; n_clusters int32 [1]), all on the
        device, no synchronisation.  Three passes over the pairs and 12 n bytes of scratch: no pair list."""
        X = X.to(self.device, torch.float32).contiguous()
        n, d = int(X.shape[0]), int(X.shape[1])
        labels = torch.empty(n, dtype=torch.int32, device=self.device)
        core = torch.empty(n, dtype=torch.uint8, device=self.device)
        n_clusters = torch.empty(1, dtype=torch.int32, device=self.device)
        work = self._buf("join_dbscan", (max(int(self.lib.amdkge_join_dbscan_workspace_bytes(n)) // 4, 1),), torch.int32)
        check(self.lib.amdkge_join_dbscan(_ptr(X), n, d, float(thr), int(min_samples), _ptr(labels), _ptr(core), _ptr(n_clusters), _ptr(work),
                                          _stream()))
        return labels, core.view(torch.bool), n_clusters

    # ------------------------------------------------------------------ discovery.KMeans (kge_kmeans.hip)
    KMEANS_WORK_BYTES = 1 << 30   # bound of the Lloyd workspace (the per-block partial sums): more runs than fit go in groups

    def kmeans_assign(self, X, centres):
        """Nearest centre of every row of the fp32 device matrix X [n, d] (amdkge_kmeans_assign): centres [runs, k, d] ->
        (labels int32 [runs, n], mind2 fp32 [runs, n]); centres [k, d] -> ([n], [n]).  The distance is the self-join's fp32 value,
        equal distances go to the lowest centre.  On the device, no synchronisation."""
        X = X.to(self.device, torch.float32).contiguous()
        C3 = centres.to(self.device, torch.float32).contiguous()
        single = C3.dim() == 2
        if single:
            C3 = C3[None]
        n, d = int(X.shape[0]), int(X.shape[1])
        runs, k = int(C3.shape[0]), int(C3.shape[1])
        if int(C3.shape[2]) != d:
            raise ValueError("centres have %d columns, X has %d" % (int(C3.shape[2]), d))
        labels = torch.empty(runs, n, dtype=torch.int32, device=self.device)
        mind2 = torch.empty(runs, n, dtype=torch.float32, device=self.device)
        check(self.lib.amdkge_kmeans_assign(_ptr(X), n, d, _ptr(C3), k, runs, _ptr(labels), _ptr(mind2), _stream()))
        return (labels[0], mind2[0]) if single else (labels, mind2)

    def kmeans(self, X, centres0, max_iter, tol_abs, check_every=8):
        """Lloyd's iterations of `runs` independent restarts over the rows of the fp32 device matrix X [n, d], from centres0 [runs, k, d]
        (amdkge_kmeans_lloyd; the stop rules and the empty-cluster rule are stated in include/amdkge.h) -> (centres fp32 [runs, k, d],
        labels int32 [runs, n], inertia fp64 [runs], n_iter int32 [runs], done int32 [runs]: 1 = no label changed, 2 = the centres
        moved by no more than tol_abs, 0 = max_iter reached), all on the device.  The iterations are enqueued check_every at a time
        (the last chunk shortened to max_iter); between chunks one read of the runs' state is the only synchronisation.  Runs go in
        groups whose workspace stays under KMEANS_WORK_BYTES.  A run's result does not depend on runs, the grouping or check_every."""
        X = X.to(self.device, torch.float32).contiguous()
        C = centres0.to(self.device, torch.float32).clone().contiguous()
        n, d = int(X.shape[0]), int(X.shape[1])
        runs, k = int(C.shape[0]), int(C.shape[1])
        if C.dim() != 3 or int(C.shape[2]) != d:
            raise ValueError("centres0 must be [runs, k, %d]" % d)
        max_iter, check_every = int(max_iter), max(int(check_every), 1)
        labels = torch.full((runs, n), -1, dtype=torch.int32, device=self.device)
        mind2 = torch.empty(runs, n, dtype=torch.float32, device=self.device)
        state = torch.zeros(runs, 4, dtype=torch.int32, device=self.device)
        inertia = torch.zeros(runs, dtype=torch.float64, device=self.device)
        one = int(self.lib.amdkge_kmeans_workspace_bytes(n, d, k, 1))
        if one < 0:
            raise ValueError("kmeans: sizes out of range (n %d, d %d, k %d)" % (n, d, k))
        group = max(1, min(runs, self.KMEANS_WORK_BYTES // max(one, 1)))
        for r0 in range(0, runs, group):
            g = min(group, runs - r0)
            work = self._buf("kmeans_work", (max(int(self.lib.amdkge_kmeans_workspace_bytes(n, d, k, g)) // 8, 1),), torch.int64)
            args = (_ptr(labels[r0:r0 + g]), _ptr(mind2[r0:r0 + g]), _ptr(state[r0:r0 + g]), _ptr(inertia[r0:r0 + g]), _ptr(work), _stream())

            def lloyd(iters):
                check(self.lib.amdkge_kmeans_lloyd(_ptr(X), n, d, _ptr(C[r0:r0 + g]), k, g, iters, float(tol_abs), *args))

            it, done = 0, torch.zeros(g, dtype=torch.int32)
            while it < max_iter:
                step = min(check_every, max_iter - it)
                lloyd(step)
                it += step
                done = state[r0:r0 + g, 1].cpu()
                if bool((done != 0).all()):
                    break
            if n > 0 and bool((done != 1).any()):
                lloyd(0)   # labels and inertia of the final centres (a strict stop has them already)
        return C, labels, inertia, state[:, 0].contiguous(), state[:, 1].contiguous()

    # ------------------------------------------------------------------ discover_facts(strategy="exhaustive") (kge_discover.hip)
    _INT32_MIN = -(1 << 31)

    def select_margin(self, rel_id):
        """margin_q of amdkge_discover_select for relation rel_id: an upper bound, in quanta of 1e-3, on the distance between
        rank_prep's and the tile chain's fp32 value of one (s, rel_id, o) pair, from the largest entity row norm and the relation
        row (DESIGN.md section 3 has the derivation): both values evaluate one sum of monomials with at most K + 18 roundings on
        any path, so each is within gamma(K + 18) * B of the exact score, B = a bound on the sum of the monomials' magnitudes."""
        col = torch.empty(self.n_ents, dtype=torch.float32, device=self.device)
        check(self.lib.amdkge_row_sqnorms(_ptr(self.ent), self.Ks, None, 0, self.n_ents, 1.0, 0, _ptr(col), _stream()))
        p = self.rel[int(rel_id)].to(torch.float64)
        s2 = float(col.max().item()) * 1.001   # (the fp32 norm itself carries (K + 1) roundings)
        p_inf, p_2 = float(p.abs().max().item()), float(torch.linalg.vector_norm(p).item())
        K = float(self.Ks)
        st = self.scoring_type
        if st == "TransE":
            B = np.sqrt(K) * (2.0 * np.sqrt(s2) + p_2)   # sum_c |s_c| + |p_c| + |o_c|, |x|_1 <= sqrt(K) |x|_2
        elif st == "RotatE":
            B = 3.0 * np.sqrt(K) * np.sqrt(s2)           # sum_c (|cos| + |sin|)(|s_re| + |s_im|) + |o_re| + |o_im|
        else:
            B = p_inf * s2                               # sum_c |s_c p_c o_c| <= |p|_inf |s|_2 |o|_2
            if st != "DistMult":
                B *= 2.0                                 # four triple products per complex unit
            if st == "HolE":
                B *= 2.0 / self.k_full
        n_round = K + 18.0
        u = 2.0 ** -24
        gamma = n_round * u / (1.0 - n_round * u)
        mq = 1.0 + np.ceil(1000.0 * 2.0 * gamma * B)
        return int(mq) if np.isfinite(mq) and mq < 2 ** 30 else 2 ** 30

    def _select_thresholds_sorted(self, vals, flt, R):
        """T of amdkge_discover_select by a full device sort of the quantised rows: R beyond the streaming selection's 1024."""
        n, m = int(vals.shape[0]), int(vals.shape[1])
        v = vals.to(torch.float32)
        bad = ~torch.isfinite(v).all(1)
        q = torch.trunc(torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0) * 1000.0).clamp(-2147483648.0, 2147483520.0).to(torch.int64)
        gone = -(1 << 40)
        if flt is not None:
            lo, hi, ids = flt
            cnt = (hi - lo).clamp(min=0)
            rows = torch.repeat_interleave(torch.arange(n, device=self.device), cnt)
            first = torch.cumsum(cnt, 0) - cnt
            pos = torch.arange(int(rows.shape[0]), device=self.device) - first[rows] + lo[rows]
            cols = ids[pos].to(torch.int64)
            ok = (cols >= 0) & (cols < m)
            q[rows[ok], cols[ok]] = gone
        thr = torch.full((n,), self._INT32_MIN, dtype=torch.int64, device=self.device)
        if m >= R:
            t = torch.sort(q, dim=1, descending=True).values[:, R - 1]
            thr = torch.where((t == gone) | bad, thr, t)
        return thr.to(torch.int32)

    def select_rows(self, vals, queries, side, R, margin_q, flt=None, row_base=0, cap=None):
        """amdkge_discover_select on the score block vals [n, m] (columns = entity ids) of the query rows `queries` (int32 [n, 3]):
        -> (pairs int32 [c, 2] of (row_base + row, column), in no particular order; thresholds int32 [n]).  One synchronisation
        reads the count; a count beyond the buffer's capacity relaunches with a buffer of that size."""
        n, m = int(vals.shape[0]), int(vals.shape[1])
        R = int(R)
        given = 1 if R > 1024 else 0
        thr = self._select_thresholds_sorted(vals, flt, R) if given else torch.empty(n, dtype=torch.int32, device=self.device)
        lo, hi, ids = flt if flt is not None else (None, None, None)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        cap = max(4096, 2 * min(R, m) * n) if cap is None else int(cap)
        while True:
            pairs = torch.empty(cap, 2, dtype=torch.int32, device=self.device)
            check(self.lib.amdkge_discover_select(_ptr(vals), n, m, int(vals.stride(0)) if n else m, _ptr(queries), int(side), _ptr(lo), _ptr(hi),
                                                  _ptr(ids), R, int(margin_q), _ptr(thr), given, int(row_base), _ptr(pairs), cap, _ptr(count),
                                                  _stream()))
            c = int(count.item())
            if c <= cap:
                break
            cap = c
        return pairs[:c], thr

    def corruption_select(self, triples, side, R, margin_q, flt=None):
        """select_rows over the 1-vs-all scores of every query triple against ALL entities: queries go through
        amdkge_corruption_scores in chunks whose score block stays under SCORE_CHUNK_BYTES (as corruption_topk), each chunk
        straight into the selection.  -> (pairs int32 [c, 2] of (query, entity), thresholds int32 [n])."""
        n, m = int(triples.shape[0]), self.n_ents
        out = [torch.empty(0, 2, dtype=torch.int32, device=self.device)]
        thr = torch.empty(n, dtype=torch.int32, device=self.device)
        for c0, c1, blk in self._corruption_blocks(triples, side, None, 0, m):
            p_, thr[c0:c1] = self.select_rows(blk, triples[c0:c1], side, R, margin_q, self._flt_chunk(flt, c0, c1), row_base=c0)
            out.append(p_)
        return torch.cat(out), thr

    def platt_step(self, scores_pos, scores_neg, w, b, label_pos, label_neg, weight_pos, weight_neg):
        """(loss, dloss/dw, dloss/db) of the Platt-scaling objective for one batch (amdkge_platt_step)."""
        out = torch.zeros(3, dtype=torch.float64, device=self.device)
        check(self.lib.amdkge_platt_step(_ptr(scores_pos), int(scores_pos.shape[0]), _ptr(scores_neg),
                                         int(scores_neg.shape[0]), float(w), float(b), float(label_pos), float(label_neg),
                                         float(weight_pos), float(weight_neg), _ptr(out), _stream()))
        return [float(v) for v in out.tolist()]

    # ------------------------------------------------------------------ evaluate
    def _workspace(self, n, lane=0):
        need = int(self.lib.amdkge_rank_workspace_bytes(C.byref(self.model), n))
        if lane:
            return self._buf(f"rank_work_lane{lane}", (need,), torch.uint8)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._work

    SCREEN_MAX_BYTES = 4 << 30

    def _side_stream(self, lane=0):
        """Extra streams of this engine's device: 2 * lane for the filter pass of rank_side (beside the count pass), 2 * lane + 1
        for the lane itself when rank_sides runs several corruption sides at once."""
        st = getattr(self, "_fstreams", None)
        if st is None:
            st = self._fstreams = {}
        if lane not in st:
            st[lane] = torch.cuda.Stream(device=self.device)
        return st[lane]

    def screen_stats(self):
        """Of the LAST rank_side call (with rank_sides: its last lane): None when no screening / early-exit workspace was handed to
        the count pass (huge candidate ranges, or the library sees nothing to gain), else (pairs the exact chain re-checked,
        fell back to the exact kernel?) -- contraction models: of the int8 screening pass; TransE / RotatE: of the exact early exit
        ((0, False) when its probe picked the plain kernel; likewise problems too small for either pass).  Synchronises."""
        s = getattr(self, "_last_screen", None)
        if s is None:
            return None
        v = s[:8].view(torch.int32).cpu().numpy()
        return int(v[0]), bool(v[1])

    def rank_sides(self, triples, jobs, strategy="worst", ent_ids=None, subset_pos=None):
        """Several corruption sides of the same triples AT ONCE: jobs = [(side, flt, out, out_stride), ...], each on a stream and
        with workspaces of its own, joined into the current stream.  A side is one long kernel (the screening / count pass) between
        a dozen short latency-bound ones (query vectors, limbs, thresholds, merge, compose: ~13 % of a side at the C2 shape); with
        two sides in flight the short kernels of one run under the long kernel of the other."""
        if len(jobs) == 1:
            side, flt, out, stride = jobs[0]
            return [self.rank_side(triples, side, strategy, flt, ent_ids, subset_pos, out=out, out_stride=stride)]
        if os.environ.get("AMDKGE_EVAL_LANES") == "1":   # (A/B measurements: the sides one after the other)
            return [self.rank_side(triples, side, strategy, flt, ent_ids, subset_pos, out=out, out_stride=stride) for side, flt, out, stride in jobs]
        # Every lane keeps workspaces of its own (query vectors, the screening pass's fixed-point rows and recheck list -- up to
        # SCREEN_MAX_BYTES --, the filter pass's copy), so two sides in flight about double evaluate()'s peak memory.
        # Beside resident training state on a large table that can be what runs the device out of memory: the sides then run one
        # after the other on the first lane's workspaces.
        n = int(triples.shape[0])
        m = (self.n_ents if ent_ids is None else int(ent_ids.shape[0]))
        per_lane = 2 * int(self.lib.amdkge_rank_workspace_bytes(C.byref(self.model), n)) + \
            min(max(int(self.lib.amdkge_rank_screen_workspace_bytes(C.byref(self.model), n, m)), 0), self.SCREEN_MAX_BYTES)
        extra = per_lane * (len(jobs) - 1)
        have = sum(int(t.numel()) * int(t.element_size()) for k_, t in self._bufs.items() if "_lane" in k_)   # BYTES earlier calls already hold
        # (the driver query costs ~10 us and is only made when the lanes' workspaces still have to grow)
        if extra > have and extra - have > torch.cuda.mem_get_info(self.device)[0] // 4:
            return [self.rank_side(triples, side, strategy, flt, ent_ids, subset_pos, out=out, out_stride=stride) for side, flt, out, stride in jobs]
        main = torch.cuda.current_stream()
        res, lanes = [], []
        for i, (side, flt, out, stride) in enumerate(jobs):
            st = self._side_stream(2 * i + 1)
            st.wait_stream(main)
            lanes.append(st)
            with torch.cuda.stream(st):
                res.append(self.rank_side(triples, side, strategy, flt, ent_ids, subset_pos, out=out, out_stride=stride, lane=i))
        for st in lanes:
            main.wait_stream(st)
        return res

    def rank_side(self, triples, side, strategy="worst", flt=None, ent_ids=None, subset_pos=None,
                  ent_lo=0, ent_hi=None, out=None, out_stride=1, flt_range=None, lane=0):
        """Ranks (1-based, reference semantics) of `triples` for one corruption side.

        flt: None or (lo int64[n], hi int64[n], ids int32[*]) cuda tensors; flt_range: id range the filter ids are
        checked against when it differs from the candidate positions [ent_lo, ent_hi) (row-sharded subsets); lane: which set of
        workspaces / side stream to use (rank_sides)."""
        n = int(triples.shape[0])
        if ent_hi is None:
            ent_hi = self.n_ents if ent_ids is None else int(ent_ids.shape[0])
        work = self._workspace(n, lane)
        sfx = f"_lane{lane}" if lane else ""
        counts = torch.zeros(n, 2, dtype=torch.int32, device=self.device)
        # contraction models: the int8 screening pass + exact recheck (kge_rank_screen.hip) -- the same counts, bit for bit, at a
        # multiple of the fp32 matrix rate; its workspace (fixed-point copies of the query vectors and the candidate rows, the
        # recheck list) is kept between calls.  Beyond SCREEN_MAX_BYTES (huge candidate ranges) the exact kernel runs alone.
        screen, sbytes = None, 0
        need = int(self.lib.amdkge_rank_screen_workspace_bytes(C.byref(self.model), n, int(ent_hi) - int(ent_lo))) if n > 0 else 0
        if 0 < need <= self.SCREEN_MAX_BYTES:
            screen, sbytes = self._buf("rank_screen" + sfx, (need,), torch.uint8), need
            screen[:256].zero_()   # the statistics words are written only by the passes that run (stale bytes otherwise)
        self._last_screen = screen
        # The filter pass (a latency-bound walk over each triple's known positives) is independent of the count pass: it runs
        # beside it on a second stream with a workspace of its own and is joined before the two are composed.
        sub, main, fstream = None, torch.cuda.current_stream(), None
        if flt is not None:
            lo, hi, ids = flt
            sub = torch.zeros(n, dtype=torch.int32, device=self.device)
            f_lo, f_hi = (ent_lo, ent_hi) if flt_range is None else flt_range
            fwork = self._buf("rank_work_filter" + sfx, (work.numel(),), torch.uint8)
            fstream = self._side_stream(2 * lane)
            fstream.wait_stream(main)
            with torch.cuda.stream(fstream):
                check(self.lib.amdkge_rank_filter(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples),
                                                  n, side, _ptr(lo), _ptr(hi), _ptr(ids), _ptr(subset_pos),
                                                  int(f_lo), int(f_hi), _ptr(sub), _ptr(fwork), _stream()))
        check(self.lib.amdkge_rank_counts_screened(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), _ptr(triples), n,
                                                   side, _ptr(ent_ids), int(ent_lo), int(ent_hi), _ptr(counts),
                                                   _ptr(work), _ptr(screen), sbytes, _stream()))
        if fstream is not None:
            main.wait_stream(fstream)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
            out_stride = 1
        check(self.lib.amdkge_rank_compose(_ptr(counts), _ptr(sub), n, _ffi.RANK_STRATEGY[strategy], _ptr(out),
                                           int(out_stride), _stream()))
        return out, counts, sub

    def rank_lists(self, triples, side, cand, strategy="worst", flt=None, out=None, out_stride=1, want_scores=False, lane=0):
        """Ranks (1-based) of `triples` for one corruption side, each against ITS OWN candidate list (amdkge_rank_lists,
        include/amdkge_lists.h): cand = (lo int64[n], hi int64[n], ids int32[*], max_len) -- triple i's candidates are the table
        rows ids[lo[i]:hi[i]], every occurrence a candidate of its own, ids outside the table skipped; max_len bounds hi - lo (it
        only plans the launch).  flt as in rank_side: None or (lo, hi, ids), the known positives ascending inside a range.  Returns
        (ranks, counts, sub), and with want_scores a fourth: fp32 scores parallel to `ids` (-inf at a skipped id; positions no list
        covers are not written)."""
        n = int(triples.shape[0])
        lo, hi, ids, max_len = cand
        work = self._workspace(n, lane)
        counts = torch.zeros(n, 2, dtype=torch.int32, device=self.device)
        sub = f_lo = f_hi = f_ids = None
        if flt is not None:
            f_lo, f_hi, f_ids = flt
            sub = torch.zeros(n, dtype=torch.int32, device=self.device)
        scores = torch.empty(int(ids.shape[0]), dtype=torch.float32, device=self.device) if want_scores else None
        check(self.lib.amdkge_rank_lists(C.byref(self.model), _ptr(self.ent), _ptr(self.rel), int(self.ent.shape[0]), _ptr(triples), n,
                                         int(side), _ptr(lo), _ptr(hi), _ptr(ids), int(max_len), _ptr(f_lo), _ptr(f_hi), _ptr(f_ids),
                                         _ptr(counts), _ptr(sub), _ptr(scores), _ptr(work), _stream()))
        out = self.compose_ranks(counts, sub, strategy, out, out_stride)
        return (out, counts, sub, scores) if want_scores else (out, counts, sub)
