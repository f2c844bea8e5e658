"""Entity tables beyond 2^31 elements whose every row the host knows: test infrastructure of tests/test_gpu_wide_offsets.py (the product
does not import it).

Row i of a table is base[i % P]: `base` holds P = 4 099 fp32 rows drawn on the host and copied to the device once; the table is filled
there by chunked index_select, so no host array of the table's size ever exists and a reference never copies the table back.

P is prime and the row widths used (2 000 and 400 floats) divide neither 2^31 nor 2^32, so an element offset that wrapped at 32 bits
lands in the middle of a row -- 2^31 mod 2 000 = 1 648, 2^32 mod 2 000 = 1 296, 2^31 mod 400 = 48, 2^32 mod 400 = 96 -- never at
the start of a copy of the intended row: a wrapped read returns other values, a wrapped write dirties a row the test holds to its
bits.  (A row index that wrapped instead moves by 2^31 or 2^32 rows: 2^31 mod 4 099 = 2 107 and 2^32 mod 4 099 = 115, again another
base row.)

M <= 4 096 consecutive rows have distinct residues mod P: a window's compact copy is base[(lo + arange(M)) % P], and the oracle runs
on that copy with the ids shifted by lo."""
import numpy as np
import torch

P = 4099
M = 4096
CHUNK = 1 << 18           # rows per pass of a whole-table fill (a Geometry's checks take fewer where rows are long: Geometry.chunk)
_LIVE = []                # geometries that hold device memory: at most one at a time


def release_all():
    for g in list(_LIVE):
        g.release()


class Geometry:
    """One table shape: N = P * mult rows of Ks stored floats and R relation rows, shared by every model of that row width (one
    allocation: the engines of a geometry are views of the same flat parameter buffer)."""

    def __init__(self, name, mult, Ks, R):
        self.name, self.mult, self.Ks, self.R = name, int(mult), int(Ks), int(R)
        self.N = P * self.mult
        self.chunk = min(CHUNK, (1 << 27) // (4 * self.Ks))   # rows per pass of a whole-table check: temporaries of at most 128 MiB
        assert self.N * self.Ks > 2 ** 31 and (2 ** 31) % self.Ks != 0 and (2 ** 32) % self.Ks != 0
        self.flat = None
        self.engines = {}
        self.g_flat = None
        self.slot_flat = {}
        self.base = self.rel = self.base_d = None
        self.family = None
        # the windows: T the last M rows; S centred on the first row that starts beyond element 2^31 - 1 (the row before it
        # crosses the boundary); B centred on the row that crosses BYTE offset 2^32 (element 2^30)
        self.first_high = (2 ** 31 - 1) // self.Ks + 1
        self.T = self.N - M
        self.S = self.first_high - M // 2
        self.B = (2 ** 30) // self.Ks - M // 2
        assert 0 < self.B and self.B + M < self.S and self.S + M < self.T
        assert (self.S + M - 1) * self.Ks > 2 ** 31 - 1 > self.S * self.Ks
        assert (self.B + M - 1) * self.Ks * 4 > 2 ** 32 - 1 > self.B * self.Ks * 4

    # ------------------------------------------------------------------ memory
    def engine(self, model, k, k_full=None):
        """The KgeEngine of (model, k) on this geometry's table: the first one allocates the flat buffer, the others share it.
        k_full: a column-slice engine (k of the k_full units of a wider model's rows)."""
        from ampligraph_amd.engine import KgeEngine

        key = (model, k, k_full)
        if key in self.engines:
            return self.engines[key]
        for g in list(_LIVE):
            if g is not self:
                g.release()
        if self not in _LIVE:
            _LIVE.append(self)
        shared = self.flat

        class _TableEngine(KgeEngine):
            def _flat(self, pad_to=64 * 16, fill=0.0):
                nonlocal shared
                if shared is not None:
                    t, shared = shared, None
                    return t
                return super()._flat(pad_to, fill)

        eng = _TableEngine(model, k, self.N, self.R, max_rel_size=self.R, k_full=k_full)
        assert eng.Ks == self.Ks == eng.K, (model, k, eng.Ks, eng.K)   # no padding units: stored rows are dense rows
        assert eng.ent.numel() > 2 ** 31
        if self.flat is None:
            self.flat = eng.p_flat
        assert eng.p_flat.data_ptr() == self.flat.data_ptr() and eng.p_flat.numel() == self.flat.numel()
        self.engines[key] = eng
        return eng

    @property
    def ent(self):
        return next(iter(self.engines.values())).ent

    @property
    def rel_d(self):
        return next(iter(self.engines.values())).rel

    def release(self):
        for eng in self.engines.values():
            eng.p_flat = eng.ent = eng.rel = eng.g_flat = eng.g_ent = eng.g_rel = None
            eng.slots, eng.slot_flat, eng._bufs, eng._work, eng._twork, eng._last_screen = {}, {}, {}, None, None, None
        self.engines = {}
        self.flat = self.g_flat = self.base_d = None
        self.slot_flat = {}
        self.family = None
        if self in _LIVE:
            _LIVE.remove(self)
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ content
    def fill(self, family, seed=0, scale=0.25, rel_scale=None):
        """Row i <- base[i % P].  family "gaussian": normal * scale; "ties": small integers / 8 (relations: / 4), as
        test_gpu_rank_widths_oracle._contraction_tables."""
        assert self.engines, "fill() needs an engine (it owns the buffer)"
        key = (family, seed, scale, rel_scale)
        if self.family == key:
            return
        self.host_tables(family, seed, scale, rel_scale)
        self.base_d = torch.as_tensor(self.base).cuda()
        self.rel_d.copy_(torch.as_tensor(self.rel))
        self.restore()
        self.family = key

    def host_tables(self, family, seed=0, scale=0.25, rel_scale=None):
        """the host side of fill(): `base` and the relation rows (no device needed)"""
        rng = np.random.default_rng(seed)
        if family == "ties":
            self.base = (rng.integers(-4, 5, size=(P, self.Ks)) / 8.0).astype(np.float32)
            self.rel = (rng.integers(-2, 3, size=(self.R, self.Ks)) / 4.0).astype(np.float32)
        else:
            self.base = (rng.normal(size=(P, self.Ks)) * scale).astype(np.float32)
            self.rel = (rng.normal(size=(self.R, self.Ks)) * (scale if rel_scale is None else rel_scale)).astype(np.float32)

    def _idx(self, r0, r1):
        return torch.arange(r0, r1, device="cuda") % P

    def restore(self, table=None, lo=0, hi=None, source=None):
        """rows [lo, hi) of the table (or of `table`, a buffer of its shape) <- their base rows (or source[i % P], a device [P, Ks])"""
        table = self.ent if table is None else table
        source = self.base_d if source is None else source
        hi = self.N if hi is None else hi
        for r0 in range(lo, hi, CHUNK):
            r1 = min(hi, r0 + CHUNK)
            torch.index_select(source, 0, self._idx(r0, r1), out=table[r0:r1])

    def restore_rel(self):
        self.rel_d.copy_(torch.as_tensor(self.rel))

    def window(self, lo, m=M):
        """the compact host copy of rows [lo, lo + m)"""
        return self.base[(lo + np.arange(m)) % P]

    def rows(self, ids):
        return self.base[np.asarray(ids, dtype=np.int64) % P]

    # ------------------------------------------------------------------ whole-table checks, CHUNK rows at a time
    def rows_differing(self, table=None, source=None):
        """bool [N] (device): rows of the table (or of `table`) whose BITS differ from their base row (or from source[i % P])"""
        table = self.ent if table is None else table
        source = self.base_d if source is None else source
        out = torch.empty(self.N, dtype=torch.bool, device="cuda")
        for r0 in range(0, self.N, self.chunk):
            r1 = min(self.N, r0 + self.chunk)
            want = source.index_select(0, self._idx(r0, r1))
            out[r0:r1] = (table[r0:r1].view(torch.int32) != want.view(torch.int32)).any(1)
        return out

    def rows_nonzero(self, buf):
        """bool [N] (device): rows of a table-shaped buffer that hold a set bit (-0.0 counts: 'exactly zero' is all bits clear)"""
        out = torch.empty(self.N, dtype=torch.bool, device="cuda")
        for r0 in range(0, self.N, self.chunk):
            r1 = min(self.N, r0 + self.chunk)
            out[r0:r1] = (buf[r0:r1].view(torch.int32) != 0).any(1)
        return out

    def assert_only(self, changed, touched_ids, what):
        """`changed` (rows_differing / rows_nonzero) holds no row outside touched_ids and at least one inside"""
        allowed = torch.zeros(self.N, dtype=torch.bool, device="cuda")
        allowed[torch.as_tensor(np.unique(np.asarray(touched_ids, dtype=np.int64))).cuda()] = True
        stray = torch.nonzero(changed & ~allowed).flatten()
        assert stray.numel() == 0, (what, "rows outside the touched set changed", stray[:8].tolist(), int(stray.numel()))
        assert bool((changed & allowed).any()), (what, "no row inside the touched set moved")

    # ------------------------------------------------------------------ training state (one gradient buffer per geometry)
    def training(self, eng, optimizer="sgd"):
        """KgeEngine.prepare_training on buffers the geometry's engines share: the gradient buffer and the optimizer slots are
        allocated once (zero-filled) and zeroed here."""
        from ampligraph_amd import _ffi

        if self.g_flat is None:
            self.g_flat = torch.zeros_like(self.flat)
        else:
            self.g_flat.zero_()
        ne, nr, off = eng._ne, eng._nr, eng._off
        eng.opt_kind = optimizer
        eng.g_flat = self.g_flat
        eng.g_ent = self.g_flat[:ne].view_as(eng.ent)
        eng.g_rel = self.g_flat[off:off + nr].view_as(eng.rel)
        eng.slots, eng.slot_flat = {}, {}
        for nme in _ffi.OPT_SLOTS[optimizer]:
            if nme not in self.slot_flat:
                self.slot_flat[nme] = torch.zeros_like(self.flat)
            fl = self.slot_flat[nme]
            fl.fill_(0.1 if nme == "a" else 0.0)
            eng.slot_flat[nme] = fl
            eng.slots[nme + "_e"] = fl[:ne].view_as(eng.ent)
            eng.slots[nme + "_r"] = fl[off:off + nr].view_as(eng.rel)
        eng.loss_acc.zero_()

    def drop_scratch(self):
        """the engines' cached workspaces (rank / screening / score-block / tiled-step buffers)"""
        for eng in self.engines.values():
            eng._bufs, eng._work, eng._twork, eng._last_screen = {}, None, None, None
        torch.cuda.empty_cache()

    def drop_slots(self):
        for eng in self.engines.values():
            eng.slots, eng.slot_flat = {}, {}
        self.slot_flat = {}
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ ids
    def window_triples(self, rng, lo, B, m=M):
        """(X with table ids in [lo, lo + m), Xc the same with ids shifted by lo) int32 [B, 3]"""
        Xc = np.stack([rng.integers(0, m, B), rng.integers(0, self.R, B), rng.integers(0, m, B)], 1).astype(np.int32)
        X = Xc.copy()
        X[:, 0] += lo
        X[:, 2] += lo
        assert int(X[:, [0, 2]].max()) * self.Ks > 2 ** 31 - 1
        return X, Xc

    def spread_ids(self, rng, n):
        """n row ids drawn from T, S and B in turn (int64); the first three are the last row, the first row beyond 2^31 - 1
        elements and the row that crosses it"""
        los = np.array([self.T, self.S, self.B])[np.arange(n) % 3]
        ids = los + rng.integers(0, M, n)
        ids[:3] = (self.N - 1, self.first_high, self.first_high - 1)
        assert int(ids.max()) * self.Ks > 2 ** 31 - 1
        return ids.astype(np.int64)

    def spread_triples(self, rng, n):
        X = np.stack([self.spread_ids(rng, n), rng.integers(0, self.R, n), self.spread_ids(rng, n)[::-1]], 1).astype(np.int32)
        assert int(X[:, 0].max()) * self.Ks > 2 ** 31 - 1 and int(X[:, 2].max()) * self.Ks > 2 ** 31 - 1
        return X

    def mod(self, X):
        """triples with their entity ids reduced mod P: the same triples on `base`"""
        Xm = np.array(X, dtype=np.int32, copy=True)
        Xm[:, 0] %= P
        Xm[:, 2] %= P
        return Xm


WIDE = Geometry("wide", 281, 2000, 16)       # 1 151 819 rows x 2 000 floats: DistMult k = 2 000, RotatE k = 1 000
NARROW = Geometry("narrow", 1342, 400, 16)   # 5 500 858 rows x 400 floats: DistMult / TransE k = 400, ComplEx / HolE k = 200
