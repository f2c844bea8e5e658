"""Guard-band buffers: a software red zone around every buffer a C-ABI call is handed.

`guarded(shape, dtype, device, fill, offset=0)` makes ONE uint8 allocation of [band | offset | payload | band] bytes and hands
out the payload as a tensor whose end is exact to the byte: torch's caching allocator rounds every request to 512 bytes and
carves small ones out of shared blocks, so a kernel that writes a few bytes past an ordinary test tensor lands in slack nobody
looks at.  `.check()` asserts that every byte outside the payload still holds its fill.  `guarded_host` is the numpy twin for the
host arrays the session layer fills.

The bands are BAND = 1 MiB on each side -- more than any tile a kernel of this library moves at once.  An access that lands
further away (a wrong 64-bit offset, a row index scaled twice) is OUT OF THIS HARNESS'S REACH: it neither dirties a band nor
reads one.  The harness detects, it never provokes: both fills of a dtype are values that are legal inside the buffer (no NaN,
no word that would be an out-of-range id), so a kernel that over-reads a band does nothing it would not do on an ordinary
tensor -- it only computes something that depends on the fill, which running the same call on fill A and on fill B shows.

Alignment: the payload starts on a 256-byte boundary (what every tensor of the suite has), or `offset` bytes behind one:
workspaces the library aligns itself (d_work / d_screen) are handed over at offset = 16, so the self-alignment slack their
`*_workspace_bytes` functions budget is really consumed.  Where the allocator's base is not itself on a 256-byte boundary (the
host allocators), up to 255 alignment bytes are added in front; they belong to the leading band and are checked with it.
"""
import numpy as np

BAND = 1 << 20

# dtype name -> (fill A, fill B): the word every band element holds
FILLS = {"int32": (0, 1), "int64": (0, 1), "float32": (0.0, 1000.0), "float64": (0.0, 1000.0), "uint8": (0, 1)}


def _np_dtype(dtype):
    """numpy dtype of a torch / numpy dtype or a name"""
    name = str(dtype).replace("torch.", "") if not isinstance(dtype, type) else np.dtype(dtype).name
    if name not in FILLS:
        raise ValueError(f"guarded: no band fill is defined for dtype {dtype!r}")
    return np.dtype(name)


def _fill_word(dtype, fill):
    """the bytes of one band element: fill 'A' / 'B' (or 0 / 1) selects the dtype's word"""
    dt = _np_dtype(dtype)
    which = {"A": 0, "B": 1, 0: 0, 1: 1}[fill]
    return np.array([FILLS[dt.name][which]], dtype=dt).view(np.uint8).copy()


def _nbytes(shape, dt):
    n = dt.itemsize
    for d in (shape if isinstance(shape, (tuple, list)) else (shape,)):
        n *= int(d)
    return n


def _raise_if_dirty(what, lead_bad, tail_bad, lead, nbytes):
    """lead_bad / tail_bad: ascending indices of the dirty bytes inside the leading / trailing band.  The message names the first
    and the last dirty byte as offsets relative to the payload (negative: in front of it; >= nbytes: behind it)."""
    if not len(lead_bad) and not len(tail_bad):
        return
    offs = [int(i) - lead for i in lead_bad] + [nbytes + int(i) for i in tail_bad]
    raise AssertionError(f"guard band of {what} dirty: {len(offs)} byte(s), first at payload offset {offs[0]}, last at payload offset "
                         f"{offs[-1]} (the payload is bytes [0, {nbytes}))")


class Guarded:
    """A device (torch) buffer between two bands.  .tensor: the payload; .check(): both bands intact, bit for bit."""

    def __init__(self, shape, dtype, device, fill, offset=0, name="buffer"):
        import torch

        dt = _np_dtype(dtype)
        self.name, self.fill = name, fill
        self.nbytes = _nbytes(shape, dt)
        if offset < 0 or offset % dt.itemsize:
            raise ValueError("guarded: offset must be a non-negative multiple of the element size")
        self.raw = torch.empty(BAND + offset + self.nbytes + BAND + 255, dtype=torch.uint8, device=device)
        slack = (-self.raw.data_ptr()) % 256          # 0 for torch's device allocator (512-byte aligned blocks)
        self.raw = self.raw[:slack + BAND + offset + self.nbytes + BAND]
        self.lead = slack + BAND + offset
        word = torch.as_tensor(_fill_word(dtype, fill)).to(device)
        # the band elements continue the payload's element grid on both sides (a kernel reads whole elements)
        head = self.lead % dt.itemsize
        self.raw[:head] = word[dt.itemsize - head:] if head else word[:0]
        self.raw[head:self.lead].view(-1, dt.itemsize)[:] = word
        self.raw[self.lead + self.nbytes:].view(-1, dt.itemsize)[:] = word
        self._want_lead = self.raw[:self.lead].clone()
        self._want_tail = self.raw[self.lead + self.nbytes:].clone()
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.tensor = self.raw[self.lead:self.lead + self.nbytes].view(getattr(torch, dt.name)).view(shape)

    def check(self):
        import torch

        lead_bad = torch.nonzero(self.raw[:self.lead] != self._want_lead).flatten()
        tail_bad = torch.nonzero(self.raw[self.lead + self.nbytes:] != self._want_tail).flatten()
        _raise_if_dirty(self.name, lead_bad.cpu().tolist(), tail_bad.cpu().tolist(), self.lead, self.nbytes)


class GuardedHost:
    """The numpy twin: .array (alias .tensor) is the payload, .check() as above."""

    def __init__(self, shape, dtype, fill, offset=0, name="host buffer"):
        dt = _np_dtype(dtype)
        self.name, self.fill = name, fill
        self.nbytes = _nbytes(shape, dt)
        if offset < 0 or offset % dt.itemsize:
            raise ValueError("guarded_host: offset must be a non-negative multiple of the element size")
        raw = np.empty(BAND + offset + self.nbytes + BAND + 255, dtype=np.uint8)
        slack = (-raw.ctypes.data) % 256
        self.raw = raw[:slack + BAND + offset + self.nbytes + BAND]
        self.lead = slack + BAND + offset
        word = _fill_word(dtype, fill)
        head = self.lead % dt.itemsize
        self.raw[:head] = word[dt.itemsize - head:] if head else word[:0]
        self.raw[head:self.lead].reshape(-1, dt.itemsize)[:] = word
        self.raw[self.lead + self.nbytes:].reshape(-1, dt.itemsize)[:] = word
        self._want_lead = self.raw[:self.lead].copy()
        self._want_tail = self.raw[self.lead + self.nbytes:].copy()
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        self.array = self.tensor = self.raw[self.lead:self.lead + self.nbytes].view(dt).reshape(shape)

    def check(self):
        lead_bad = np.flatnonzero(self.raw[:self.lead] != self._want_lead)
        tail_bad = np.flatnonzero(self.raw[self.lead + self.nbytes:] != self._want_tail)
        _raise_if_dirty(self.name, lead_bad.tolist(), tail_bad.tolist(), self.lead, self.nbytes)


def guarded(shape, dtype, device, fill, offset=0, name="buffer"):
    """[band | offset | payload | band] on `device`; fill: 'A' or 'B' (FILLS[dtype]).  -> Guarded (.tensor, .check())."""
    return Guarded(shape, dtype, device, fill, offset, name)


def guarded_host(shape, dtype, fill, offset=0, name="host buffer"):
    """The same in host memory, with numpy.  -> GuardedHost (.array / .tensor, .check())."""
    return GuardedHost(shape, dtype, fill, offset, name)
