"""The guard-band harness itself (tests/guarded.py) and the coverage of include/amdkge.h by the case table of
tests/test_gpu_guard_bands.py -- no GPU needed."""
import numpy as np
import pytest
import torch

from abi_decl import declared_names
from guarded import BAND, FILLS, guarded, guarded_host

# Entry points without a guard-band case, each with its reason.  Everything else the header declares must be a key of CASES.
EXEMPT = {
    "amdkge_abi_version": "no pointer argument",
    "amdkge_last_error": "returns a string the library owns",
    "amdkge_device_count": "writes one host int",
    "amdkge_release_scratch": "no argument",
    "amdkge_set_device": "no pointer argument",
    "amdkge_dev_alloc": "allocator: hands out memory, computes nothing",
    "amdkge_dev_free": "allocator",
    "amdkge_h2d": "a hipMemcpy of the byte count it is given",
    "amdkge_d2h": "a hipMemcpy of the byte count it is given",
    "amdkge_dev_memset": "a hipMemset of the byte count it is given",
    "amdkge_stream_sync": "no pointer argument",
    "amdkge_internal_k": "host arithmetic",
    "amdkge_padded_k": "host arithmetic",
    "amdkge_row_floats": "host arithmetic on the descriptor",
    "amdkge_set_tile_direct": "process-wide switch (exercised by the tiled-step cases)",
    "amdkge_set_rank_kernel": "process-wide switch (exercised by the rank-count cases)",
    "amdkge_set_rank_rotate_fast": "process-wide switch, no pointer argument",
    "amdkge_set_rank_early": "process-wide switch (exercised by the screened rank-count cases)",
    "amdkge_train_tiled_workspace_bytes": "size function: every tiled-step case allocates exactly what it returns",
    "amdkge_rank_workspace_bytes": "size function: the rank / filter / corruption-score cases allocate exactly what it returns",
    "amdkge_rank_screen_workspace_bytes": "size function: the screened rank-count cases allocate exactly what it returns",
    "amdkge_filter_build_workspace_bytes": "size function: the filter-build cases allocate exactly what it returns",
    "amdkge_join_dbscan_workspace_bytes": "size function: the DBSCAN cases allocate exactly what it returns",
    "amdkge_kmeans_workspace_bytes": "size function: the Lloyd cases allocate exactly what it returns",
    "amdkge_relation_workspace_bytes": "size function: the relation-score cases allocate exactly what it returns",
    "amdkge_shard_route_workspace_bytes": "size function: the routing cases allocate exactly what it returns",
    "amdkge_train_tiled_status": "reads one flag of the workspace into a host int; synchronises",
    "amdkge_session_create": "session life cycle: the library owns every device buffer",
    "amdkge_session_destroy": "session life cycle",
    "amdkge_session_set_rows": "reads a host array, writes library-owned memory",
    "amdkge_session_train_step": "reads host arrays, writes one host double",
    "amdkge_session_set_hot_rows": "reads a host id list",
    "amdkge_session_screen_stats": "writes three host scalars",
    "amdkge_session_group_create": "group life cycle",
    "amdkge_session_group_create_ex": "group life cycle",
    "amdkge_session_group_create_rows": "group life cycle",
    "amdkge_session_group_create_cols": "group life cycle",
    "amdkge_session_group_destroy": "group life cycle",
    "amdkge_session_group_info": "writes two host scalars",
    "amdkge_session_group_size": "no pointer argument besides the handle",
    "amdkge_session_group_replica": "hands out a handle",
    "amdkge_session_group_set_rows": "reads a host array, writes library-owned memory",
    "amdkge_session_group_train_step": "reads host arrays, writes one host double",
    "amdkge_session_group_route_overflow": "writes one host int",
}


def _raises_naming(fn, *offsets):
    with pytest.raises(AssertionError) as e:
        fn()
    for off in offsets:
        assert f"payload offset {off}" in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype", sorted(FILLS))
@pytest.mark.parametrize("fill", ["A", "B"])
def test_harness_detects_one_byte_on_either_side(dtype, fill):
    """An untouched buffer passes; one byte written at payload_end, and separately at payload_start - 1, through an oversized view fails
    with the offset in the message.  The written value differs from the band's byte at that place whatever the fill."""
    shape = (37, 5)
    for make in (lambda: guarded(shape, dtype, "cpu", fill, offset=16), lambda: guarded_host(shape, dtype, fill)):
        g = make()
        nbytes = 37 * 5 * np.dtype(dtype).itemsize
        assert g.nbytes == nbytes and tuple(g.tensor.shape) == shape
        g.tensor[...] = 3                                   # writing the whole payload is what a call does
        g.check()
        end = g.lead + nbytes                               # g.raw is the oversized view: the whole allocation
        old = int(g.raw[end])
        g.raw[end] = old ^ 0x40
        _raises_naming(g.check, nbytes)
        g.raw[end] = old
        g.check()
        old = int(g.raw[g.lead - 1])
        g.raw[g.lead - 1] = old ^ 0x40
        _raises_naming(g.check, -1)
        g.raw[g.lead - 1] = old
        g.check()
        g.raw[0] ^= 0x01                                    # the far ends of both bands, together: first and last are both named
        g.raw[-1] ^= 0x01
        _raises_naming(g.check, -g.lead, nbytes + BAND - 1)


def test_exact_sizes_and_alignment():
    g = guarded((37, 130), torch.float32, "cpu", "A")
    t = g.tensor
    assert t.dtype == torch.float32 and tuple(t.shape) == (37, 130) and t.numel() * t.element_size() == 19240 == g.nbytes
    assert t.data_ptr() % 256 == 0
    assert g.raw.numel() - g.lead - g.nbytes == BAND == 1 << 20 and g.lead >= BAND       # the end is exact to the byte
    assert g.raw.data_ptr() + g.lead == t.data_ptr()
    w = guarded((37, 130), torch.float32, "cpu", "B", offset=16)
    assert w.tensor.data_ptr() % 256 == 16 and w.nbytes == 19240
    h = guarded_host((37, 130), np.float32, "A", offset=16)
    assert h.array.ctypes.data % 256 == 16 and h.array.nbytes == 19240 and h.array.shape == (37, 130)
    # the bands hold whole elements of the payload's type, both fills legal values of it
    for dtype, (a, b) in FILLS.items():
        for fill, want in (("A", a), ("B", b)):
            g = guarded_host((3,), dtype, fill)
            tail = g.raw[g.lead + g.nbytes:].view(dtype)
            head = g.raw[g.lead % np.dtype(dtype).itemsize:g.lead].view(dtype)
            assert (tail == want).all() and (head == want).all() and np.isfinite(float(want))
    with pytest.raises(ValueError):
        guarded((3,), torch.float16, "cpu", "A")


def test_every_header_entry_has_a_case_or_a_reason():
    """A new ABI entry cannot arrive without a guard-band case or a stated reason.  (The case table is data: importing it needs no GPU.)"""
    from test_gpu_guard_bands import CASES
    import test_gpu_guard_bands as G

    declared = declared_names("amdkge.h")
    assert len(declared) > 80, "no declarations parsed"
    assert not set(CASES) & set(EXEMPT), set(CASES) & set(EXEMPT)
    assert not (set(CASES) | set(EXEMPT)) - declared, (set(CASES) | set(EXEMPT)) - declared        # no stale names
    missing = declared - set(CASES) - set(EXEMPT)
    assert not missing, f"no guard-band case and no exemption for: {sorted(missing)}"
    for reason in EXEMPT.values():
        assert reason and "\n" not in reason
    for entry, cases in CASES.items():
        assert cases, entry
        for fn, kw in cases:
            assert callable(getattr(G, "case_" + fn)), (entry, fn)
