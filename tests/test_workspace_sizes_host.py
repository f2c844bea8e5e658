"""What the *_workspace_bytes functions return, held to the record of the commit before the workspace layouts were walked by
ampligraph_amd/csrc/kge_layout.h (tests/workspace_sizes_parent.json, written by scripts/record_workspace_sizes.py from a build of that
commit; its grid: the guard-band tables' shapes, the BASELINE.json configurations, 0, 1, the refusing and the largest accepted sizes).
  group A  the old code already walked a plan (tiled, shared, relation objective, filter build, step rows, KMeans, DBSCAN): EQUAL for
           every shape, the 0 and -1 refusals included;
  group B  the old code was a hand formula beside a pointer walk (rank, rank lists, screening / early exit, relation scores, shard
           route): what the walk needs for a base of any alignment, NEVER MORE than the record (the guard-band tests, which hand every
           workspace over at exactly the returned size 16 bytes behind a 256-byte boundary, hold it from below).
No GPU needed: the size functions are host arithmetic -- except the two that ask rocPRIM for its scratch size, which needs a device:
their rows are checked by tests/test_gpu_workspace_sizes.py from the same table."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "workspace_sizes_parent.json")) as _f:
    TABLE = json.load(_f)
HOST_FUNCTIONS = sorted(fn for fn, d in TABLE["functions"].items() if not d["device"])
DEVICE_FUNCTIONS = sorted(fn for fn, d in TABLE["functions"].items() if d["device"])


def check_function(lib, fn):
    """every recorded row of fn against the loaded library -> the number of rows checked"""
    from ampligraph_amd import _ffi

    group = TABLE["functions"][fn]["group"]
    rows = [(mi, args, want) for name, mi, cases in TABLE["rows"] if name == fn for args, want in cases]
    assert len(rows) >= 8 and all(r[2] is not None for r in rows), fn
    f = getattr(lib, fn)
    for mi, args, want in rows:
        if mi is None:
            got = int(f(*args))
        else:
            m = _ffi.Model(*TABLE["models"][mi], 0)
            got = int(f(C.byref(m), *args))
        if group == "A":
            assert got == want, (fn, TABLE["models"][mi] if mi is not None else None, args, got, want)
        else:
            assert got <= want, (fn, TABLE["models"][mi] if mi is not None else None, args, got, want)
            assert (got < 0) == (want < 0) or got == -1, (fn, args, got, want)   # a refusal stays one; an overflow is reported as -1
    return len(rows)


@pytest.mark.parametrize("fn", HOST_FUNCTIONS)
def test_sizes_against_the_record(fn):
    from ampligraph_amd import _ffi

    assert check_function(_ffi.lib(), fn) > 0


def test_the_record_covers_every_size_function():
    from ampligraph_amd import _ffi

    bound = {name for table in list(_ffi.ABI.values()) + list(_ffi.ABI_EXT.values()) for name in table if name.endswith("_workspace_bytes")}
    assert len(bound) == 13 and bound == set(TABLE["functions"])
    assert len(HOST_FUNCTIONS) == 11 and len(DEVICE_FUNCTIONS) == 2
    assert {d["group"] for d in TABLE["functions"].values()} == {"A", "B"}
