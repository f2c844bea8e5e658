#!/usr/bin/env python
"""Record what every *_workspace_bytes function of a libamdkge build returns over a fixed grid of shapes.

    python scripts/record_workspace_sizes.py --lib PATH/libamdkge.so [--out tests/workspace_sizes_parent.json]

tests/workspace_sizes_parent.json is the record of the commit BEFORE the workspace layouts were walked by kge_layout.h;
tests/test_workspace_sizes_host.py (and its GPU twin for the two functions that ask rocPRIM for a size, which needs a device) hold
the current build to it: equal where the old code already walked its plan (group A), never larger where it used a hand formula (group
B).  The grid: the shapes of the guard-band case tables (tests/test_gpu_guard_bands.py and the tests/test_gpu_*_guard.py files), the
BASELINE.json configurations, and the edges -- 0, 1, the refusing sizes, the largest accepted sizes.

The file: {"functions": {fn: {"group", "device"}}, "models": [[scoring_type, k, n_ents, n_rels, max_rel_size, k_pad, k_full], ...],
"rows": [[fn, index into models or null, [[args, value], ...]], ...]} -- one line per function and model.  The values of a function
that needs a device are null when recorded on a machine without a GPU."""
import argparse
import ctypes as C
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {"TransE": 0, "DistMult": 1, "ComplEx": 2, "HolE": 3, "RotatE": 4}
I64, I32 = C.c_int64, C.c_int32


class Model(C.Structure):   # include/amdkge.h
    _fields_ = [("scoring_type", I32), ("k", I32), ("n_ents", I64), ("n_rels", I64), ("max_rel_size", I32), ("k_pad", I32), ("k_full", I32),
                ("reserved_", I32)]


# fn -> (group, needs a device, takes a model, types of the other arguments)
FUNCTIONS = {
    "amdkge_train_tiled_workspace_bytes": ("A", False, True, [I64, I32]),
    "amdkge_train_shared_workspace_bytes": ("A", False, True, [I64, I64, I32]),
    "amdkge_train_shared_dist_workspace_bytes": ("A", False, True, [I64, I64, I32]),
    "amdkge_train_relation_workspace_bytes": ("A", False, True, [I64]),
    "amdkge_filter_build_workspace_bytes": ("A", True, False, [I64, I64, I64]),
    "amdkge_step_rows_workspace_bytes": ("A", True, False, [I64, I64]),
    "amdkge_kmeans_workspace_bytes": ("A", False, False, [I64, I32, I32, I32]),
    "amdkge_join_dbscan_workspace_bytes": ("A", False, False, [I64]),
    "amdkge_rank_workspace_bytes": ("B", False, True, [I64]),
    "amdkge_rank_lists_workspace_bytes": ("B", False, True, [I64]),
    "amdkge_rank_screen_workspace_bytes": ("B", False, True, [I64, I64]),
    "amdkge_relation_workspace_bytes": ("B", False, True, [I64]),
    "amdkge_shard_route_workspace_bytes": ("B", False, False, [I64, I64]),
}


def model(name, k, N, R, pad=True, k_full=0):
    return [TYPES[name], k, N, R, R, (k + 3) // 4 * 4 if pad else 0, k_full]


def grid():
    """-> [(fn, model or None, args)], in a fixed order"""
    rows = []
    # the guard-band tables' models at their table sizes, and the BASELINE.json configurations (FB15K-237, WN18RR, YAGO3-10, one
    # GPU's shard of the 50 M-entity graph)
    small = [model(n, k, 130, 4, pad) for n, k, pad in (
        ("ComplEx", 50, True), ("TransE", 7, False), ("TransE", 7, True), ("RotatE", 350, True), ("DistMult", 200, True), ("HolE", 516, True),
         ("ComplEx", 16, True), ("RotatE", 12, True), ("DistMult", 12, True), ("DistMult", 50, True), ("ComplEx", 200, True), ("HolE", 350, True),
         ("RotatE", 50, True), ("TransE", 200, True), ("TransE", 50, True), ("TransE", 64, True), ("RotatE", 64, True), ("DistMult", 7, False),
         ("HolE", 200, True), ("ComplEx", 7, False))]
    base = [model("TransE", 50, 14505, 237), model("ComplEx", 200, 14505, 237), model("DistMult", 400, 40943, 11),
            model("ComplEx", 200, 123182, 37), model("RotatE", 1000, 6250000, 1000), model("RotatE", 1000, 50000000, 1000)]
    edge = [model("ComplEx", 200, 1, 1), model("TransE", 2048, 2 ** 31 - 1, 2 ** 31 - 1), model("RotatE", 2048, 2 ** 31 - 1, 1),
            model("DistMult", 2052, 1000, 5), model("ComplEx", 50, 0, 5), model("ComplEx", 0, 100, 5), [7, 50, 100, 5, 5, 52, 0]]
    models = small + base + edge
    for m in models:
        for B, eta in [(37, 5), (3000, 2), (2000, 3), (10000, 20), (10000, 5), (10000, 30), (8192, 20), (65536, 64), (0, 1), (1, 1), (-1, 5), (37, 0),
                       (2 ** 30 - 1, 1), (2 ** 30, 1), (2 ** 26, 30), (100, 100000)]:
            rows.append(("amdkge_train_tiled_workspace_bytes", m, [B, eta]))
        for B, G, M in [(37, 5, 33), (37, 5, 65), (37, 500, 33), (37, 5, 23), (1, 1, 1), (10000, 100, 1000), (10000, 10000, 14505), (8192, 64, 123182),
                        (700000, 1000, 2 ** 24 - 1), (0, 5, 33), (37, 0, 33), (37, 5, 0), (37, 5, 2 ** 24), (2 ** 40, 2 ** 40, 2), (2 ** 31, 1, 2 ** 24 - 1)]:
            rows.append(("amdkge_train_shared_workspace_bytes", m, [B, G, M]))   # (a model takes one of the two; the other returns 0)
            if (B, G, M) in ((37, 5, 33), (37, 500, 33), (1, 1, 1), (10000, 100, 1000), (0, 5, 33), (37, 5, 2 ** 24)):   # (the same plan)
                rows.append(("amdkge_train_shared_dist_workspace_bytes", m, [B, G, M]))
        for B in [37, 700000, 1, 0, -1, 10000, 8192, 2 ** 31]:
            rows.append(("amdkge_train_relation_workspace_bytes", m, [B]))
        for n in [37, 1, 130, 200, 70, 0, -1, 1023, 1024, 1025, 2048, 10000, 20466, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 40]:
            rows.append(("amdkge_rank_workspace_bytes", m, [n]))
            if n in (37, 0, -1, 10000, 2 ** 31 - 1):   # (forwards to the rank workspace)
                rows.append(("amdkge_rank_lists_workspace_bytes", m, [n]))
        for n, c in [(130, 523), (130, 531), (200, 531), (70, 262), (70, 270), (0, 0), (1, 1), (0, 100), (100, 0), (-1, 5), (5, -1), (2048, 14505),
                     (20466, 14505), (3134, 40943), (5000, 123182), (1024, 6250000), (300, 4000), (2 ** 31 - 2, 2 ** 31 - 2), (2 ** 20, 2 ** 31 - 1)]:
            rows.append(("amdkge_rank_screen_workspace_bytes", m, [n, c]))
        for c in [9, 130, 0, 1, -1, 237, 1000, 2 ** 31 - 16, 7]:
            rows.append(("amdkge_relation_workspace_bytes", m, [c]))
    for m_, N, R in [(37, 23, 5), (130, 23, 5), (1, 23, 5), (0, 23, 5), (-1, 23, 5), (37, 0, 5), (37, 23, 0), (272115, 14505, 237), (1079040, 123182, 37),
                     (2 ** 32 - 1, 14505, 237), (1000, 2 ** 31 - 1, 2), (257, 130, 9)]:
        rows.append(("amdkge_filter_build_workspace_bytes", None, [m_, N, R]))
    for N, keys in [(130, 138), (130, 2), (130, 1), (97, 857), (100000, 4097), (130, 0), (0, 5), (130, -1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31, 5), (5, 2 ** 31),
                    (14505, 20000 + 14505), (123182, 16384 + 123182)]:
        rows.append(("amdkge_step_rows_workspace_bytes", None, [N, keys]))
    for a in [(130, 7, 3, 2), (257, 52, 37, 1), (257, 9, 130, 1), (0, 7, 3, 2), (1, 1, 1, 1), (-1, 7, 3, 2), (130, 0, 3, 2), (130, 7, 0, 2), (130, 7, 3, 0),
              (14505, 400, 50, 10), (123182, 400, 1000, 4), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1),
              (2 ** 31 - 1, 2 ** 20, 2 ** 20, 2 ** 10), (2 ** 31 - 1, 4096, 4096, 64), (2 ** 31, 7, 3, 2)]:
        rows.append(("amdkge_kmeans_workspace_bytes", None, list(a)))
    for n in [130, 257, 0, 1, -1, 14505, 2 ** 31 - 1, 2 ** 31]:
        rows.append(("amdkge_join_dbscan_workspace_bytes", None, [n]))
    for b, g in [(37, 0), (37, 111), (130, 0), (0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (255, 0), (256, 0), (257, 0), (10000, 200000), (8192, 163840), (65536, 4194304),
                 (2 ** 27, 2 ** 27 - 1), (2 ** 27, 2 ** 27), (2 ** 28 - 1, 0), (2 ** 28, 0)]:
        rows.append(("amdkge_shard_route_workspace_bytes", None, [b, g]))
    return rows


def bind(path):
    lib = C.CDLL(path)
    for fn, (_, _, takes_model, args) in FUNCTIONS.items():
        f = getattr(lib, fn)
        f.restype = I64
        f.argtypes = ([C.POINTER(Model)] if takes_model else []) + args
    lib.amdkge_device_count.restype = I32
    lib.amdkge_device_count.argtypes = [C.POINTER(I32)]
    return lib


def call(lib, fn, m, args):
    if FUNCTIONS[fn][2]:
        mm = Model(*m, 0)
        return int(getattr(lib, fn)(C.byref(mm), *args))
    return int(getattr(lib, fn)(*args))


def have_device(lib):
    n = I32(0)
    return lib.amdkge_device_count(C.byref(n)) == 0 and n.value > 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the libamdkge.so to record")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "workspace_sizes_parent.json"))
    a = ap.parse_args()
    lib = bind(a.lib)
    dev = have_device(lib)
    models, out, n = [], {}, 0
    for fn, m, args in grid():
        if m is not None and m not in models:
            models.append(m)
        out.setdefault((fn, None if m is None else models.index(m)), []).append([args, call(lib, fn, m, args) if dev or not FUNCTIONS[fn][1] else None])
        n += 1
    out = [[fn, mi, cases] for (fn, mi), cases in out.items()]
    with open(a.out, "w") as f:
        f.write('{"functions": ' + json.dumps({fn: {"group": g, "device": d} for fn, (g, d, _, _) in FUNCTIONS.items()}) + ',\n"models": ' + json.dumps(models) +
                ',\n"rows": [\n' + ",\n".join(json.dumps(r) for r in out) + "\n]}\n")
    print(f"{n} shapes -> {a.out}" + ("" if dev else " (no device: the rows that need one hold null)"))


if __name__ == "__main__":
    main()
