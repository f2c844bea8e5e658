#!/usr/bin/env python3
"""Records tests/golden/product_tile_scores_v1.npz: the pos_scores / neg_scores (rel_scores) outputs of amdkge_train_shared_fwdbwd and
amdkge_train_relation_fwdbwd on the seeded cases of tests/test_gpu_product_tile.py, from a library built from the commit BEFORE
shared_gemm_kernel and relpred_gemm_kernel were rewritten on kge_product_tile.h.  The FWD products are deterministic, so a later
build must reproduce these floats bit for bit; the test asserts it.

Build that commit's library with the project's Makefile into a directory of its own (OBJDIR=... OUT=.../libamdkge.so), then

    AMDKGE_LIB=.../libamdkge.so python scripts/record_product_tile_scores.py --parent-commit <its 40-digit hash> [--out FILE]

on a machine with a GPU.  Per case the file holds `<name>/seed`, `<name>/pos_scores`, `<name>/scores`; `meta_script` and
`meta_parent_commit` say where it came from.  The C ABI and the Python layer did not change with the rewrite, so the cases run
through this tree's binding."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "product_tile_scores_v1.npz"))
    a = ap.parse_args()
    if len(a.parent_commit) != 40 or not os.environ.get("AMDKGE_LIB"):
        sys.exit("record_product_tile_scores: needs the parent's full hash and AMDKGE_LIB = the library built from it")
    import test_gpu_product_tile as T

    out = {"meta_script": np.array("scripts/record_product_tile_scores.py"), "meta_parent_commit": np.array(a.parent_commit)}
    for name, entry, model, k, pad, shape, plant_inf, seed in T.cases():
        eng, ent, rel, X, ids, side = T.inputs(entry, model, k, pad, shape, plant_inf, seed)
        got = T.run(entry, eng, X, shape, ids, side)
        out[name + "/seed"] = np.int64(seed)
        out[name + "/pos_scores"], out[name + "/scores"] = got[3], got[4]
        print(f"{name}: {got[3].size} + {got[4].size} floats, {int((~np.isfinite(got[4])).sum())} non-finite")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
