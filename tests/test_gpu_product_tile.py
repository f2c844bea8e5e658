"""The one product tile (kge_product_tile.h) under its two kernels, shared_gemm_kernel and relpred_gemm_kernel, at the smallest shapes
at which a tile can go wrong.  The FWD products are deterministic (one wave sums each output in a fixed order), so the scores of a
build must equal, bit for bit, those that scripts/record_product_tile_scores.py recorded from the commit BEFORE the two kernels
were rewritten on the shared pieces (tests/golden/product_tile_scores_v1.npz names that commit).  The gradients go through atomics:
they and the loss are held to the references with the bars of test_gpu_shared.py / test_gpu_relation_objective.py.

Shapes that those two files do not run (they have K = 7 for DistMult, R = 65 padded, R = 1 and B = 37 already):
  one short tile (B = G = 5, M = 1); an edge in every dimension (B = 70, G = 33: a short last group, M = 65: one column in the second
  tile); 2 ks = 16 with k = 5 (ComplEx, padded) and dense rows of k = 7; the relation objective at R = 1 / 65 with B = 70 and at
  B = 513, R = 3 (DREL's second slice holds one row); one ComplEx case per entry point with an inf in an entity row (the
  reference-order rescoring of a non-finite product; bits only -- the non-finite sets are test_gpu_nonfinite_shared.py's and
  test_gpu_relation_objective.py::test_nonfinite_sets')."""
import os

import numpy as np
import pytest

import shared_ref as SR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "product_tile_scores_v1.npz")
MODELS = ("DistMult", "ComplEx")
ROWS = ((5, True), (7, False))                       # (k, pad): k = 5 stored as 8; dense rows of 7
SHARED_SHAPES = ((5, 5, 1), (70, 33, 65))            # (B, G, M)
RELATION_SHAPES = ((1, 70), (65, 70), (3, 513))      # (R, B)
N_ENTS, N_RELS_SHARED = 90, 4


def cases():
    """-> [(name, entry, model, k, pad, shape, plant_inf, seed)]; the seed of a case is its position"""
    out = []
    for model in MODELS:
        for k, pad in ROWS:
            row = f"{model}-k{k}{'p' if pad else 'd'}"
            out += [(f"shared-{row}-B{B}G{G}M{M}", "shared", model, k, pad, (B, G, M), False) for B, G, M in SHARED_SHAPES]
            out += [(f"relation-{row}-R{R}B{B}", "relation", model, k, pad, (R, B), False) for R, B in RELATION_SHAPES]
    out += [("shared-ComplEx-k5p-B70G33M65-inf", "shared", "ComplEx", 5, True, (70, 33, 65), True),
            ("relation-ComplEx-k5p-R65B70-inf", "relation", "ComplEx", 5, True, (65, 70), True)]
    return [c + (100 + i,) for i, c in enumerate(out)]


def inputs(entry, model, k, pad, shape, plant_inf, seed):
    """-> (engine, ent, rel, X, ids, side); ids / side are None for the relation objective"""
    from ampligraph_amd.engine import KgeEngine
    from oracle import kge_oracle as O
    from test_gpu_kernels import rand_triples

    R = N_RELS_SHARED if entry == "shared" else shape[0]
    B = shape[0] if entry == "shared" else shape[1]
    rng = np.random.default_rng(seed)
    K = O.internal_k(model, k)
    ent = (rng.normal(size=(N_ENTS, K)) * 0.5).astype(np.float32)
    rel = (rng.normal(size=(R, K)) * 0.5).astype(np.float32)
    X = rand_triples(rng, B, N_ENTS, R)
    ids = side = None
    if entry == "shared":
        ids, side = SR.sample_shared(X, shape[1], shape[2], seed, 3, sample_range=N_ENTS)
    if plant_inf:   # an entity that is scored: a list entry of the first group / the first positive's subject
        ent[int(ids[0, 0]) if entry == "shared" else int(X[0, 0]), 1] = np.inf
    eng = KgeEngine(model, k, N_ENTS, R, max_rel_size=R, pad=pad)
    eng.set_tables(ent, rel)
    return eng, ent, rel, X, ids, side


LOSS, REDUCTION, WEIGHT = "multiclass_nll", "sum", 0.25


def run(entry, eng, X, shape, ids, side):
    """-> (loss sum, dense entity gradient, dense relation gradient, positive scores, corruption / relation scores)"""
    from test_gpu_relation_objective import run_step
    from test_gpu_shared import run_shared

    if entry == "shared":
        return run_shared(eng, X, shape[1], ids, side, LOSS, REDUCTION)
    return run_step(eng, X, LOSS, REDUCTION, WEIGHT, None)[0]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_golden_file_holds_exactly_these_cases(golden):
    names = {c[0] for c in cases()}
    assert {k.split("/")[0] for k in golden.files if not k.startswith("meta_")} == names
    assert str(golden["meta_script"]) == "scripts/record_product_tile_scores.py" and len(str(golden["meta_parent_commit"])) == 40
    for name, *_, seed in cases():
        assert int(golden[name + "/seed"]) == seed


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_scores_equal_the_recorded_bits_and_gradients_the_reference(gpu_lib, golden, case):
    from test_gpu_relation_objective import check_against_step
    from test_gpu_shared import check_against_oracle

    name, entry, model, k, pad, shape, plant_inf, seed = case
    eng, ent, rel, X, ids, side = inputs(entry, model, k, pad, shape, plant_inf, seed)
    got = run(entry, eng, X, shape, ids, side)
    for what, a in (("pos_scores", got[3]), ("scores", got[4])):
        want = golden[f"{name}/{what}"]
        assert a.dtype == np.float32 and a.shape == want.shape
        differ = np.flatnonzero(a.view(np.uint32) != want.view(np.uint32))
        assert differ.size == 0, (what, differ[:5], a[differ[:5]], want[differ[:5]])
    if plant_inf:   # the rescoring ran: non-finite scores are there, and their bits are the recorded ones
        assert not np.isfinite(got[4]).all()
        return
    if entry == "shared":
        check_against_oracle(model, ent, rel, X, shape[1], ids, side, got, LOSS, REDUCTION, rel.shape[0], tag=name)
    else:
        R, B = shape
        check_against_step(model, ent, rel, X, np.zeros((B, R), dtype=bool), got, LOSS, REDUCTION, WEIGHT, tag=name, cancelling=R == 1)
    if pad:   # the padding floats of both gradient tables were never written
        for t in (eng.g_ent, eng.g_rel):
            assert not t.cpu().numpy().reshape(t.shape[0], -1, eng.ks)[:, :, eng.k:].any()
