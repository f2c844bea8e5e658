"""Relation prediction at the FB15K-237 test shape (n = 20 438 query pairs, R = 237 relations, N = 14 505 entities, k = 200):
(a) the only route to the (n, R) relation scores before amdkge_relation_scores -- build the n x R id triples on the device, then
    amdkge_score --,
(b) engine.relation_scores (amdkge_relation_scores),
(c) the whole evaluate_relations (filtered with the training set) and query_topn_relations (filtered, top 10) calls.
One process; the tables are the ones a one-epoch fit on a uniform-random graph leaves.  (a) and (b) alternate inside every
repetition, each timed by device events around `--inner` back-to-back calls; (c) by a host clock around synchronised calls.  After
warm-up, `--reps` repetitions: min / median / max of each, the ratio of the medians, whether the slowest (b) is below the fastest
(a), and (b)'s achieved bytes/s for the bytes its algorithm moves (computed from the shape below).  The two score blocks are
compared bit for bit before anything is timed.  Writes profiles/relation_timing_<model>_k<k>.json and prints the same JSON line.

    python scripts/relation_timing.py [--model ComplEx] [--k 200] [--reps 12] [--inner 5] [--out profiles/...json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ampligraph_amd import discovery  # noqa: E402
from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel  # noqa: E402


def stats(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ComplEx")
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--n-ents", type=int, default=14505)
    ap.add_argument("--n-rels", type=int, default=237)
    ap.add_argument("--n-triples", type=int, default=272115)
    ap.add_argument("--queries", type=int, default=20438)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("relation_timing.py measures on a GPU: none found")
    rng = np.random.default_rng(0)
    N, R, nt, n = a.n_ents, a.n_rels, a.n_triples, a.queries
    X = np.stack([rng.integers(0, N, nt), rng.integers(0, R, nt), rng.integers(0, N, nt)], 1)
    X[:N, 0] = np.arange(N)          # every entity and relation occurs
    X[:R, 1] = np.arange(R)
    m = ScoringBasedEmbeddingModel(eta=2, k=a.k, scoring_type=a.model, seed=0)
    m.compile(optimizer="adam", loss="nll")
    m.fit(X, batch_size=30000, epochs=1, verbose=False)
    T = X[rng.choice(nt, n, replace=False)]
    eng = m._engine
    Xd = torch.as_tensor(m.data_indexer.get_indexes(T)).to(eng.device)
    rel = torch.arange(R, dtype=torch.int32, device=eng.device)

    def parents_way():
        tri = torch.empty(n, R, 3, dtype=torch.int32, device=eng.device)
        tri[:, :, 0] = Xd[:, 0:1]
        tri[:, :, 1] = rel[None, :]
        tri[:, :, 2] = Xd[:, 2:3]
        return eng.score(tri.view(-1, 3)).view(n, R)

    out = torch.empty(n, R, dtype=torch.float32, device=eng.device)

    def kernel():
        return eng.relation_scores(Xd, out=out)

    same = bool(torch.equal(parents_way().view(torch.int32), kernel().view(torch.int32)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / a.inner

    for _ in range(3):
        timed(parents_way), timed(kernel)
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(timed(parents_way))
        tb.append(timed(kernel))

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    ev = lambda: m.evaluate_relations(T, use_filter={"train": X})   # noqa: E731
    qt = lambda: discovery.query_topn_relations(m, T[:, [0, 2]], top_n=a.top_n, use_filter={"train": X})   # noqa: E731
    wall(ev), wall(qt)
    t_ev = [wall(ev) for _ in range(a.reps)]
    t_qt = [wall(qt) for _ in range(a.reps)]

    # bytes (b) moves, from the shape: every query's s and o row once, the relation table once per group of queries that share a
    # wave (kge_relation.hip: QPW by the width), the score block once.  The relation reads are L2 traffic (the table is R rows).
    Ks = int(eng.Ks)
    nc = Ks // int(eng.ks)
    nit = -(-(int(eng.ks) // 4) // 64)
    qpw = 4 if nit * 8 * nc <= 16 else (2 if nit * 8 * nc <= 32 else 1)
    b_rel = -(-n // qpw) * R * Ks * 4
    b_hbm = 2 * n * Ks * 4 + n * R * 4 + R * Ks * 4
    sa, sb = stats(ta), stats(tb)
    res = {"model": a.model, "k": a.k, "n_ents": N, "n_rels": R, "queries": n, "reps": a.reps, "inner": a.inner,
           "bits_equal": same,
           "materialise_then_amdkge_score_s": sa, "relation_scores_s": sb,
           "ratio_of_medians": sa["median"] / sb["median"], "slowest_b_below_fastest_a": sb["max"] < sa["min"],
           "queries_per_wave": qpw, "relation_row_bytes_from_l2": b_rel, "relation_row_bytes_per_s": b_rel / sb["median"],
           "compulsory_bytes": b_hbm, "compulsory_bytes_per_s": b_hbm / sb["median"],
           "parents_way_bytes": n * R * (3 * Ks * 4 + 12 + 4) + n * R * 12, "evaluate_relations_s": stats(t_ev),
           "query_topn_relations_s": stats(t_qt), "top_n": a.top_n}
    line = json.dumps(res)
    path = a.out or os.path.join(ROOT, "profiles", "relation_timing_{}_k{}.json".format(a.model, a.k))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
