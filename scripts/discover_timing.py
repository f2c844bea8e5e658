"""Wall time of discover_facts(strategy="exhaustive") for ONE relation at the headline shape (FB15K-237's sizes: N = 14 541 entities,
237 relations, 272 115 triples; ComplEx k = 200), beside the only other route to the same answer: evaluate() over every candidate
row, timed on the full candidate rows of a fixed sample of 64 subjects and scaled to N subjects.  The graph is uniform-random and
the tables are the ones a one-epoch fit leaves (nothing to learn in a random graph; bench.py's planted "trained-like" tables exist
for the distance models only).  Warm-up, then the median of repeated runs (host clock around synchronised calls).  Prints one JSON
line: both times, the phase split of the exhaustive path, the survivor counts after each phase and the derived margin_q.

    python scripts/discover_timing.py [--reps 5] [--top-n 10] [--model ComplEx] [--k 200]"""
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


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--model", default="ComplEx")
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--n-ents", type=int, default=14541)
    ap.add_argument("--n-rels", type=int, default=237)
    ap.add_argument("--n-triples", type=int, default=272115)
    ap.add_argument("--subjects", type=int, default=64)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    N, R, n = a.n_ents, a.n_rels, a.n_triples
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1)
    X[:N, 0] = np.arange(N)          # every entity and relation occurs
    X[:R, 1] = np.arange(R)
    m = ScoringBasedEmbeddingModel(eta=2, k=a.k, scoring_type=a.model, seed=0)
    m.compile(optimizer="adam", loss="multiclass_nll")
    m.fit(X, batch_size=30000, epochs=1, verbose=False)
    rel = [X[0, 1]]
    r_id = int(m.data_indexer.get_indexes(np.asarray(rel), "r")[0])

    def exhaustive(stats=None):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = discovery._discover_exhaustive(X, m, a.top_n, rel, stats=stats)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    exhaustive()                                                       # warm-up (filter index, workspaces)
    total = median([exhaustive()[0] for _ in range(a.reps)])
    phases = []
    for _ in range(a.reps):                                            # the phase split needs a synchronisation per phase: timed apart
        st = {}
        exhaustive(st)
        phases.append(st["relations"][0])
    split = {k_: median([p[k_] for p in phases]) for k_ in ("t_score_select", "t_intersect", "t_exact_ranks")}
    counts = {k_: phases[0][k_] for k_ in ("R", "margin_q", "emitted_o", "emitted_s", "survivors", "found")}

    # the parent's route: every candidate row of a sample of subjects through evaluate()
    ix = m.data_indexer
    subj = np.sort(rng.choice(N, a.subjects, replace=False))
    s, o = np.meshgrid(subj, np.arange(N), indexing="ij")
    cand = np.stack([s.ravel(), np.full(s.size, r_id), o.ravel()], 1)
    cand = ix.get_indexes(cand[cand[:, 0] != cand[:, 2]], "t", "ind2raw")

    def brute():
        torch.cuda.synchronize()
        t = time.perf_counter()
        ranks = m.evaluate(cand, use_filter={"test": X}, corrupt_side="s,o", verbose=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t, ranks

    brute()
    t_brute = median([brute()[0] for _ in range(a.reps)])
    ranks = brute()[1]
    # (rows of X among the sampled candidates rank as evaluate() ranks them; they are not candidates of the exhaustive strategy)
    print(json.dumps({"model": a.model, "k": a.k, "n_ents": N, "n_rels": R, "n_triples": n, "top_n": a.top_n, "reps": a.reps,
                      "exhaustive_one_relation_s": total, "phases_s": split, **counts,
                      "candidates_per_relation": N * (N - 1), "evaluate_sampled_subjects": a.subjects, "evaluate_sampled_rows": int(len(cand)),
                      "evaluate_sampled_s": t_brute, "evaluate_scaled_to_all_subjects_s": t_brute * N / a.subjects,
                      "speedup": t_brute * N / a.subjects / total,
                      "sampled_rows_with_mean_rank_within_top_n": int((ranks.mean(1) <= a.top_n).sum())}), flush=True)


if __name__ == "__main__":
    main()
