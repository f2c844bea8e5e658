"""Wall time of find_clusters with its default algorithm (DBSCAN) on the device path (amdkge_join_dbscan, kge_join.hip) beside the
path it replaces: download the embeddings and run sklearn.cluster.DBSCAN.fit_predict on the host (n_jobs at its default).  Same
tables, same eps / min_samples, whole calls.  Not part of bench.py.

Shapes: n = 14 505, d = 400 (the headline entity table, ComplEx k = 200) and n = 100 000, d = 64 (ComplEx
k = 32).  The entity table of a one-epoch model is overwritten with planted rows: blobs of `--blob` rows (sigma 0.05 around centres
3 N(0, 1) apart) made of groups of four near-copies (2e-3 around the group's first row).  Each shape runs with a sparse eps (the
three near-copies are a row's only neighbours) and a dense one (the whole blob: clusters of thousands); min_samples = 3.

Device path: warm-up, then the median of `--reps` calls, host clock around a synchronised call (the call ends with its own
download of the labels).  Host path: the download (median of `--reps`, synchronised) plus fit_predict in a child process of its
own (no GPU in it) under `--host-limit` seconds; a run that hits the limit is reported as "did not finish in T".  The two label
arrays are compared when the host run finishes.  One JSON line per shape and eps.

    python scripts/cluster_timing.py [--reps 5] [--shapes 14505x400,100000x64] [--host-limit 120] [--no-host]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def host_child(path, eps, min_samples):
    """fit_predict on the saved embeddings; prints seconds and writes the labels beside the input."""
    from sklearn.cluster import DBSCAN

    E = np.load(path)
    t = time.perf_counter()
    labels = DBSCAN(eps=eps, min_samples=min_samples).fit_predict(E)
    dt = time.perf_counter() - t
    np.save(path + ".labels.npy", labels)
    print(json.dumps({"fit_predict_s": dt}), flush=True)


def planted_rows(rng, n, d, blob):
    groups = (n + 3) // 4
    centres = 3.0 * rng.normal(size=((n + blob - 1) // blob, d))
    first = centres[(np.arange(groups) * 4) // blob] + 0.05 * rng.normal(size=(groups, d))
    X = np.repeat(first, 4, axis=0)[:n] + 2e-3 * rng.normal(size=(n, d))
    return X[rng.permutation(n)].astype(np.float32)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="14505x400,100000x64")
    ap.add_argument("--blob", type=int, default=2000)
    ap.add_argument("--host-limit", type=float, default=120.0)
    ap.add_argument("--no-host", action="store_true", help="device path only (for a kernel trace)")
    ap.add_argument("--host-child", nargs=3, metavar=("NPY", "EPS", "MIN_SAMPLES"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.host_child:
        return host_child(a.host_child[0], float(a.host_child[1]), int(a.host_child[2]))

    import torch
    from sklearn.cluster import DBSCAN

    from ampligraph_amd.discovery import _device_embeddings, find_clusters
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel

    rng = np.random.default_rng(0)
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        T = np.stack([np.arange(n), np.zeros(n, dtype=np.int64), rng.permutation(n)], 1)   # every entity occurs
        m = ScoringBasedEmbeddingModel(eta=1, k=d // 2, scoring_type="ComplEx", seed=0)
        m.compile(optimizer="adam", loss="nll")
        m.fit(T, batch_size=min(n, 30000), epochs=1, verbose=False)
        eng = m._engine
        assert eng.K == d and eng.n_ents == n
        eng.set_tables(planted_rows(rng, n, d, a.blob), eng.get_tables()[1])
        ents = m.data_indexer.get_indexes(np.arange(n), "e", "ind2raw")
        # near-copies lie 2e-3 sqrt(2 d) apart, rows of a blob 0.05 sqrt(2 d), blobs 3 sqrt(2 d)
        for name, eps in (("sparse", 0.01 * np.sqrt(2.0 * d)), ("dense", 0.075 * np.sqrt(2.0 * d))):
            eps = float(eps)

            def device():
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = find_clusters(ents, m, DBSCAN(eps=eps, min_samples=3))
                torch.cuda.synchronize()
                return time.perf_counter() - t, out

            def download():
                torch.cuda.synchronize()
                t = time.perf_counter()
                E = _device_embeddings(m, ents, "e").cpu().numpy()
                return time.perf_counter() - t, E

            device()
            t_dev = median([device()[0] for _ in range(a.reps)])
            labels = device()[1]
            line = {"n": n, "d": d, "eps": name, "eps_value": eps, "min_samples": 3, "reps": a.reps, "device_find_clusters_s": t_dev,
                    "clusters": int(labels.max()) + 1, "noise_rows": int((labels < 0).sum()),
                    "largest_cluster": int(np.bincount(labels[labels >= 0]).max()) if (labels >= 0).any() else 0}
            if not a.no_host:
                download()
                t_down = median([download()[0] for _ in range(a.reps)])
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "emb.npy")
                    np.save(path, download()[1])
                    line["host_download_s"] = t_down
                    try:
                        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-child", path, repr(eps), "3"], check=True,
                                             capture_output=True, text=True, timeout=a.host_limit)
                        t_fit = json.loads(out.stdout.strip().splitlines()[-1])["fit_predict_s"]
                        line.update({"host_fit_predict_s": t_fit, "host_total_s": t_down + t_fit, "speedup": (t_down + t_fit) / t_dev,
                                     "labels_equal": bool(np.array_equal(np.load(path + ".labels.npy"), labels))})
                    except subprocess.TimeoutExpired:
                        line["host_fit_predict_s"] = "did not finish in %g s" % a.host_limit
            print(json.dumps(line), flush=True)
        del m, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
