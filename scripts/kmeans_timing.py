"""Wall time of the device KMeans (discovery.KMeans: amdkge_kmeans_lloyd, kge_kmeans.hip) beside sklearn.cluster.KMeans with the same
parameters on the host.  Same table, whole fits; the two use different seedings (plain against greedy k-means++), so the inertias are
reported beside the times, not compared bit for bit.  Not part of bench.py.

Shapes:
  a  n = 14 505, d = 400: the headline entity table with the reference's documented KMeans(n_clusters=6, n_init=100, max_iter=500)
  b  n = 1 000 000, d = 64, k = 64, n_init = 4
Rows: blobs of sigma 0.5 around `blobs` centres 2 N(0, 1) apart (2 k blobs: the restarts do not all end in one optimum).

Device path: one warm-up fit, then the median of `--reps` fits, host clock around a synchronised call on a matrix that is already
on the device (what find_clusters hands the estimator); the iterations of the best run and the largest over the runs are reported.
Host path: sklearn in a child process of its own (no GPU in it) under `--host-limit` seconds; a run that hits the limit is reported
as "did not finish in T".  One JSON line per shape.

    python scripts/kmeans_timing.py [--reps 3] [--shapes a,b] [--host-limit 300] [--no-host]"""
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

SHAPES = {"a": dict(n=14505, d=400, k=6, n_init=100, max_iter=500), "b": dict(n=1_000_000, d=64, k=64, n_init=4, max_iter=300)}


def host_child(path, k, n_init, max_iter):
    from sklearn.cluster import KMeans

    E = np.load(path)
    t = time.perf_counter()
    km = KMeans(n_clusters=k, n_init=n_init, max_iter=max_iter, random_state=0).fit(E)
    print(json.dumps({"fit_s": time.perf_counter() - t, "inertia": float(km.inertia_), "n_iter": int(km.n_iter_)}), flush=True)


def rows(n, d, k, seed=0):
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.normal(size=(2 * k, d))
    return (centres[rng.integers(0, 2 * k, n)] + 0.5 * rng.normal(size=(n, d))).astype(np.float32)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--host-limit", type=float, default=300.0)
    ap.add_argument("--no-host", action="store_true", help="device path only (for a kernel trace)")
    ap.add_argument("--host-child", nargs=4, metavar=("NPY", "K", "N_INIT", "MAX_ITER"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.host_child:
        return host_child(a.host_child[0], *(int(v) for v in a.host_child[1:]))

    import torch

    from ampligraph_amd.discovery import KMeans
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine("DistMult", 4, 4, 2)
    for name in a.shapes.split(","):
        s = SHAPES[name]
        E = rows(s["n"], s["d"], s["k"])
        Ed = torch.as_tensor(E).cuda()
        seen = {}
        real = eng.kmeans

        def spy(*args, **kw):
            out = real(*args, **kw)
            seen["n_iter"] = out[3].cpu().numpy()
            return out

        eng.kmeans = spy

        def device():
            torch.cuda.synchronize()
            t = time.perf_counter()
            km = KMeans(n_clusters=s["k"], n_init=s["n_init"], max_iter=s["max_iter"], random_state=0).fit(Ed, engine=eng)
            torch.cuda.synchronize()
            return time.perf_counter() - t, km

        device()
        t_dev = median([device()[0] for _ in range(a.reps)])
        km = device()[1]
        eng.kmeans = real
        line = {"shape": name, **s, "reps": a.reps, "device_fit_s": t_dev, "device_inertia": km.inertia_, "device_n_iter_best": km.n_iter_,
                "device_n_iter_max": int(seen["n_iter"].max()), "device_iterations_total": int(seen["n_iter"].sum())}
        if not a.no_host:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "emb.npy")
                np.save(path, E)
                env = {k: v for k, v in os.environ.items() if k not in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES")}
                env["HIP_VISIBLE_DEVICES"] = ""   # the child gets no GPU
                try:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-child", path, str(s["k"]), str(s["n_init"]), str(s["max_iter"])],
                                         check=True, capture_output=True, text=True, timeout=a.host_limit, env=env)
                    h = json.loads(out.stdout.strip().splitlines()[-1])
                    line.update({"host_fit_s": h["fit_s"], "host_inertia": h["inertia"], "host_n_iter_best": h["n_iter"], "speedup": h["fit_s"] / t_dev})
                except subprocess.TimeoutExpired:
                    line["host_fit_s"] = "did not finish in %g s" % a.host_limit
        print(json.dumps(line), flush=True)
        del Ed
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
