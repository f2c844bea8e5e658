#!/usr/bin/env python3
"""Alternating A/B runs of bench.py over several builds of libamdkge.so (AMDKGE_LIB), one process per run.

usage: ab_bench.py OUT.jsonl RUNS[:SERIES] name=LIB [name=LIB ...] -- CONFIG [CONFIG ...]
       a CONFIG is a quoted string of bench.py flags ("" = the headline, "--config C3", "--model TransE", ...)

For every CONFIG, RUNS rounds; a round runs every library once, in the order given (so drift hits all of them alike).  Appends
{"series" (if given: the measuring session, where one file collects several), "config", "lib", "run", "ms_per_step", "wall_s"} per run
to OUT.jsonl and prints median and median absolute deviation per
(config, library) at the end.  Every run has its own time limit; the first run that fails, faults or times out ends the script."""
import json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    cut = argv.index("--")
    out, libs, configs = argv[1], [a.split("=", 1) for a in argv[3:cut]], argv[cut + 1:]
    runs, _, series = argv[2].partition(":")
    runs, head = int(runs), ({"series": int(series)} if series else {})
    seen = {}
    for cfg in configs:
        for run in range(runs):
            for name, lib in libs:
                t0 = time.perf_counter()
                cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "280", "--warmup", "28"] + cfg.split()
                p = subprocess.run(cmd, env=dict(os.environ, AMDKGE_LIB=os.path.abspath(lib)), capture_output=True, text=True)
                line = next((l for l in reversed(p.stdout.splitlines()) if l.startswith("{")), None)
                if p.returncode != 0 or line is None:
                    print("FAILED", cfg, name, "rc", p.returncode, p.stderr[-2000:], flush=True)
                    return 1
                rec = {**head, "config": cfg or "C2", "lib": name, "run": run, "ms_per_step": json.loads(line)["ms_per_step"], "wall_s": round(time.perf_counter() - t0, 1)}
                with open(out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                seen.setdefault((rec["config"], name), []).append(rec["ms_per_step"])
        for name, _ in libs:
            v = seen[(cfg or "C2", name)]
            med = statistics.median(v)
            print("%-18s %-8s median %.5f ms  mad %.5f  n %d" % (cfg or "C2", name, med, statistics.median(abs(x - med) for x in v), len(v)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
