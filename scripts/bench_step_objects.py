"""Python cost of trainer.StepLoop.step, without a GPU: the median microseconds of a step on an engine whose methods do nothing, for
three rows of tests/test_step_calls_host.py (its models, samplers and bind path).  --root DIR measures the package of another
checkout (the parent commit) with this checkout's table:  python scripts/bench_step_objects.py [--root DIR] [--steps 4000]
-> one JSON line; profiles/step_objects.json holds parent, new, parent."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--steps", type=int, default=4000)
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.root), os.path.join(HERE, "tests")]

import pytest   # noqa: E402
import torch    # noqa: E402

import test_step_calls_host as T   # noqa: E402


class NoOpEngine(T.RecordingEngine):
    def _record(self, method, *a, **kw):
        pass

    def sample_shared(self, triples, group_size, num_negs, seed, step, **kw):
        return self._drawn

    _drawn = (torch.zeros(2, 1, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))


T.RecordingEngine = NoOpEngine
out = {"root": os.path.abspath(args.root), "steps": args.steps, "median_us": {}}
for want in ("no sampler, atomic", "shared masked identity", "KvsAll query"):
    name, scoring, loss, negatives, path, _ = next(r for r in T.ROWS if r[0] == want)
    with pytest.MonkeyPatch.context() as mp:
        loop, eng, train = T._setup(scoring, loss if isinstance(loss, str) else loss(), negatives and negatives(), False, False, mp, path)
        batches, times = (train[0:6], train[6:12]), []
        for i in range(args.steps + 200):
            t0 = time.perf_counter_ns()
            loop.step(batches[i & 1], i)
            times.append(time.perf_counter_ns() - t0)
    out["median_us"][name] = round(statistics.median(times[200:]) / 1e3, 3)
print(json.dumps(out))
