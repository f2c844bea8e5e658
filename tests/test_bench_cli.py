"""bench.py's run control on the host: what a plain run does against --full, and what --dump-outputs writes (tables through a
host-side stand-in for the engine's unpack)."""
import sys

import numpy as np
import pytest
import torch

import bench


def parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_times_one_region_of_the_given_steps(monkeypatch):
    a = parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.full, a.reps, a.steps, a.warmup, a.also, a.dump_outputs) == (False, 1, 7, 2, "none", None)


def test_full_run_keeps_the_former_default_measurements(monkeypatch):
    a = parse(["--gpus", "1", "--full"], monkeypatch)
    assert (a.reps, a.also) == (5, "C1,C3,C4,C5")
    assert parse(["--full", "--config", "C3"], monkeypatch).also == "none"
    assert parse(["--full", "--reps", "2"], monkeypatch).reps == 2


@pytest.mark.parametrize("extra", [["--also", "C3"], ["--dropin"], ["--trained-eval"]])
def test_measurements_beside_the_headline_need_full(monkeypatch, extra):
    with pytest.raises(SystemExit):
        parse(extra, monkeypatch)
    parse(extra + ["--full"], monkeypatch)


class HostEngine:
    """the attributes dump_outputs reads; stored rows = dense rows (no padding)"""

    def __init__(self, n_ents, n_rels, K):
        g = torch.Generator().manual_seed(0)
        self.K, self.n_rels = K, n_rels
        self.ent = torch.rand(n_ents + 3, K, generator=g)   # 3 rows past the ones this rank holds (request slots)
        self.rel = torch.rand(n_rels, K, generator=g)

    def unpack(self, stored):
        return stored.clone()


def test_dump_budget_is_under_64_mb():
    assert sum(bench.DUMP_TABLE_BYTES.values()) + 1024 <= 64_000_000


def test_dump_writes_whole_small_tables(tmp_path):
    eng = HostEngine(50, 4, 8)
    bench.dump_outputs(str(tmp_path), eng, 50, 1.25)
    ent, rel = np.load(tmp_path / "entity_table.npy"), np.load(tmp_path / "relation_table.npy")
    assert ent.dtype == np.float32 and np.array_equal(ent, eng.ent[:50].numpy())
    assert rel.dtype == np.float32 and np.array_equal(rel, eng.rel.numpy())
    assert np.array_equal(np.load(tmp_path / "entity_table_rows.npy"), np.arange(50, dtype=np.float64))
    loss = np.load(tmp_path / "mean_batch_loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.25]
    assert all(np.load(f).dtype in (np.float32, np.float64) for f in tmp_path.iterdir())


def test_dump_samples_large_tables_the_same_rows_every_time(tmp_path, monkeypatch):
    monkeypatch.setitem(bench.DUMP_TABLE_BYTES, "entity", 40 * (4 * 8 + 8))   # room for 40 rows of K = 8
    eng = HostEngine(1000, 4, 8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), eng, 1000, 0.5)
    ids = np.load(tmp_path / "a" / "entity_table_rows.npy")
    assert ids.shape == (40,) and np.all(np.diff(ids) > 0) and ids.max() < 1000
    assert np.array_equal(ids, np.load(tmp_path / "b" / "entity_table_rows.npy"))
    ent = np.load(tmp_path / "a" / "entity_table.npy")
    assert np.array_equal(ent, eng.ent.numpy()[ids.astype(np.int64)])
    assert np.array_equal(ent, np.load(tmp_path / "b" / "entity_table.npy"))
