"""CPU test of the host-side staging of amdkge_session_group_rank for row-sharded groups (ampligraph_amd/csrc/kge_group_staging.h, used
by kge_session_group.hip rows_rank): the product's own C++ functions, compiled with g++ into a small harness (tests/csrc/staging_check.cpp)
that runs one thread per replica as the library does on distinct devices.  Checked against a numpy restatement: every distinct s / o
entity of a chunk gets exactly one scratch slot, exactly one replica (its owner under the reference's bucket rule,
/root/reference/ampligraph/datasets/graph_partitioner.py:339-344: contiguous ranges of ceil(N / W) ids) is asked to gather it, and the
re-indexed queries decode back to the original ids on every replica.  The two host-only pieces every session entry shares live in the same
header and are checked here too: the entities-subset tables (stage_subset) and the triple validation (first_bad_triple)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("staging") / "staging_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "staging_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("W,N,nq,seed", [(1, 50, 40, 0), (2, 2601, 300, 1), (3, 100, 7, 2), (4, 1000, 500, 3), (8, 97, 200, 4), (4, 5, 64, 5)])
def test_staging_of_a_row_sharded_rank_chunk(harness, W, N, nq, seed):
    rng = np.random.default_rng(seed)
    rows_per = -(-N // W)
    T = np.stack([rng.integers(0, N, nq), rng.integers(0, 7, nq), rng.integers(0, N, nq)], 1).astype(np.int32)
    T[: min(5, nq), 2] = T[: min(5, nq), 0]       # s == o queries
    T[-1, 0] = N - 1                               # the last row of the (ragged) last shard
    text = f"{W} {rows_per} {N} {nq}\n" + " ".join(str(int(v)) for v in T.reshape(-1)) + "\n"
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    first = np.array(out[0].split(), dtype=np.int64)
    nu, U = int(first[0]), first[1:]
    want_U = np.unique(np.concatenate([T[:, 0], T[:, 2]]))
    assert nu == len(want_U) and np.array_equal(U, want_U)
    owners = np.zeros(nu, dtype=np.int64)
    for d in range(W):
        row = np.array(out[1 + d].split(), dtype=np.int64)
        lo, n_local = int(row[0]), int(row[1])
        assert lo == d * rows_per and n_local == max(0, min(N, lo + rows_per) - lo)
        x, idx = row[2:2 + 3 * nq].reshape(nq, 3), row[2 + 3 * nq:]
        assert len(idx) == nu
        # the queries in the replica's local index space: scratch slot -> entity id gives the original triples back
        assert np.array_equal(U[x[:, 0] - n_local], T[:, 0]) and np.array_equal(U[x[:, 2] - n_local], T[:, 2]) and np.array_equal(x[:, 1], T[:, 1])
        assert x[:, [0, 2]].min() >= n_local and x[:, [0, 2]].max() < n_local + nu
        owned = (U >= lo) & (U < lo + n_local)
        assert np.array_equal(idx >= 0, owned) and np.array_equal(idx[owned], U[owned] - lo)
        owners += owned
    assert np.array_equal(owners, np.ones(nu, dtype=np.int64))          # one contributor per row: the bit-wise sum over replicas IS the row
    assert out[1 + W].split() == ["0", "4", "7", "7"]                    # stage_csr_slice


def _run(harness, mode, text):
    return subprocess.run([harness, mode], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")


@pytest.mark.parametrize("W", [1, 3, 4])
@pytest.mark.parametrize("N", [5, 97, 1000])
def test_entities_subset_tables_per_shard(harness, W, N):
    """stage_subset against a numpy restatement (ScoringBasedEmbeddingModel.py:1639-1643): per shard the owned candidates in the
    caller's order with duplicates kept, position = index of the LAST occurrence, -1 elsewhere, scratch rows all -1."""
    rng = np.random.default_rng(100 * W + N)
    rows_per, S = -(-N // W), 6
    subsets = {
        "duplicates": np.concatenate([rng.integers(0, N, 40), rng.integers(0, N, 40)[:15], [2, 2, 2]]),
        "both ends": np.array([N - 1, 0, 0, N - 1, N // 2, 0]),
        "later shards empty": np.array([1, 0, 1]),
        "one id": np.array([N - 1]),
    }
    for name, sub in subsets.items():
        out = _run(harness, "subset", f"{W} {rows_per} {N} {S} {len(sub)}\n" + " ".join(str(int(v)) for v in sub) + "\n")
        assert len(out) == W
        total = 0
        for d in range(W):
            row = np.array(out[d].split(), dtype=np.int64)
            lo = min(d * rows_per, N)
            n_local = min(N, lo + rows_per) - lo
            want_lst = np.array([v - lo for v in sub if lo <= v < lo + n_local], dtype=np.int64)
            want_pos = np.full(n_local + S, -1, dtype=np.int64)
            for j, v in enumerate(want_lst):
                want_pos[v] = j                                        # last wins
            ok, nl, npos = row[:3]
            lst, pos = row[3:3 + nl], row[3 + nl:]
            assert ok == 1 and npos == n_local + S == len(pos), (name, d)
            assert np.array_equal(lst, want_lst), (name, d)
            assert np.array_equal(pos, want_pos) and np.all(pos[n_local:] == -1), (name, d)
            total += nl
            if name == "later shards empty" and d > 0 and lo > 1:
                assert nl == 0 and np.all(pos == -1)
        assert total == len(sub)                                       # every candidate has exactly one owner
    for bad in (N, -1):                                                # an id outside [0, N): refused on every shard, wherever it stands
        sub = np.array([0, bad, 1])
        out = _run(harness, "subset", f"{W} {rows_per} {N} {S} {len(sub)}\n" + " ".join(str(int(v)) for v in sub) + "\n")
        assert [r.split()[0] for r in out] == ["0"] * W


def test_triple_validation_reports_the_first_bad_index(harness):
    """first_bad_triple: -1 for triples inside the tables (both ends included), else the index of the FIRST one outside -- whichever of
    s, p, o it is, too large or negative."""
    ne, nr, n = 50, 4, 12
    good = np.stack([np.arange(n) % ne, np.arange(n) % nr, (np.arange(n) * 7) % ne], 1)
    good[0] = (0, 0, ne - 1)
    good[-1] = (ne - 1, nr - 1, 0)

    def first(t, n_ents=ne, n_rels=nr):
        return int(_run(harness, "triples", f"{n_ents} {n_rels} {len(t)}\n" + " ".join(str(int(v)) for v in t.reshape(-1)) + "\n")[0])

    assert first(good) == -1 and first(good[:0]) == -1
    for i, col, val in ((0, 0, ne), (5, 2, ne), (5, 1, nr), (n - 1, 0, -1), (3, 1, -1), (7, 2, 1 << 30)):
        bad = good.copy()
        bad[i, col] = val
        assert first(bad) == i, (i, col, val)
        bad[min(i + 2, n - 1), 0] = ne + 3                             # a later bad triple does not move the report
        assert first(bad) == i
    assert first(good, n_ents=ne - 1) == 0 and first(good, n_rels=nr - 1) == 3   # the tables' own size decides
