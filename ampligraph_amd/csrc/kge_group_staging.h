// Host-side staging of amdkge_session_group_rank for a ROW-SHARDED group (kge_session_group.hip rows_rank): which entity rows a chunk of
// queries needs, where they sit behind every shard, and what each replica is asked to gather -- with the two host-only pieces every
// session entry shares (triple validation, the entities-subset tables).  Pure C++ (no HIP types): compiled into the
// library and, by tests/test_group_staging.py, into a CPU harness -- the logic every replica's host thread runs on a multi-GPU node.
//
// The reference's analogue is the partition loop of evaluate() (/root/reference/ampligraph/latent_features/models/ScoringBasedEmbeddingModel.py:1431-1452):
// there one process walks the entity partitions; here partition d lives on replica d, the rows of the queries' own s / o entities are
// gathered from their owners into scratch rows behind every shard, and the queries are re-indexed into that local index space.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace kge {

// the sorted distinct s / o ids of the chunk's queries tq[0 .. 3 nq): slot j of the scratch rows holds entity U[j] on EVERY replica
inline void stage_distinct_rows(const int32_t* tq, int64_t nq, std::vector<int32_t>& U) {
    U.resize((size_t)(2 * nq));
    for (int64_t i = 0; i < nq; ++i) { U[(size_t)(2 * i)] = tq[3 * i]; U[(size_t)(2 * i + 1)] = tq[3 * i + 2]; }
    std::sort(U.begin(), U.end());
    U.erase(std::unique(U.begin(), U.end()), U.end());
}

// One replica's staging (its own vectors: nothing here is shared with another replica's thread, U is read-only):
//   x   [3 nq]  the chunk's triples in the replica's LOCAL index space: s, o -> n_local + slot (the scratch rows behind the shard)
//   idx [|U|]   per slot the shard-local row to gather (the replica owns global rows [lo, lo + n_local)), -1 where another replica does
inline void stage_replica(const int32_t* tq, int64_t nq, const std::vector<int32_t>& U, int64_t lo, int64_t n_local,
                          std::vector<int32_t>& x, std::vector<int32_t>& idx) {
    auto slot_of = [&](int32_t id) { return (int64_t)(std::lower_bound(U.begin(), U.end(), id) - U.begin()); };
    x.resize((size_t)(3 * nq));
    for (int64_t i = 0; i < nq; ++i) {
        x[(size_t)(3 * i)] = (int32_t)(n_local + slot_of(tq[3 * i]));
        x[(size_t)(3 * i + 1)] = tq[3 * i + 1];
        x[(size_t)(3 * i + 2)] = (int32_t)(n_local + slot_of(tq[3 * i + 2]));
    }
    const int64_t nu = (int64_t)U.size();
    idx.resize((size_t)nu);
    for (int64_t j = 0; j < nu; ++j) {
        const int64_t v = (int64_t)U[(size_t)j] - lo;
        idx[(size_t)j] = (v >= 0 && v < n_local) ? (int32_t)v : -1;
    }
}

// the first of n host triples (s, p, o) with an id outside [0, n_ents) / [0, n_rels), or -1: an out-of-range id would become an
// out-of-bounds gather (or a scatter into the gradient tables) on the device, so every entry checks before anything is uploaded
inline int64_t first_bad_triple(const int32_t* t, int64_t n, int64_t n_ents, int64_t n_rels) {
    for (int64_t i = 0; i < n; ++i)
        if (t[3 * i] < 0 || t[3 * i] >= n_ents || t[3 * i + 2] < 0 || t[3 * i + 2] >= n_ents || t[3 * i + 1] < 0 || t[3 * i + 1] >= n_rels) return i;
    return -1;
}

// entities_subset for the candidates that live in rows [lo, lo + n_local) of the entity table (a whole table: lo = 0, n_local = N):
//   lst           the owned candidates as local rows (id - lo), in the caller's order, duplicates counted as given
//   pos [total_rows]  local row -> position in lst of the filter pass (last wins, ScoringBasedEmbeddingModel.py:1639-1643); -1 elsewhere,
//                     the scratch rows [n_local, total_rows) behind a shard included
// false when an id lies outside [0, N) (nothing is usable then)
inline bool stage_subset(const int32_t* subset, int64_t n_subset, int64_t N, int64_t lo, int64_t n_local, int64_t total_rows,
                         std::vector<int32_t>& lst, std::vector<int32_t>& pos) {
    lst.clear();
    pos.assign((size_t)total_rows, -1);
    for (int64_t i = 0; i < n_subset; ++i) {
        const int64_t v = (int64_t)subset[i] - lo;
        if (subset[i] < 0 || subset[i] >= N) return false;
        if (v < 0 || v >= n_local) continue;
        pos[(size_t)v] = (int32_t)lst.size();
        lst.push_back((int32_t)v);
    }
    return true;
}

// the chunk's slice [q0, q0 + nq] of a CSR offset array, zero-based
inline void stage_csr_slice(const int64_t* off, int64_t q0, int64_t nq, std::vector<int64_t>& lo) {
    lo.resize((size_t)(nq + 1));
    for (int64_t i = 0; i <= nq; ++i) lo[(size_t)i] = off[q0 + i] - off[q0];
}

}  // namespace kge
