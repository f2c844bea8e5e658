// CPU harness of ampligraph_amd/csrc/kge_group_staging.h (tests/test_group_staging.py): reads a problem from stdin, runs the product's
// staging functions for every replica of a row-sharded group IN ONE THREAD PER REPLICA (as rows_rank does on distinct devices) and
// prints what they staged.
//   (no argument)   in : W rows_per N nq  then nq triples (s p o)
//                   out: |U| U...  then per replica: lo n_local, x[3 nq], idx[|U|]
//   subset          in : W rows_per N S n_subset  then the subset ids (S scratch rows behind every shard)
//                   out: per replica: ok |lst| |pos|, lst..., pos...   (stage_subset)
//   triples         in : n_ents n_rels n  then n triples
//                   out: the index of the first triple outside the tables, or -1   (first_bad_triple)
#include <stdio.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../ampligraph_amd/csrc/kge_group_staging.h"

static bool read_ints(std::vector<int32_t>& v) {
    for (auto& e : v) { int x; if (scanf("%d", &x) != 1) return false; e = x; }
    return true;
}

static int subset_mode() {
    long long W, rows_per, N, S, ns;
    if (scanf("%lld %lld %lld %lld %lld", &W, &rows_per, &N, &S, &ns) != 5) return 2;
    std::vector<int32_t> sub((size_t)ns), lst, pos;
    if (!read_ints(sub)) return 2;
    for (long long d = 0; d < W; ++d) {
        const long long lo = d * rows_per < N ? d * rows_per : N, hi = (lo + rows_per < N) ? lo + rows_per : N;
        const bool ok = kge::stage_subset(sub.data(), ns, N, lo, hi - lo, hi - lo + S, lst, pos);
        printf("%d %zu %zu", ok ? 1 : 0, lst.size(), pos.size());
        for (int32_t v : lst) printf(" %d", v);
        for (int32_t v : pos) printf(" %d", v);
        printf("\n");
    }
    return 0;
}

static int triples_mode() {
    long long ne, nr, n;
    if (scanf("%lld %lld %lld", &ne, &nr, &n) != 3) return 2;
    std::vector<int32_t> t((size_t)(3 * n));
    if (!read_ints(t)) return 2;
    printf("%lld\n", (long long)kge::first_bad_triple(t.data(), n, ne, nr));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "subset")) return subset_mode();
    if (argc > 1 && !strcmp(argv[1], "triples")) return triples_mode();
    long long W, rows_per, N, nq;
    if (scanf("%lld %lld %lld %lld", &W, &rows_per, &N, &nq) != 4) return 2;
    std::vector<int32_t> t((size_t)(3 * nq));
    for (auto& v : t) { int x; if (scanf("%d", &x) != 1) return 2; v = x; }
    std::vector<int32_t> U;
    kge::stage_distinct_rows(t.data(), nq, U);
    std::vector<std::vector<int32_t>> xl((size_t)W), idxl((size_t)W);
    std::vector<std::thread> th;
    for (long long d = 0; d < W; ++d)
        th.emplace_back([&, d]() {
            const long long lo = d * rows_per, hi = (lo + rows_per < N) ? lo + rows_per : N;
            kge::stage_replica(t.data(), nq, U, lo, hi > lo ? hi - lo : 0, xl[(size_t)d], idxl[(size_t)d]);
        });
    for (auto& x : th) x.join();
    printf("%zu", U.size());
    for (int32_t v : U) printf(" %d", v);
    printf("\n");
    for (long long d = 0; d < W; ++d) {
        const long long lo = d * rows_per, hi = (lo + rows_per < N) ? lo + rows_per : N;
        printf("%lld %lld", lo, hi > lo ? hi - lo : 0);
        for (int32_t v : xl[(size_t)d]) printf(" %d", v);
        for (int32_t v : idxl[(size_t)d]) printf(" %d", v);
        printf("\n");
    }
    std::vector<int64_t> off = {5, 5, 9, 12, 12, 20}, lo;
    kge::stage_csr_slice(off.data(), 1, 3, lo);
    printf("%lld %lld %lld %lld\n", (long long)lo[0], (long long)lo[1], (long long)lo[2], (long long)lo[3]);
    return 0;
}
