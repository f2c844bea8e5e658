// evaluate(use_filter=...): the true-positive filter index, built ON THE DEVICE.
//
// Replaces the reference's per-batch pandas group-by + Python `sum(lists, [])`
// (/root/reference/ampligraph/datasets/graph_data_loader.py:287-350,382-439) and this repo's earlier host-side numpy
// restatement of it (datasets/filters.py, kept as the checker): for a test triple (s, p, o) the subject-side filter is the SET
// {s' : (s', p, o) in any filter dataset}, the object-side filter the SET {o' : (s, p, o') in any filter dataset}.
// As a CSR over sorted group keys:
//     subject side: group key (p * N + o), values s      object side: group key (s * R + p), values o
//   1. one 64-bit key per filter triple, key = group * N + value              (filter_keys_kernel)
//   2. device radix sort of the keys (rocPRIM, only the bits R * N^2 needs)
//   3. flags "new key" / "new group" per sorted position, one exclusive scan of the packed pair of counters (rocPRIM)
//   4. scatter: ids[unique position] = key % N; keys[group] = key / N, start[group] = unique position   (filter_emit_kernel)
// HBM-bound integer work: 310 k filter triples at C2 are 2.5 MB of keys -- microseconds; the point is that evaluate() no longer
// spends 15 ms in host sorts.
// The per-triple lookup into this index (amdkge_filter_ranges, amdkge_pair_filter_ranges) is one lower-bound kernel below; build and
// lookup take a triple's group key from the same function (filter_group_key).
#include <string.h>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "kge_host.h"

namespace kge {

// third key form (relation prediction, amdkge_pair_filter_build): group key (s * N + o), values p -- the divisor that separates
// group and value is then R instead of N
constexpr int FILTER_KEY_PAIR = 4;
// fourth and fifth key form (relation sets, include/amdkge_types.h): the group is the relation alone, the values are the subjects
// (a relation's DOMAIN) or the objects (its RANGE) seen with it
constexpr int FILTER_KEY_DOMAIN = 5;
constexpr int FILTER_KEY_RANGE = 6;

// THE definition of the five key forms: the group a triple belongs to.  The build sorts by group * divisor + value, the lookup
// searches the sorted groups for the query's.
//   AMDKGE_SIDE_S: group (p, o), value s      AMDKGE_SIDE_O: group (s, p), value o      FILTER_KEY_PAIR: group (s, o), value p
//   FILTER_KEY_DOMAIN: group p, value s       FILTER_KEY_RANGE: group p, value o
__host__ __device__ inline bool filter_key_is_relation(int form) { return form == FILTER_KEY_DOMAIN || form == FILTER_KEY_RANGE; }
__host__ __device__ inline uint64_t filter_group_key(int form, uint64_t s, uint64_t p, uint64_t o, uint64_t N, uint64_t R) {
    return filter_key_is_relation(form) ? p : form == FILTER_KEY_PAIR ? s * N + o : form == AMDKGE_SIDE_S ? p * N + o : s * R + p;
}
__host__ __device__ inline uint64_t filter_key_divisor(int form, uint64_t N, uint64_t R) { return form == FILTER_KEY_PAIR ? R : N; }

__global__ void filter_keys_kernel(const int32_t* __restrict__ tri, int64_t m, int form, uint64_t N, uint64_t R, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t s = (uint64_t)tri[3 * i], p = (uint64_t)tri[3 * i + 1], o = (uint64_t)tri[3 * i + 2];
    const uint64_t value = form == FILTER_KEY_PAIR ? p : (form == AMDKGE_SIDE_S || form == FILTER_KEY_DOMAIN) ? s : o;
    keys[i] = filter_group_key(form, s, p, o, N, R) * filter_key_divisor(form, N, R) + value;
}

// the lookup: one thread per query triple, lower_bound of its group key in the sorted group keys.  A group that is absent, or holds
// fewer than min_size ids, gives the fallback range (fb_lo, fb_hi): (0, 0) with min_size 0 for the filter lookups, the caller's
// for the relation sets -- THE place of the min_size rule.
__global__ void filter_ranges_kernel(const int64_t* keys, const int64_t* start, int64_t n_keys, const int32_t* triples, int64_t n, int form,
                                     int64_t n_ents, int64_t n_rels, int64_t min_size, int64_t fb_lo, int64_t fb_hi, int64_t* lo_out,
                                     int64_t* hi_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t q = (int64_t)filter_group_key(form, (uint64_t)triples[3 * i], (uint64_t)triples[3 * i + 1], (uint64_t)triples[3 * i + 2],
                                                (uint64_t)n_ents, (uint64_t)n_rels);
    int64_t a = 0, b = n_keys;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (keys[m] < q) a = m + 1; else b = m;
    }
    int64_t lo = fb_lo, hi = fb_hi;
    if (a < n_keys && keys[a] == q) {
        const int64_t g_lo = start[a], g_hi = start[a + 1];
        if (g_hi - g_lo >= min_size) { lo = g_lo; hi = g_hi; }
    }
    lo_out[i] = lo;
    hi_out[i] = hi;
}

// low 32 bits: 1 where a NEW KEY starts (duplicates of a triple across the filter datasets collapse), high 32 bits: 1 where a
// new GROUP starts
__global__ void filter_flags_kernel(const uint64_t* __restrict__ k, int64_t m, uint64_t N, uint64_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const bool nk = i == 0 || k[i] != k[i - 1];
    const bool ng = i == 0 || k[i] / N != k[i - 1] / N;
    flags[i] = (nk ? 1ull : 0ull) | (ng ? (1ull << 32) : 0ull);
}

__global__ void filter_emit_kernel(const uint64_t* __restrict__ k, const uint64_t* __restrict__ flags, const uint64_t* __restrict__ pos,
                                   int64_t m, uint64_t N, int64_t* __restrict__ keys_out, int64_t* __restrict__ start, int32_t* __restrict__ ids,
                                   int64_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t f = flags[i], at = pos[i];
    const int64_t u = (int64_t)(at & 0xFFFFFFFFull), g = (int64_t)(at >> 32);
    if (f & 1ull) ids[u] = (int32_t)(k[i] % N);
    if (f >> 32) { keys_out[g] = (int64_t)(k[i] / N); start[g] = u; }
    if (i == m - 1) {
        const int64_t n_unique = u + (int64_t)(f & 1ull), n_groups = g + (int64_t)(f >> 32);
        start[n_groups] = n_unique;
        counts[0] = n_groups;
        counts[1] = n_unique;
    }
}

struct FilterPlan {
    int64_t off_a, off_b, off_tmp, off_pos, total;   // the walk (the library aligns d_work up itself)
    size_t tmp_bytes;
    int key_bits;
};

static int key_bits_of(int64_t n_ents, int64_t n_rels) {
    // keys < R * N^2 (subject side: (p N + o) N + s; object side: (s R + p) N + o; pairs: (s N + o) R + p)
    long double top = (long double)n_rels * (long double)n_ents * (long double)n_ents;
    int b = 1;
    while (b < 64 && ldexpl(1.0L, b) < top) ++b;
    return b;
}

static int make_filter_plan(int64_t m, int64_t n_ents, int64_t n_rels, FilterPlan& p) {
    p.key_bits = key_bits_of(n_ents, n_rels);
    size_t t_sort = 0, t_scan = 0;
    uint64_t* nul = nullptr;
    if (rocprim::radix_sort_keys(nullptr, t_sort, nul, nul, (size_t)m, 0u, (unsigned)p.key_bits, (hipStream_t)0) != hipSuccess) return -1;
    if (rocprim::exclusive_scan(nullptr, t_scan, nul, nul, (uint64_t)0, (size_t)m, rocprim::plus<uint64_t>(), (hipStream_t)0) != hipSuccess) return -1;
    p.tmp_bytes = t_sort > t_scan ? t_sort : t_scan;
    Layout l;
    p.off_a = l.take(m, 8);                     // unsorted keys, then the flags
    p.off_b = l.take(m, 8);                     // sorted keys
    p.off_tmp = l.take((int64_t)p.tmp_bytes);   // rocPRIM scratch
    p.off_pos = l.take(m, 8);                   // scanned positions
    p.total = l.any_base(l.next());
    return 0;
}

}  // namespace kge

using namespace kge;

extern "C" int64_t amdkge_filter_build_workspace_bytes(int64_t m, int64_t n_ents, int64_t n_rels) {
    if (m < 0 || n_ents <= 0 || n_rels <= 0) return -1;
    if (m == 0) return 256;
    FilterPlan p;
    if (make_filter_plan(m, n_ents, n_rels, p)) return -1;
    return p.total;
}

static int filter_error(int code, const char* who, const char* what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return set_error(code, msg);
}

// the build behind the three entry points; form: AMDKGE_SIDE_S / AMDKGE_SIDE_O / FILTER_KEY_PAIR / FILTER_KEY_DOMAIN / FILTER_KEY_RANGE,
// who: the entry point, for the messages
static int filter_build_run(const char* who, const int32_t* d_triples, int64_t m, int form, int64_t n_ents, int64_t n_rels, int64_t* d_keys,
                            int64_t* d_start, int32_t* d_ids, int64_t* d_counts, void* d_work, hipStream_t st) {
    if (m < 0 || n_ents <= 0 || n_rels <= 0 || m > 0xFFFFFFFFll) return filter_error(AMDKGE_EINVAL, who, "bad sizes (at most 2^32 - 1 filter triples)");
    if ((long double)n_rels * (long double)n_ents * (long double)n_ents >= 9.2e18L)
        return filter_error(AMDKGE_EUNSUPPORTED, who, "n_rels * n_ents^2 does not fit the packed 64-bit sort keys");
    if (!d_start || !d_counts) return filter_error(AMDKGE_EINVAL, who, "NULL pointer");
    if (m == 0) {
        if (hipError_t e = hipMemsetAsync(d_start, 0, 8, st)) return set_error_hip(e, "hipMemsetAsync(filter start)");
        if (hipError_t e = hipMemsetAsync(d_counts, 0, 16, st)) return set_error_hip(e, "hipMemsetAsync(filter counts)");
        return AMDKGE_OK;
    }
    if (!d_triples || !d_keys || !d_ids || !d_work) return set_error(AMDKGE_EINVAL, "filter_build: NULL pointer");
    FilterPlan p;
    if (make_filter_plan(m, n_ents, n_rels, p)) return set_error(AMDKGE_EHIP, "filter_build: rocPRIM size query failed");
    const uint64_t div = filter_key_divisor(form, (uint64_t)n_ents, (uint64_t)n_rels);   // key = group * div + value
    char* w = aligned_base(d_work);
    uint64_t* a = (uint64_t*)(w + p.off_a);
    uint64_t* b = (uint64_t*)(w + p.off_b);
    void* tmp = w + p.off_tmp;
    uint64_t* pos = (uint64_t*)(w + p.off_pos);
    const unsigned grid = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(filter_keys_kernel, dim3(grid), dim3(256), 0, st, d_triples, m, form, (uint64_t)n_ents, (uint64_t)n_rels, a);
    if (int rc = check_launch("filter_keys")) return rc;
    size_t tb = p.tmp_bytes;
    if (hipError_t e = rocprim::radix_sort_keys(tmp, tb, a, b, (size_t)m, 0u, (unsigned)p.key_bits, st)) return set_error_hip(e, "rocprim::radix_sort_keys");
    hipLaunchKernelGGL(filter_flags_kernel, dim3(grid), dim3(256), 0, st, b, m, div, a);
    if (int rc = check_launch("filter_flags")) return rc;
    tb = p.tmp_bytes;
    if (hipError_t e = rocprim::exclusive_scan(tmp, tb, a, pos, (uint64_t)0, (size_t)m, rocprim::plus<uint64_t>(), st)) return set_error_hip(e, "rocprim::exclusive_scan");
    hipLaunchKernelGGL(filter_emit_kernel, dim3(grid), dim3(256), 0, st, b, a, pos, m, div, d_keys, d_start, d_ids, d_counts);
    return check_launch("filter_emit");
}

// the lookup behind the three entry points (the pair form's group key has no n_rels in it: its entry point passes 1; the relation
// forms' has neither size in it).  min_size, fb_lo, fb_hi: filter_ranges_kernel's; the filter lookups pass (0, 0, 0).
static int filter_ranges_run(const char* who, const int64_t* d_keys, const int64_t* d_start, int64_t n_keys, const int32_t* d_triples, int64_t n,
                             int form, int64_t n_ents, int64_t n_rels, int64_t min_size, int64_t fb_lo, int64_t fb_hi, int64_t* d_lo,
                             int64_t* d_hi, hipStream_t st) {
    if (n < 0 || n_keys < 0 || n_ents <= 0 || n_rels <= 0 || min_size < 0 || fb_lo < 0 || fb_hi < fb_lo) return filter_error(AMDKGE_EINVAL, who, "bad sizes");
    if (n == 0) return AMDKGE_OK;
    if (!d_triples || !d_lo || !d_hi || (n_keys > 0 && (!d_keys || !d_start))) return filter_error(AMDKGE_EINVAL, who, "NULL pointer");
    hipLaunchKernelGGL(filter_ranges_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_keys, d_start, n_keys, d_triples, n, form, n_ents,
                       n_rels, min_size, fb_lo, fb_hi, d_lo, d_hi);
    return check_launch(who);
}

extern "C" int amdkge_filter_build(const int32_t* d_triples, int64_t m, int32_t side, int64_t n_ents, int64_t n_rels,
                                   int64_t* d_keys, int64_t* d_start, int32_t* d_ids, int64_t* d_counts, void* d_work, void* stream) {
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "filter_build: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    return filter_build_run("filter_build", d_triples, m, (int)side, n_ents, n_rels, d_keys, d_start, d_ids, d_counts, d_work, (hipStream_t)stream);
}

// Relation prediction's filter: the same CSR keyed by the PAIR, group key (s * n_ents + o) with the SET of relations seen between
// the two (workspace: amdkge_filter_build_workspace_bytes, the plan is the same)
extern "C" int amdkge_pair_filter_build(const int32_t* d_triples, int64_t m, int64_t n_ents, int64_t n_rels, int64_t* d_keys, int64_t* d_start,
                                        int32_t* d_ids, int64_t* d_counts, void* d_work, void* stream) {
    return filter_build_run("pair_filter_build", d_triples, m, FILTER_KEY_PAIR, n_ents, n_rels, d_keys, d_start, d_ids, d_counts, d_work, (hipStream_t)stream);
}

extern "C" int amdkge_filter_ranges(const int64_t* d_keys, const int64_t* d_start, int64_t n_keys, const int32_t* d_triples,
                                    int64_t n, int32_t side, int64_t n_ents, int64_t n_rels, int64_t* d_lo, int64_t* d_hi,
                                    void* stream) {
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "filter_ranges: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    return filter_ranges_run("filter_ranges", d_keys, d_start, n_keys, d_triples, n, (int)side, n_ents, n_rels, 0, 0, 0, d_lo, d_hi, (hipStream_t)stream);
}

extern "C" int amdkge_pair_filter_ranges(const int64_t* d_keys, const int64_t* d_start, int64_t n_keys, const int32_t* d_triples, int64_t n,
                                         int64_t n_ents, int64_t* d_lo, int64_t* d_hi, void* stream) {
    return filter_ranges_run("pair_filter_ranges", d_keys, d_start, n_keys, d_triples, n, FILTER_KEY_PAIR, n_ents, 1, 0, 0, 0, d_lo, d_hi, (hipStream_t)stream);
}

// Relation sets (include/amdkge_types.h): the same CSR keyed by the relation alone -- the distinct subjects (side S: the DOMAIN) or
// objects (side O: the RANGE) seen with each relation.  Workspace: amdkge_filter_build_workspace_bytes, the plan is the same.
extern "C" int amdkge_relation_sets_build(const int32_t* d_triples, int64_t m, int32_t side, int64_t n_ents, int64_t n_rels, int64_t* d_keys,
                                          int64_t* d_start, int32_t* d_ids, int64_t* d_counts, void* d_work, void* stream) {
    if (side != AMDKGE_SIDE_S && side != AMDKGE_SIDE_O) return set_error(AMDKGE_EINVAL, "relation_sets_build: side must be AMDKGE_SIDE_S or AMDKGE_SIDE_O");
    return filter_build_run("relation_sets_build", d_triples, m, side == AMDKGE_SIDE_S ? FILTER_KEY_DOMAIN : FILTER_KEY_RANGE, n_ents, n_rels, d_keys,
                            d_start, d_ids, d_counts, d_work, (hipStream_t)stream);
}

// (the domain and the range CSR have the same group key, the relation: the lookup needs no side)
extern "C" int amdkge_relation_sets_ranges(const int64_t* d_keys, const int64_t* d_start, int64_t n_keys, const int32_t* d_triples, int64_t n,
                                           int64_t min_size, int64_t fb_lo, int64_t fb_hi, int64_t* d_lo, int64_t* d_hi, void* stream) {
    return filter_ranges_run("relation_sets_ranges", d_keys, d_start, n_keys, d_triples, n, FILTER_KEY_DOMAIN, 1, 1, min_size, fb_lo, fb_hi, d_lo,
                             d_hi, (hipStream_t)stream);
}
