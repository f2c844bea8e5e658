// evaluate(): what the translation units of the 1-vs-all ranking share.
//   kge_rank.hip        the C ABI, validation, the choice of path and its run-length planning, prep and compose
//   kge_rank_tile.hip   VALU tile kernels (rank_count_kernel, rank_rot_kernel), the distance models' early exit, corruption scores
//   kge_rank_mfma.hip   fp32 MFMA count kernels of the contraction models
//   kge_rank_screen.hip int8 screening pass, exact recheck, merge
//   kge_rank_filter.hip filter pass
// Here: the modes and their ONE accumulation chain (rank_op / rot_exact_op: tile, filter, probe and recheck kernels must keep producing
// bitwise equal scores, so there is a single definition), the geometry, the kernels' argument blocks, the workspace layouts, the
// run-time configuration, and the host functions a unit calls in another.  Every kernel is defined in exactly one unit; a kernel that
// another unit needs is reached through the launcher declared at the end of this file, which also owns the kernel's attribute set-up.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "kge_host.h"

namespace kge {

enum { MODE_DOT = 0, MODE_L1 = 1, MODE_ROT_O = 2, MODE_ROT_S = 3, MODE_L1_SUB = 4 };   // L1: |q + e| (subject side), L1_SUB: |q - e| (object side)

template <int MODE> struct ModeTraits;
template <> struct ModeTraits<MODE_DOT>   { static constexpr int NQF = 1, NEF = 1; };
template <> struct ModeTraits<MODE_L1>    { static constexpr int NQF = 1, NEF = 1; };
template <> struct ModeTraits<MODE_L1_SUB> { static constexpr int NQF = 1, NEF = 1; };
template <> struct ModeTraits<MODE_ROT_O> { static constexpr int NQF = 2, NEF = 2; };
template <> struct ModeTraits<MODE_ROT_S> { static constexpr int NQF = 4, NEF = 2; };

// RotatE's per-unit modulus: the hardware v_sqrt_f32 (1 ulp).  One sqrt per (query, entity, unit) is what bounds RotatE's
// evaluation; its 1-ulp error is below the fp32 summation-order noise the ranks already tolerate (oracle.fragile_rank_mask),
// and the tile and the filter kernel share this function, so they still agree bit for bit.
__device__ __forceinline__ float rank_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// acc + |d| as ONE v_add_f32 with the abs source modifier.  Written as plain C the SLP vectoriser pairs the accumulations into
// v_pk_add_f32, which has no abs modifier, and pays a v_and_b32 per unit for it: 4 issue slots per 2 units (pk sub, 2 and, pk add)
// instead of 3 (pk sub, 2 add-abs).  Same IEEE operations, same order: bitwise identical scores.
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float add_abs(float acc, float d) {
    float r;
    asm("v_add_f32 %0, %1, |%2|" : "=v"(r) : "v"(acc), "v"(d));
    return r;
}

// One unit of the corruption score, accumulated in unit order.  Shared by the tile kernel and the
// filter kernel so that both produce bitwise identical scores (compiled with -ffp-contract=off).
template <int MODE>
__device__ __forceinline__ float rank_op(float acc, const float (&q)[ModeTraits<MODE>::NQF],
                                         const float (&e)[ModeTraits<MODE>::NEF], float sgn) {
    if constexpr (MODE == MODE_DOT) {
        return fmaf(q[0], e[0], acc);
    } else if constexpr (MODE == MODE_L1) {
        return add_abs(acc, q[0] + e[0]);  // subject side: e + (p - o)        (TransE.py:77-83)
    } else if constexpr (MODE == MODE_L1_SUB) {
        return add_abs(acc, q[0] - e[0]);  // object side: (s + p) - e         (TransE.py:107-113); the sign is a template
                                           // parameter, not a multiply: 2 VALU instructions per unit instead of 3
    } else if constexpr (MODE == MODE_ROT_O) {
        const float re = q[0] - e[0], im = q[1] - e[1];   // RotatE.py:209-214
        return acc + rank_sqrt(re * re + im * im);
    } else {
        // q = (cos, sin, o_re, o_im) ; RotatE.py:151-160
        const float re = e[0] * q[0] - e[1] * q[1] - q[2];
        const float im = e[0] * q[1] + e[1] * q[0] - q[3];
        return acc + rank_sqrt(re * re + im * im);
    }
}

// One unit of RotatE's exact-mode chain for ONE (query, entity) pair: the operations of rot_micro, scalar (sqrt_rn == the
// packed sequence inside its domain, libm's sqrtf outside: bitwise the tile kernel's value either way).
template <int MODE>
__device__ __forceinline__ float rot_exact_op(float acc, const float (&q)[ModeTraits<MODE>::NQF], const float (&e)[2]) {
    float re, im;
    if constexpr (MODE == MODE_ROT_O) { re = q[0] - e[0]; im = q[1] - e[1]; }
    else { re = e[0] * q[0] - e[1] * q[1] - q[2]; im = e[0] * q[1] + e[1] * q[0] - q[3]; }
    return acc + sqrt_rn(re * re + im * im);
}

struct RankGeom {
    int U;        // units accumulated per (query, entity)
    int eplane;   // float offset between entity planes (re/im halves), 0 if NEF == 1
    int qplane;   // float offset between query planes
    int QW;       // floats per query row in the workspace
    int K;        // floats per table row
    float sgn;    // MODE_L1: +1 subject side, -1 object side
};

__host__ __device__ inline int mode_of(int model, int side) {
    if (model == AMDKGE_TRANSE) return side == AMDKGE_SIDE_S ? MODE_L1 : MODE_L1_SUB;
    if (model == AMDKGE_ROTATE) return side == AMDKGE_SIDE_S ? MODE_ROT_S : MODE_ROT_O;
    return MODE_DOT;
}

// Run-time configuration of the ranking units: ONE object (defined in kge_rank.hip), written only by the amdkge_set_rank_* setters.
struct EarlyCfg {
    int on = 1;
    int check_l1 = 4, check_rot = 1;   // stages (of KT = 16 units) between two checks.  A check is ~15 % of a TransE stage (1.5 issue slots per
                                       // pair and unit) and ~2 % of a RotatE stage: measured at the C2 shape on planted tables
                                       // (profiles/r04d_distance_models_sweep.jsonl) TransE 1.25 ms with 4, 1.56 - 1.96 with 2 or 1;
                                       // RotatE 6.2 - 6.3 ms with 1, 6.6 - 6.8 with 2
    int cost = 16;                     // a re-checked pair's chain costs about this many tile-kernel pair chains (measured ~10: one lane
                                       // per pair against a 4 x 4 register tile; handing over 2 % of the pairs costs what it saves)
    int probe = 1;                     // 0: the early-exit kernel always does the work (tests)
};
struct RankConfig {
    int kernel = 0;        // amdkge_set_rank_kernel (tests): 0 = automatic, 1 forces the VALU tile kernel, 2 the first MFMA kernel, 3 the pipelined one unscreened
    // RotatE: 0 (default) = exact mode (correctly rounded modulus, rank_rot_kernel / sqrt_rn), 1 = the 1-ulp hardware v_sqrt_f32
    // in the generic tile kernel (amdkge_set_rank_rotate_fast).  The tile and the filter kernel of one mode share their chain.
    int rotate_fast = 0;
    EarlyCfg early;        // amdkge_set_rank_early: the distance models' early exit (kge_rank_early.h)
};
extern RankConfig g_rank_cfg;

// (host only: the kernels get the geometry by value, so the configuration needs no device-side copy)
inline RankGeom geom_of(const amdkge_model* m, int side) {
    RankGeom g{};
    // stored layout (include/amdkge.h): the zero padding units add exact zeros to every accumulation chain (fmaf(0, 0, acc),
    // acc + |0|, acc + sqrt(0)), so the chains of a padded and of a dense table produce the same bits
    const int ks = stored_k(m);
    g.K = row_floats(m);
    const int mode = mode_of(m->scoring_type, side);
    if (mode == MODE_DOT || mode == MODE_L1 || mode == MODE_L1_SUB) { g.U = g.K; g.eplane = 0; g.qplane = 0; g.QW = g.K; }
    else {
        // exact mode walks the LIVE units only: a padding unit's modulus is sqrt(0), outside the fast sequence's domain
        g.U = g_rank_cfg.rotate_fast ? ks : m->k; g.eplane = ks; g.qplane = ks; g.QW = (mode == MODE_ROT_S ? 4 : 2) * ks;
    }
    g.sgn = (side == AMDKGE_SIDE_S) ? 1.f : -1.f;
    return g;
}

__device__ __forceinline__ int quantise(float score) {
    return (int)(score * 1000.0f);   // AbstractScoringLayer.py:201 tf.cast(score * 1e3, int32): truncation
}

// ------------------------------------------------------------------------------------------------
// tile geometry: VALU tile kernels (QT x ET pairs per workgroup, KT units per LDS stage), fp32 MFMA kernels (MQ x ME)
// ------------------------------------------------------------------------------------------------
constexpr int QT = 64, ET = 64, KT = 16, LDP = 68;   // LDP: padded LDS row (floats), keeps float4 reads aligned
constexpr int MQ = 128, ME = 128;

// ---- the guard protocol: a kernel launched as the fall-back of the screening / early-exit pass looks at device-side words ----
// The PROBE (rank_early_probe_kernel, kge_rank_early.h) samples 4 096 (query, candidate) pairs and counts those already decided at half
// their units; probe[0] = decided, probe[1] = sampled.  On tables whose positives do not stand out (an untrained model: nothing
// is decided before the last units) the early-exit kernel would only pay for its checks and its lower occupancy (measured: TransE
// k = 200, 12 % slower than the plain kernel), so the device decides which of the two kernels of the call does the work -- both
// are launched, one returns at once, no host round trip.
__device__ __forceinline__ bool early_probe_says_yes(const int* probe) { return probe[0] * 2 >= probe[1] && probe[1] > 0; }
enum { GUARD_NONE = 0, GUARD_FLAG = 1 /* run iff *guard != 0 */, GUARD_EARLY = 2 /* run iff the probe says yes */,
       GUARD_EARLY_FALLBACK = 3 /* run iff the probe says no, or *guard (the list overflowed) != 0 */ };
__device__ __forceinline__ bool guard_says_run(int mode, const int* guard, const int* probe) {
    if (mode == GUARD_FLAG) return *guard != 0;
    if (mode == GUARD_EARLY) return early_probe_says_yes(probe);
    if (mode == GUARD_EARLY_FALLBACK) return *guard != 0 || !early_probe_says_yes(probe);
    return true;
}

// the list the EARLY tile kernels hand their undecided pairs to (kge_rank_early.h: early_spill)
struct EarlyList { int* counter; int2* pairs; int64_t cap; };   // counter: [0] pairs appended, [1] overflow flag, [2] tiles ended early

struct CountArgs {
    const float* ent;
    const float* Q;
    const int* qpos;
    const int32_t* ent_ids;
    int32_t* counts;
    int64_t n;
    int64_t ent_lo, ent_hi;
    int ent_per_block;
    RankGeom g;
    float sgn_scale;
    int qtiles, splits;   // MFMA kernel: logical grid, decoded from a 1-D XCD-aware launch
    float* scores;        // STORE variant of the VALU tile kernel: [n][ld] un-quantised scores instead of counts
    int64_t ld;
    const int* guard;     // a kernel launched as the fall-back of the screening / early-exit pass: runs only if *guard != 0 (guard_mode
                          // refines this for the early-exit path: see guard_says_run above)
    int guard_mode;       // GUARD_* ; 0 with guard != NULL means GUARD_FLAG
    const int* e_probe;   // the early-exit probe's {decided, sampled}
    // EARLY variants of the distance models' tile kernels (kge_rank_early.h)
    EarlyList e_list;         // the list undecided pairs are handed to
    const uint8_t* e_qbad;    // [n] / [candidates]: rows whose pairs must not be decided early (non-finite or huge values)
    const uint8_t* e_ebad;
    int e_check, e_cost;      // stages between two checks; relative cost of a re-checked pair
};

// filter kernels (kge_rank_filter.hip): one wave per test triple, one lane per true-positive id
struct FilterArgs {
    const float* ent;
    const float* Q;
    const int* qpos;
    const int64_t* flt_lo;
    const int64_t* flt_hi;
    const int32_t* flt_ids;
    const int32_t* subset_pos;
    int32_t* sub;
    int64_t n;
    int64_t ent_lo, ent_hi;
    RankGeom g;
    float sgn_scale;
    const int* guard;    // non-NULL: run only if *guard != 0 (the pair list of the contraction models' filter pass overflowed)
};

// ------------------------------------------------------------------------------------------------
// d_work of a rank_counts / rank_filter / corruption_scores call (amdkge_rank_workspace_bytes)
// ------------------------------------------------------------------------------------------------
struct Workspace {
    float* Q;
    int* qpos;
    int* flt_counter;    // filter pass, contraction models: [0] pairs listed, [1] overflow flag
    int2* flt_pairs;     // (query, table row of a known positive)
    int64_t flt_cap;
};

inline int64_t query_row_floats(const amdkge_model* m) { return (m->scoring_type == AMDKGE_ROTATE) ? 4ll * stored_k(m) : row_floats(m); }
inline int64_t filter_pair_cap(int64_t n) {   // 64 known positives per query on average; the list counter is an int32
    const int64_t c = n * 64 > 65536 ? n * 64 : 65536;
    return c < (1ll << 30) ? c : (1ll << 30);
}

// the walk: query positions | query vectors | the filter pass's counter | its pair list.  The library aligns d_work up itself.
// (a braced list is evaluated in order: the members of a walk's struct stand in the order of its regions)
struct RankLayout { int64_t qpos, Q, flt_counter, flt_pairs, total; };
inline RankLayout rank_layout(const amdkge_model* m, int64_t n) {
    Layout l;
    return RankLayout{l.take(n, sizeof(int)), l.take(n, query_row_floats(m) * (int64_t)sizeof(float)), l.take(256), l.take(filter_pair_cap(n), sizeof(int2)), l.any_base(l.end())};
}
inline Workspace carve(void* d_work, const amdkge_model* m, int64_t n) {
    const RankLayout r = rank_layout(m, n);
    char* w = aligned_base(d_work);
    return Workspace{(float*)(w + r.Q), (int*)(w + r.qpos), (int*)(w + r.flt_counter), (int2*)(w + r.flt_pairs), filter_pair_cap(n)};
}

// ------------------------------------------------------------------------------------------------
// d_screen of a screened call (amdkge_rank_screen_workspace_bytes): the screening pass's layout (kge_rank_screen.h), whose head --
// counters, counts, pair list -- the early exit reuses (kge_rank_early.h)
// ------------------------------------------------------------------------------------------------
constexpr int SCR_Q = 128, SCR_K = 32;   // queries per workgroup (4 waves x 32), units per stage
constexpr int SCR_ROW_SLAB = 96;                       // bytes of one row per K slab: 3 limbs x 32 units
// Limb storage is FRAGMENT-MAJOR: [block of 32 rows][slab][limb][half][row % 32][16 bytes] -- the 64 lanes of a matrix operand
// fragment (lane = half * 32 + row % 32, 16 units each) read 1 KB of CONSECUTIVE memory, from global memory as from LDS.
constexpr int SCR_BLK_SLAB = 32 * SCR_ROW_SLAB;        // bytes of one 32-row block per K slab (3 072)

struct ScreenBufs {
    int* counter;        // [0] undecided pairs appended, [1] overflow flag, [2] candidate rows > 4 bits below their tile's scale (rank_limbs_tile_kernel)
    int32_t* counts;     // [n][2] this call's (greater, equal) counts (merged into the caller's unless the call fell back)
    int8_t* qlimbs;      // [ceil(n / 32)][S][3][2][32][16]
    float4* qm;          // [n] {A = 2^-a, u (1 + 2 U u) |W q|_2, |q|_1 / 2, 0}, all rounded up
    float2* qt;          // [n] {T_ge, T_gt}
    int8_t* elimbs;      // [ceil(m / 32)][S][3][2][32][16]
    float4* em;          // [m] {B, |W e|_2, |e|_1 / 2, 0}
    float4* tm;          // [ceil(m / 64)] per tile of 64 candidates {B_t, max |W e|_2, max |e|_1 / 2, 1 / B_t}: rank_limbs_tile_kernel (kernel r)
    int2* pairs;         // [cap] (query, candidate position)
    int64_t cap;
    int S;               // K slabs per row
};

// the walk for n queries against m candidates of U units: the regions of ScreenBufs.  `pairs` is also the size of the fixed part
// (everything but the pair list), `qlimbs` that of the counters and counts a call zeroes; cap: what a buffer of `usable` bytes behind
// its aligned base leaves the list.  The library aligns d_screen up itself.
struct ScreenLayout { int64_t counter, counts, qlimbs, qm, qt, elimbs, em, tm, pairs, cap, S; };
static inline ScreenLayout screen_layout(int64_t n, int64_t m, int U, int64_t usable = 0) {
    Layout l;
    const int64_t S = (U + SCR_K - 1) / SCR_K, nb = (n + 31) / 32 + 4, mb = (m + 31) / 32 + 4;   // (+ a tile of slack: loaders read whole 128-row tiles)
    return ScreenLayout{l.take(256), l.take(n, 8), l.take(nb, S * SCR_BLK_SLAB), l.take(n, 16), l.take(n, 8), l.take(mb, S * SCR_BLK_SLAB), l.take(m, 16),
                        l.take((m + 63) / 64 + 4, 16), l.next(), l.rest(usable, 8), S};
}
static inline ScreenBufs carve_screen(void* d_screen, size_t bytes, int64_t n, int64_t m, int U) {
    const ScreenLayout s = screen_layout(n, m, U, (int64_t)bytes - base_pad(d_screen));
    char* w = aligned_base(d_screen);
    return ScreenBufs{(int*)(w + s.counter), (int32_t*)(w + s.counts), (int8_t*)(w + s.qlimbs), (float4*)(w + s.qm), (float2*)(w + s.qt),
                      (int8_t*)(w + s.elimbs), (float4*)(w + s.em), (float4*)(w + s.tm), (int2*)(w + s.pairs), s.cap, (int)s.S};
}

// the early exit's walk (kge_rank_early.h: carve_early): counters | this call's counts | row flags (queries, candidates) | pair list;
// pairs and cap as above, `qbad` the size of the counters and counts
struct EarlyLayout { int64_t counter, counts, qbad, ebad, pairs, cap; };
static inline EarlyLayout early_layout(int64_t n, int64_t m, int64_t usable = 0) {
    Layout l;
    return EarlyLayout{l.take(256), l.take(n, 8), l.take(n), l.take(m), l.next(), l.rest(usable, 8)};
}

// exact recheck of listed pairs (rank_recheck_kernel, kge_rank_screen.h): the screening pass's undecided pairs, the filter pass's (query, known positive) pairs
struct RecheckArgs {
    const float* ent;
    const float* Q;
    const int* qpos;
    const int32_t* ent_ids;
    int64_t ent_lo;
    int U, K, QW;
    float sgn_scale;
    ScreenBufs b;
};


// ------------------------------------------------------------------------------------------------
// host functions called across units (each defined next to the kernels it launches)
// ------------------------------------------------------------------------------------------------
// kge_rank.hip: positive scores and query vectors into the workspace
int run_prep(const amdkge_model* m, const float* d_ent, const float* d_rel, const int32_t* d_triples, int64_t n,
             int side, const RankGeom& g, const Workspace& w, hipStream_t st);
// kge_rank_tile.hip: the plain count kernel of the mode (rank_rot_kernel in RotatE's exact mode), the early-exit probe and sequence,
// the STORE variants
int launch_count_tile(int mode, bool v4, bool rot_exact, const CountArgs& a, dim3 grid, hipStream_t st);
int early_probe(int mode, const float* d_ent, const int32_t* d_ent_ids, int64_t ent_lo, int64_t mcand, int64_t n, const RankGeom& g,
                const Workspace& w, float sgn_scale, void* d_screen, size_t screen_bytes, bool* yes, bool* measured, hipStream_t st);
int run_early(int mode, const amdkge_model* m, const float* d_ent, const int32_t* d_ent_ids, int64_t ent_lo, int64_t mcand, int64_t n,
              const RankGeom& g, const Workspace& w, CountArgs a, dim3 grid, void* d_screen, size_t screen_bytes, const int** guard_out,
              bool probe_measured, hipStream_t st);
int launch_store(int mode, bool v4, CountArgs& a, int64_t n, int64_t m, hipStream_t st);
// kge_rank_mfma.hip: rank_count_mfma_pipe_kernel (v4 && pipe) or rank_count_mfma_kernel<v4> on a 1-D grid of nblk workgroups
int launch_count_mfma(bool v4, bool pipe, const CountArgs& a, unsigned nblk, hipStream_t st);
// kge_rank_screen.hip: the screening sequence of one call; rank_recheck_kernel<true> over the filter pass's pair list
int run_screen(const amdkge_model* m, const float* d_ent, const int32_t* d_ent_ids, int64_t ent_lo, int64_t mcand, int64_t n,
               const RankGeom& g, const Workspace& w, const ModelConst& mc, int32_t* d_counts, void* d_screen, size_t screen_bytes,
               hipStream_t st);
int launch_recheck_filter(const RecheckArgs& ra, unsigned nblk, hipStream_t st);

}  // namespace kge
