// CPU harness of ampligraph_amd/csrc/kge_order.h (tests/test_order_host.py): the selection's order-preserving key and the sorted
// membership test, compiled by g++ from the product header.  Prints one line per failed check and returns their number (0: all hold).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <random>
#include <vector>

#include "../../ampligraph_amd/csrc/kge_order.h"

static uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
static float float_of(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }

static int check_keys() {
    int bad = 0;
    typedef std::numeric_limits<float> L;
    std::vector<uint32_t> pats = {bits_of(0.f), bits_of(-0.f), bits_of(L::denorm_min()), bits_of(-L::denorm_min()), 0x007FFFFFu, 0x807FFFFFu,
                                  bits_of(L::min()), bits_of(-L::min()), bits_of(L::max()), bits_of(L::lowest()), bits_of(INFINITY), bits_of(-INFINITY),
                                  bits_of(1.f), bits_of(-1.f)};
    std::mt19937 rng(12345);
    for (int i = 0; i < 4000; ++i) pats.push_back((uint32_t)rng());
    std::vector<float> vals;
    for (uint32_t p : pats) {
        const float v = float_of(p);
        if (v != v) {   // NaN: key 0, below every other key
            if (kge::sortable(v) != 0u) { printf("NaN pattern %08x has key %08x\n", p, kge::sortable(v)); ++bad; }
            continue;
        }
        if (kge::sortable(v) == 0u) { printf("%08x shares NaN's key\n", p); ++bad; }
        if (bits_of(kge::unsortable(kge::sortable(v))) != p) { printf("round trip of %08x gives %08x\n", p, bits_of(kge::unsortable(kge::sortable(v)))); ++bad; }
        vals.push_back(v);
    }
    // strictly monotone in the order of the bit patterns' values; -0 sits directly below +0 (the one pair that compares equal as floats)
    std::sort(vals.begin(), vals.end(), [](float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); });
    vals.erase(std::unique(vals.begin(), vals.end(), [](float a, float b) { return bits_of(a) == bits_of(b); }), vals.end());
    for (size_t i = 1; i < vals.size(); ++i)
        if (!(kge::sortable(vals[i - 1]) < kge::sortable(vals[i]))) { printf("keys of %a and %a are not ascending\n", vals[i - 1], vals[i]); ++bad; }
    return bad;
}

template <typename I>
static int check_contains(const std::vector<int32_t>& ids, I lo, I hi) {
    int bad = 0;
    if (lo >= hi) return kge::sorted_contains<I>(ids.data(), lo, hi, 0) ? (printf("empty range [%lld, %lld) holds 0\n", (long long)lo, (long long)hi), 1) : 0;
    for (int64_t id = (int64_t)ids[lo] - 1; id <= (int64_t)ids[hi - 1] + 1; ++id) {
        const bool want = std::binary_search(ids.begin() + lo, ids.begin() + hi, id);
        if (kge::sorted_contains<I>(ids.data(), lo, hi, id) != want) {
            printf("id %lld in [%lld, %lld) of %zu: expected %d\n", (long long)id, (long long)lo, (long long)hi, ids.size(), (int)want);
            ++bad;
        }
    }
    return bad;
}

static int check_ranges();

int main(int argc, char** argv) {   // order_check keys | order_check contains
    const bool keys = argc == 2 && !strcmp(argv[1], "keys");
    if (!keys && !(argc == 2 && !strcmp(argv[1], "contains"))) return 2;
    const int bad = keys ? check_keys() : check_ranges();
    printf("%d failed checks\n", bad);
    return bad ? 1 : 0;
}

static int check_ranges() {
    int bad = 0;
    std::mt19937 rng(777);
    for (int len : {0, 1, 2, 63, 64, 65, 1000}) {
        std::vector<int32_t> ids(len);
        for (int32_t& v : ids) v = (int32_t)(rng() % (2 * len + 3)) - 5;   // duplicates and gaps, some ids negative
        std::sort(ids.begin(), ids.end());
        for (int lo : {0, 1, len / 3, len}) {
            for (int hi : {len, len - 1, 2 * len / 3, lo}) {
                if (lo > len || hi < lo) continue;
                bad += check_contains<int>(ids, lo, hi);
                bad += check_contains<int64_t>(ids, (int64_t)lo, (int64_t)hi);
            }
        }
    }
    // ids at the ends of int32: the probe is 64-bit, min - 1 and max + 1 do not wrap
    const std::vector<int32_t> ends = {INT32_MIN, INT32_MIN, -7, 0, INT32_MAX};
    bad += check_contains<int>(ends, 0, 1) + check_contains<int64_t>(ends, 4, 5);
    for (int64_t id : {(int64_t)INT32_MIN - 1, (int64_t)INT32_MAX + 1, (int64_t)INT32_MIN, (int64_t)INT32_MAX})
        if (kge::sorted_contains<int64_t>(ends.data(), 0, 5, id) != (id == INT32_MIN || id == INT32_MAX)) { printf("end of range id %lld\n", (long long)id); ++bad; }
    return bad;
}
