// CPU harness for the workspace walker (ampligraph_amd/csrc/kge_layout.h), driven by tests/test_layout_host.py and built with
// -fsanitize=address,undefined: every region a walk hands out is written in full inside a heap block of EXACTLY the size the walk
// reports, so a region that leaves the buffer is an AddressSanitizer report, and a size that wraps is an UndefinedBehaviorSanitizer one.
// usage: layout_check CASE ; prints "ok CASE <checks>" and exits 0, or the failed check and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../ampligraph_amd/csrc/kge_layout.h"

using kge::Layout;

static long g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

struct Region { int64_t off, bytes; };

// a walk over `sizes` on `align`: offsets aligned, regions in order and disjoint, end() and next() as documented
static std::vector<Region> walk(Layout& l, int64_t align, const std::vector<int64_t>& sizes) {
    std::vector<Region> r;
    int64_t prev_end = 0;
    for (int64_t b : sizes) {
        const int64_t at = l.take(b);
        CHECK(l.ok());
        CHECK(at % align == 0);
        CHECK(at >= prev_end && at - prev_end < align);
        CHECK(l.end() == at + b);
        CHECK(l.next() == kge::round_up(at + b, align) && l.next() - l.end() < align);
        prev_end = at + b;
        r.push_back({at, b});
    }
    return r;
}

// a heap block whose usable part starts `behind` bytes behind a 256-byte boundary and is EXACTLY `bytes` long: base + bytes is the end
// of the block the sanitizer knows
struct Block {
    char *raw = nullptr, *base;
    Block(int64_t behind, int64_t bytes) {
        void* p = nullptr;
        CHECK(posix_memalign(&p, 256, (size_t)(behind + bytes)) == 0);
        raw = (char*)p;
        base = raw + behind;
    }
    ~Block() { free(raw); }
};

static void case_alignments() {
    for (int64_t align : {4, 8, 256}) {
        Layout l(align);
        walk(l, align, {1, 3, 4, 5, 255, 256, 257, 1000, 7});
        Layout c(align);   // take(count, each) is take(count * each)
        CHECK(c.take(3, 5) == 0 && c.end() == 15);
        CHECK(c.take(7, 8) == kge::round_up(15, align) && c.end() == kge::round_up(15, align) + 56);
    }
    CHECK(kge::round_up(0) == 0 && kge::round_up(1) == 256 && kge::round_up(256) == 256 && kge::round_up(257) == 512);
    CHECK(kge::round_up(5, 4) == 8 && kge::round_up(8, 8) == 8 && kge::round_up(9, 8) == 16);
    Layout d;   // the default alignment is 256
    d.take(1);
    CHECK(d.take(1) == 256);
}

static void case_zero_length() {
    for (int64_t align : {4, 8, 256}) {
        Layout l(align);
        CHECK(l.take(0) == 0 && l.end() == 0 && l.next() == 0);
        CHECK(l.take(0) == 0);
        CHECK(l.take(5) == 0);
        const int64_t z = l.take(0);   // an empty region sits where the next one starts and moves nothing but the rounding
        CHECK(z == kge::round_up(5, align) && l.end() == z && l.next() == z);
        CHECK(l.take(0, 16) == z && l.take(16, 0) == z);
        CHECK(l.take(9) == z && l.end() == z + 9);
        CHECK(l.ok());
    }
}

static void case_bases() {
    for (int64_t behind : {0, 16, 255}) {
        Layout l;
        const std::vector<Region> regions = walk(l, 256, {40, 0, 256, 1, 4096 + 12, 77});
        // sized for any base: the last region as long as it was taken (end) and filled up to the alignment (next)
        for (int64_t need : {l.end(), l.next()}) {
            const int64_t total = l.any_base(need);
            CHECK(total == need + 256);
            Block b(behind, total);
            CHECK(((uintptr_t)b.base & 255) == (uintptr_t)behind);
            char* w = kge::aligned_base(b.base);
            CHECK(((uintptr_t)w & 255) == 0);
            CHECK(w - b.base == kge::base_pad(b.base) && kge::base_pad(b.base) == (256 - behind) % 256);
            for (const Region& r : regions) {
                CHECK(w + r.off + r.bytes <= b.base + total);
                memset(w + r.off, 0xA5, (size_t)r.bytes);   // (outside the block: an AddressSanitizer report)
            }
        }
        // a base that the library does not align: alignment 4 and 8 walks start at the caller's pointer
        for (int64_t align : {4, 8}) {
            Layout s(align);
            const std::vector<Region> rs = walk(s, align, {12, 4, 0, 20, 8});
            Block b(behind, s.end());
            for (const Region& r : rs) memset(b.base + r.off, 0x5A, (size_t)r.bytes);
            CHECK(kge::base_pad(b.base, 1) == 0 && kge::aligned_base(b.base, 1) == b.base);
        }
    }
    CHECK(kge::base_pad(nullptr) == 0);
}

static void case_rest() {
    Layout l;
    l.take(256);
    l.take(1000);   // fixed part: 256 + 1024
    const int64_t fixed = l.next();
    CHECK(fixed == 1280);
    CHECK(l.rest(0, 8) == 0);
    CHECK(l.rest(-5, 8) == 0);                    // (a buffer shorter than the bytes skipped to align its base)
    CHECK(l.rest(fixed - 1, 8) == 0);             // shorter than the fixed part: no list, and no negative count
    CHECK(l.rest(100, 8) == 0);
    CHECK(l.rest(fixed, 8) == 0);
    CHECK(l.rest(fixed + 7, 8) == 0);
    CHECK(l.rest(fixed + 8, 8) == 1);
    CHECK(l.rest(fixed + 8 * 1000 + 7, 8) == 1000);
    CHECK(l.rest(fixed + 80, 0) == 0);
    CHECK(l.rest(INT64_MAX, 8) == (INT64_MAX - fixed) / 8);
    // the list that rest() sizes lies inside the buffer, whatever the base
    for (int64_t behind : {0, 16, 255}) {
        const int64_t bytes = fixed + 8 * 100 + 256 + 3;
        Block b(behind, bytes);
        const int64_t cap = l.rest(bytes - kge::base_pad(b.base), 8);
        CHECK(cap >= 100 && cap <= 100 + 32);
        char* w = kge::aligned_base(b.base);
        CHECK(w + fixed + cap * 8 <= b.base + bytes && w + fixed + (cap + 1) * 8 > b.base + bytes);
        memset(w + fixed, 0x11, (size_t)(cap * 8));
    }
}

static void case_overflow() {
    const int64_t big = INT64_MAX;
    {   // the sum of two regions
        Layout l;
        CHECK(l.take(big - 1000) == 0 && l.ok());
        CHECK(l.take(2000) == -1 && !l.ok());
        CHECK(l.end() == -1 && l.next() == -1 && l.any_base(l.end()) == -1 && l.rest(big, 8) == 0);
        CHECK(l.take(1) == -1 && !l.ok());   // the report sticks
    }
    {   // count * each
        Layout l(8);
        CHECK(l.take((int64_t)1 << 62, 4) == -1 && !l.ok() && l.end() == -1);
    }
    {   // the rounding of the last region, and the alignment unit of any_base
        Layout l;
        CHECK(l.take(big - 3) == 0 && l.ok() && l.end() == big - 3);
        CHECK(l.next() == -1);
        CHECK(l.any_base(l.end()) == -1);
        CHECK(l.take(1) == -1 && !l.ok());   // (no aligned offset for another region)
    }
    {   // near 2^63 and still representable
        Layout l(8);
        CHECK(l.take(((int64_t)1 << 62) - 8, 2) == 0 && l.ok());
        CHECK(l.end() == big - 15 && l.next() == big - 15);   // (2^63 - 16: a multiple of 8)
        CHECK(l.any_base(l.next()) == big - 7);
        CHECK(l.rest(big, 8) == 1);
    }
    {   // negative sizes are refused, not walked backwards
        Layout l;
        l.take(512);
        CHECK(l.take(-1) == -1 && !l.ok());
        Layout m;
        CHECK(m.take(-4, 4) == -1 && !m.ok());
        Layout n;
        CHECK(n.take(4, -4) == -1 && !n.ok());
        CHECK(n.any_base(-1) == -1);
    }
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "alignments") case_alignments();
    else if (which == "zero_length") case_zero_length();
    else if (which == "bases") case_bases();
    else if (which == "rest") case_rest();
    else if (which == "overflow") case_overflow();
    else { printf("unknown case '%s'\n", which.c_str()); return 2; }
    printf("ok %s %ld\n", which.c_str(), g_checks);
    return 0;
}
