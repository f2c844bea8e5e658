// The layout of a device workspace, walked ONCE: the *_workspace_bytes function of a buffer and every entry point that touches the
// buffer read the same walk, so the size a caller is told and the regions a kernel is handed cannot disagree.
// Pure C++ (no HIP types), as kge_once.h: tests/test_layout_host.py compiles it into a CPU harness under the sanitizers.
// A walk is over OFFSETS; a pointer is formed only at the end, from the caller's base (aligned_base), so nothing here does arithmetic
// on a null pointer.  Sizes are int64 and an overflow is reported (ok() == false, every total -1), never wrapped.
#pragma once
#include <stdint.h>

namespace kge {

// THE round-up: x to the next multiple of a (a power of two, x >= 0, x + a - 1 representable)
constexpr int64_t round_up(int64_t x, int64_t a = 256) { return (x + a - 1) & ~(a - 1); }

// Where the library starts a workspace that it aligns up itself: the first `a`-byte boundary at or behind `base`.  Such a buffer is
// sized with Layout::any_base(), which covers the bytes skipped here whatever the base's alignment.
inline int64_t base_pad(const void* base, int64_t a = 256) { return (int64_t)(-(uintptr_t)base & (uintptr_t)(a - 1)); }
inline char* aligned_base(void* base, int64_t a = 256) { return (char*)base + base_pad(base, a); }

class Layout {
  public:
    explicit Layout(int64_t align = 256) : align_(align) {}
    // the offset of the next region: `bytes` bytes (resp. `count` elements of `each` bytes) from the next multiple of the alignment
    int64_t take(int64_t bytes) {
        const int64_t at = next();
        if (bytes < 0 || at < 0 || __builtin_add_overflow(at, bytes, &end_)) return fail();
        return at;
    }
    int64_t take(int64_t count, int64_t each) {
        int64_t bytes;
        return (count < 0 || each < 0 || __builtin_mul_overflow(count, each, &bytes)) ? fail() : take(bytes);
    }
    // the elements of `elem` bytes that fit between next() and the end of a buffer of `total_bytes` (counted from the aligned base):
    // for a list that takes what is left.  A buffer shorter than the regions taken so far holds none.
    int64_t rest(int64_t total_bytes, int64_t elem) const {
        const int64_t at = next();
        return (at < 0 || elem < 1 || total_bytes <= at) ? 0 : (total_bytes - at) / elem;
    }
    bool ok() const { return ok_; }
    int64_t end() const { return ok_ ? end_ : -1; }   // bytes behind an aligned base, the last region as long as it was taken
    int64_t next() const {                            // ... with the last region filled up to the alignment: where another would start
        int64_t e;
        return (!ok_ || __builtin_add_overflow(end_, align_ - 1, &e)) ? -1 : (e & ~(align_ - 1));
    }
    // `bytes` (an end() or a next()) for a base of ANY alignment: one alignment unit on top
    int64_t any_base(int64_t bytes) const {
        int64_t t;
        return (bytes < 0 || __builtin_add_overflow(bytes, align_, &t)) ? -1 : t;
    }

  private:
    int64_t fail() { ok_ = false; return -1; }
    int64_t align_, end_ = 0;
    bool ok_ = true;
};

}  // namespace kge
