// "Once per device" for set-up that belongs to (function, DEVICE), such as a kernel's dynamic-LDS limit: a process may drive several
// devices (session groups: one replica and one host thread per GPU), so a process-wide `static bool` would set up device 0 only.
// Pure C++ (no HIP types): kge_host.h wraps it with hipGetDevice / hipFuncSetAttribute (ensure_dynamic_lds), and
// tests/test_per_device_once.py compiles it into a CPU harness that drives it from several threads.
#pragma once

namespace kge {

// One bit per device ordinal (mod 64).  The ordinal lives in a local of the caller's thread, never in the object: threads on different
// devices share the object, and a bit must only ever be set for the device whose set-up succeeded.  Racing threads of ONE device at
// worst both do the idempotent set-up.
struct PerDeviceOnce {
    unsigned long long mask = 0ull;

    // current_device() -> ordinal; set_up() -> true on success.  Returns false only if set_up ran and failed (the device stays
    // unmarked, so the next call tries again).
    template <class CurrentDevice, class SetUp>
    bool run(CurrentDevice&& current_device, SetUp&& set_up) {
        const unsigned long long bit = 1ull << (current_device() & 63);
        if (__atomic_load_n(&mask, __ATOMIC_ACQUIRE) & bit) return true;
        if (!set_up()) return false;
        __atomic_fetch_or(&mask, bit, __ATOMIC_RELEASE);
        return true;
    }
};

}  // namespace kge
