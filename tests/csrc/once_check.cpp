// CPU harness of the per-device "once" logic (ampligraph_amd/csrc/kge_once.h) behind ensure_dynamic_lds: the product's own header,
// driven as a session group drives it -- one host thread per device, all of them through ONE PerDeviceOnce -- with an injected
// "current device" and an injected "set attribute" that can fail.  No HIP, no GPU.
//
// stdin:  n_devices threads_per_device calls_per_thread n_failing f_0 f_1 ...   (devices whose FIRST fail_first set-ups fail) fail_first
// stdout: per device one line "successes failures set-ups_after_marked marked calls_returning_false"
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../ampligraph_amd/csrc/kge_once.h"

int main() {
    int D, T, C, NF, fail_first;
    if (scanf("%d %d %d %d", &D, &T, &C, &NF) != 4 || D < 1 || D > 64) return 2;
    std::vector<int> fails(D, 0);
    for (int i = 0; i < NF; ++i) { int f; if (scanf("%d", &f) != 1 || f < 0 || f >= D) return 2; fails[f] = 1; }
    if (scanf("%d", &fail_first) != 1) return 2;
    kge::PerDeviceOnce once;
    std::vector<std::atomic<int>> attempts(D), ok(D), failed(D), after_marked(D), returned_false(D);
    for (int d = 0; d < D; ++d) { attempts[d] = 0; ok[d] = 0; failed[d] = 0; after_marked[d] = 0; returned_false[d] = 0; }
    std::atomic<int> go{0};
    std::vector<std::thread> th;
    for (int d = 0; d < D; ++d)
        for (int t = 0; t < T; ++t)
            th.emplace_back([&, d] {
                while (!go.load()) std::this_thread::yield();
                for (int c = 0; c < C; ++c) {
                    const bool marked_before = (__atomic_load_n(&once.mask, __ATOMIC_ACQUIRE) >> d) & 1ull;
                    bool ran = false;
                    const bool r = once.run([&] { return d; },
                                            [&] {
                                                ran = true;
                                                const int a = attempts[d].fetch_add(1);
                                                if (fails[d] && a < fail_first) { failed[d]++; return false; }
                                                ok[d]++;
                                                return true;
                                            });
                    if (ran && marked_before) after_marked[d]++;   // a marked device is never set up again
                    if (!r) returned_false[d]++;
                    std::this_thread::yield();
                }
            });
    go = 1;
    for (auto& t : th) t.join();
    for (int d = 0; d < D; ++d)
        printf("%d %d %d %d %d\n", ok[d].load(), failed[d].load(), after_marked[d].load(), (int)((once.mask >> d) & 1ull), returned_false[d].load());
    return 0;
}
