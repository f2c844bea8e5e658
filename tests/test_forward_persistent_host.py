"""The persistent forward kernels without a GPU: the resources of every STAGE = true, one-wave-per-positive instantiation of
train_fwdbwd_kernel from the built code object."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ampligraph_amd", "lib", "libamdkge.so")
# train_fwdbwd_kernel<MODEL, 4, W = 1, CH, STAGE = true, DET>
PERSISTENT = re.compile(r"^_ZN3kge19train_fwdbwd_kernelILi(\d)ELi4ELi1ELi([12])ELb1ELb([01])EEEvNS_9TrainArgsE$")
C2 = "_ZN3kge19train_fwdbwd_kernelILi2ELi4ELi1ELi1ELb1ELb0EEEvNS_9TrainArgsE"   # ComplEx, one quad per lane, default mode


def test_persistent_forward_kernels_use_no_scratch_and_c2_keeps_three_waves():
    from ampligraph_amd.utils.codeobj import kernel_resources

    assert os.path.exists(LIB), "library not built: run build() first"
    res = kernel_resources(LIB)
    mine = {n: k for n, k in res.items() if PERSISTENT.match(n)}
    # four staged models x one or two quads per lane x the deterministic variant
    assert len(mine) == 16 and C2 in mine, sorted(mine)
    for n, k in mine.items():
        assert k["scratch"] == 0, (n, k)
    assert mine[C2]["vgpr"] <= 168 and mine[C2]["waves_per_simd"] >= 3, mine[C2]
