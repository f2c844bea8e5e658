"""CPU test of the once-per-device logic behind ensure_dynamic_lds (ampligraph_amd/csrc/kge_once.h, wrapped by kge_host.h with
hipGetDevice / hipFuncSetAttribute): the product's own header, compiled with g++ into a small harness (tests/csrc/once_check.cpp) that
runs host threads per device through ONE PerDeviceOnce, as a session group does through the static object in front of every large-LDS
launch.  The device ordinal used to live in the shared object: one thread's "done" could mark another thread's device, whose set-up
had failed or not happened."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("once") / "once_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "once_check.cpp"), "-o", exe], check=True)
    return exe


def run(harness, D, T, C, failing, fail_first):
    text = f"{D} {T} {C} {len(failing)} " + " ".join(map(str, failing)) + f" {fail_first}\n"
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == D
    return [tuple(int(v) for v in l.split()) for l in out]


@pytest.mark.parametrize("D,T,C", [(1, 1, 5), (8, 1, 50), (8, 4, 200), (64, 2, 20)])
def test_every_device_is_set_up_and_a_marked_device_is_not_set_up_again(harness, D, T, C):
    for ok, failed, after_marked, marked, returned_false in run(harness, D, T, C, [], 0):
        assert 1 <= ok <= T            # at least once; racing threads of ONE device at worst each do the idempotent set-up
        assert failed == 0 and returned_false == 0
        assert after_marked == 0 and marked == 1


def test_a_device_whose_set_up_failed_is_not_marked(harness):
    D, T, C = 8, 2, 100
    failing = [1, 4, 7]
    rows = run(harness, D, T, C, failing, 10 ** 9)   # devices 1, 4, 7 never succeed, while the others' threads mark theirs
    for d, (ok, failed, after_marked, marked, returned_false) in enumerate(rows):
        if d in failing:
            assert ok == 0 and marked == 0 and failed == T * C and returned_false == T * C   # every call tried again and reported it
        else:
            assert 1 <= ok <= T and failed == 0 and marked == 1 and returned_false == 0
        assert after_marked == 0


def test_a_failed_set_up_is_retried_until_it_succeeds(harness):
    D, T, C = 4, 1, 20
    rows = run(harness, D, T, C, [2], 3)
    assert rows[2] == (1, 3, 0, 1, 3)
    for d in (0, 1, 3):
        assert rows[d] == (1, 0, 0, 1, 0)
