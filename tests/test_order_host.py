"""CPU test of ampligraph_amd/csrc/kge_order.h, the ordering helpers every selection and filter lookup on the device shares: the header
compiled with g++ into a small harness (tests/csrc/order_check.cpp).
  keys     : unsortable(sortable(v)) == v bit for bit and sortable strictly monotone over +-0, denormals, +-inf, the largest and smallest
             finite values and 4 000 random bit patterns; every NaN maps to key 0, below everything.
  contains : sorted_contains<int> (a range staged in LDS) and sorted_contains<int64_t> (a range in global memory) against
             std::binary_search on ascending arrays of 0, 1, 2, 63, 64, 65 and 1 000 ids with duplicates, every id from min - 1 to max + 1,
             whole arrays and sub-ranges [lo, hi) that start and end inside them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("order") / "order_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "order_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("what", ["keys", "contains"])
def test_order_helpers(harness, what):
    out = subprocess.run([harness, what], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 failed checks"), out.stdout[-2000:]
