"""CPU test of the workspace walker (ampligraph_amd/csrc/kge_layout.h), the one place where every *_workspace_bytes function and every
entry point that carves the buffer get their regions from: the product's own header, compiled with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer into a stand-alone harness (tests/csrc/layout_check.cpp) that writes every region of a walk in full inside
a heap block of exactly the reported size.  A region outside its buffer, or a size that wraps, ends the harness with a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# alignments 4 / 8 / 256; zero-length regions; a base 0, 16 and 255 bytes behind a 256-byte boundary; rest() with a buffer shorter
# than the fixed part (cap == 0, never negative); sizes near 2^63 (the overflow report)
CASES = ["alignments", "zero_length", "bases", "rest", "overflow"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "layout_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "layout_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("case", CASES)
def test_walker(harness, case):
    r = subprocess.run([harness, case], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, name, checks = r.stdout.split()
    assert (word, name) == ("ok", case) and int(checks) > 0


def test_an_unknown_case_is_not_a_pass(harness):
    assert subprocess.run([harness, "no_such_case"], capture_output=True).returncode == 2
