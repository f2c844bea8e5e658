"""The GPU twin of tests/test_workspace_sizes_host.py: amdkge_filter_build_workspace_bytes and amdkge_step_rows_workspace_bytes ask
rocPRIM for the size of its scratch, which needs a device.  Same table, same rule (both are group A: equal to the record)."""
import pytest

from test_workspace_sizes_host import DEVICE_FUNCTIONS, check_function

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fn", DEVICE_FUNCTIONS)
def test_sizes_against_the_record(gpu_lib, fn):
    assert check_function(gpu_lib, fn) > 0
