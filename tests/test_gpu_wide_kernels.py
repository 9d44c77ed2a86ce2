"""Single-process parity of the fold kernels with XMPI_SUM_WIDE on the MI355X (tests/wide_scenarios.py sc_kernels):
xmpi_reduce_local_n and xmpi_reduce_local_multi, 1..9 and 16 sources (every unrolled count and the run-time-count kernel), 1 / 2 / 8
destinations with one aliasing a source, {1, 7, 8, 9, 1000, 4099, 65536 + 5} elements, aligned and one element behind a 16-byte
boundary, kernel_mode 0 / 1 / 2 and a capped grid -- against the numpy restatement of the operator.  This is where the hardware's
f32 subnormal handling and its f32 -> f16 conversion are held to numpy's.

The job of one rank runs in a child process (tests/wide_worker.py): the test runner itself never opens the GPU, so the 8-process
tests of the other modules do not find a ninth process there."""
import pytest

from mpi_amd import xmpi
from tests.wide_harness import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [xmpi.F16, xmpi.BF16])
def test_local_kernels(dtype):
    outs = run_ranks("kernels", 1, {"dtype": dtype}, timeout=240)
    assert "launches checked" in outs[0]
