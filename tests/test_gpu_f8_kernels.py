"""Single-process parity of the fold kernels with XMPI_F8E4M3 / XMPI_F8E5M2 on the MI355X (tests/f8_scenarios.py sc_kernels): every
pair of encodings through xmpi_reduce_local and through xmpi_reduce_local_n with 2, 3, 8 and 16 sources, under SUM, PROD, MIN, MAX
and SUM_WIDE; the midpoints between neighbouring values of the format and the values just off them as a three-source sum (v + ulp/2
+- the smallest subnormal: rounding and stickiness in isolation); xmpi_reduce_local_n / _multi / _batch at {1, 7, 8, 9, 15, 16, 17,
1000, 4099, 32768, 32769, 65536 + 5} elements, aligned and one element behind a 16-byte boundary; kernel_mode 0 / 1 / 2 and a capped
grid -- against the numpy restatement of the types (tests/f8_ref.py).  This is where v_cvt_pk_f32_fp8 / _bf8 and v_cvt_pk_fp8_f32 /
_bf8_f32 behind their explicit clamp are held to the software definition: if the hardware disagrees anywhere, the kernel is what is
fixed.

The job of one rank runs in a child process (tests/f8_worker.py): the test runner itself never opens the GPU, so the 8-process tests
of the other modules do not find a ninth process there."""
import pytest

from tests import f8_ref as fr
from tests.f8_harness import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
def test_local_kernels(dtype):
    outs = run_ranks("kernels", 1, {"dtype": dtype}, timeout=120)
    assert "launches checked" in outs[0]
