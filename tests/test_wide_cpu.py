"""XMPI_SUM_WIDE without the library: the numpy restatement (tests/wide_ref.py) against hand-computed cases, and the two facts the
operator rests on, reproduced from the suite's own inputs (tests/hard_inputs.py, 4099 elements) -- with 2 sources it IS XMPI_SUM,
with 3 / 4 / 8 it differs in a large share of dense elements.  The second keeps a SUM_WIDE that quietly aliases SUM from passing
the tests that compare the library with this reference."""
import numpy as np
import pytest

from mpi_amd import xmpi
from tests import hard_inputs as hi
from tests import wide_ref as wr

N = 4099


def _bits(dtype, *patterns):
    return [hi.from_bits(np.array([p], dtype=np.uint16), dtype) for p in patterns]


def _one(dtype, *patterns):
    return int(hi.bits_of(wr.wide_sum(_bits(dtype, *patterns), dtype), dtype)[0])


def _narrow_sum(dtype, *patterns):
    return int(hi.bits_of(hi.np_reduce_ranks(_bits(dtype, *patterns), dtype, xmpi.SUM), dtype)[0])


def test_the_enumerator():
    assert xmpi.SUM_WIDE == 4 and (xmpi.SUM, xmpi.PROD, xmpi.MIN, xmpi.MAX) == (0, 1, 2, 3)


def test_hand_computed_bf16():
    one, half_ulp, maxfin, inf = 0x3F80, 0x3B80, 0x7F7F, 0x7F80  # 1, 2^-8 (half an ulp of 1: 7 mantissa bits), max finite, +Inf
    # 1 + 2^-8 + 2^-8: rounding after each source ties to even twice and stays 1; accumulated wide it is 1 + 2^-7
    assert _narrow_sum(xmpi.BF16, one, half_ulp, half_ulp) == one
    assert _one(xmpi.BF16, one, half_ulp, half_ulp) == 0x3F81
    # maxfin + maxfin - maxfin: bf16 has f32's exponent range, so the accumulator overflows where the type does -- Inf either way
    # (f16 below is where the wide accumulator holds the sum)
    assert _narrow_sum(xmpi.BF16, maxfin, maxfin, 0x8000 | maxfin) == inf
    assert _one(xmpi.BF16, maxfin, maxfin, 0x8000 | maxfin) == inf
    # 256 + 1 + 1: 257 is halfway between 256 and 258 -- stays 256 twice; wide: 258 (256 = 0x4380, 258 = 0x4381)
    assert _narrow_sum(xmpi.BF16, 0x4380, one, one) == 0x4380
    assert _one(xmpi.BF16, 0x4380, one, one) == 0x4381
    # order: (2^24 + 1) + -2^24 loses the 1 in f32, 2^24 + -2^24 + 1 keeps it (2^24 = 0x4B80)
    assert _one(xmpi.BF16, 0x4B80, one, 0xCB80) == 0x0000
    assert _one(xmpi.BF16, 0x4B80, 0xCB80, one) == one
    # zeros: -0 + -0 = -0, -0 + +0 = +0; Inf - Inf is NaN; a NaN stays one; a subnormal survives (f32 keeps it, nothing is flushed)
    assert _one(xmpi.BF16, 0x8000, 0x8000, 0x8000) == 0x8000
    assert _one(xmpi.BF16, 0x8000, 0x0000, 0x8000) == 0x0000
    assert hi.is_nan(wr.wide_sum(_bits(xmpi.BF16, inf, 0xFF80, one), xmpi.BF16), xmpi.BF16)[0]
    assert hi.is_nan(wr.wide_sum(_bits(xmpi.BF16, one, 0x7F81, one), xmpi.BF16), xmpi.BF16)[0]
    assert _one(xmpi.BF16, 0x0001, 0x0001, 0x0001) == 0x0003


def test_hand_computed_f16():
    one, half_ulp, maxfin, inf = 0x3C00, 0x1000, 0x7BFF, 0x7C00  # 1, 2^-11 (half an ulp of 1: 10 mantissa bits), 65504, +Inf
    assert _narrow_sum(xmpi.F16, one, half_ulp, half_ulp) == one
    assert _one(xmpi.F16, one, half_ulp, half_ulp) == 0x3C01
    assert _narrow_sum(xmpi.F16, maxfin, maxfin, 0x8000 | maxfin) == inf
    assert _one(xmpi.F16, maxfin, maxfin, 0x8000 | maxfin) == maxfin
    assert _one(xmpi.F16, maxfin, maxfin, one) == inf  # 131009 is beyond the type: the ONE narrowing overflows
    assert _one(xmpi.F16, 0x8000, 0x8000, 0x8000) == 0x8000
    assert _one(xmpi.F16, 0x8000, 0x0000, 0x8000) == 0x0000
    assert _one(xmpi.F16, 0x0001, 0x0001, 0x0001) == 0x0003  # subnormals of the type are normal f32 values
    assert _one(xmpi.F16, 0x0001, 0x83FF, 0x0400) == 0x0002   # 2^-24 - 1023 x 2^-24 + 1024 x 2^-24
    assert hi.is_nan(wr.wide_sum(_bits(xmpi.F16, inf, 0xFC00, one), xmpi.F16), xmpi.F16)[0]


@pytest.mark.parametrize("dtype", wr.WIDE_DTYPES)
def test_one_source_is_a_copy_and_other_types_are_the_plain_sum(dtype):
    x = hi.special(dtype, N, 9100, 0, 2)
    assert wr.wide_sum([x], dtype).tobytes() == x.tobytes()  # signalling NaNs included: nothing is converted
    for other in (xmpi.F32, xmpi.F64):
        ins = hi.rank_inputs(other, 257, 9200, 3, xmpi.SUM, "dense")
        assert wr.wide_sum(ins, other).tobytes() == hi.np_reduce_ranks(ins, other, xmpi.SUM).tobytes()


@pytest.mark.parametrize("kind", ["special", "dense"])
@pytest.mark.parametrize("dtype", wr.WIDE_DTYPES)
def test_with_two_sources_wide_is_the_plain_sum_everywhere(dtype, kind):
    """f32 holds the exact sum of two 16-bit floats to within one rounding that the second cannot undo (24 >= 2 p + 2 for p = 11 and
    p = 8): rounding once from f32 and rounding the exact sum give the same bits -- which is why xmpi_reduce_local maps the operator"""
    ins = hi.rank_inputs(dtype, N, 9300, 2, xmpi.SUM, kind)
    hi.same_floats(wr.wide_sum(ins, dtype), hi.np_reduce_ranks(ins, dtype, xmpi.SUM), dtype, xmpi.SUM, f"2 sources {kind}")
    assert wr.differing(wr.wide_sum(ins, dtype), hi.np_reduce_ranks(ins, dtype, xmpi.SUM), dtype) == 0


@pytest.mark.parametrize("size", [3, 4, 8])
@pytest.mark.parametrize("dtype", wr.WIDE_DTYPES)
def test_with_more_sources_wide_differs_from_the_plain_sum(dtype, size):
    """measured on these inputs: 20 / 30 / 47 % of 4099 dense elements; asserted: at least 10 %"""
    ins = hi.rank_inputs(dtype, N, 9400, size, xmpi.SUM, "dense")
    d = wr.differing(wr.wide_sum(ins, dtype), hi.np_reduce_ranks(ins, dtype, xmpi.SUM), dtype)
    print(f"{xmpi.DTYPE_NAME[dtype]} {size} sources: {d} of {N} elements differ ({100.0 * d / N:.1f} %)")
    assert d >= N // 10, f"{d} of {N}"
    special = hi.rank_inputs(dtype, N, 9400, size, xmpi.SUM, "special")
    assert wr.differing(wr.wide_sum(special, dtype), hi.np_reduce_ranks(special, dtype, xmpi.SUM), dtype) > 0
