"""XMPI_SUM_WIDE restated in numpy (helper module, no conftest): the expectation of every test of the operator.

The oracle (oracle/xmpi_oracle.c) has the reference's four operators and cannot grow a fifth, so the definition of include/xmpi.h is
spelled out here, independently of the kernels:

    narrow( ((f32(x0) + f32(x1)) + f32(x2)) + ... + f32(xN-1) )          f16 / bf16, N >= 2 sources, in rank order

  widen    bf16: the 16 bits shifted into the top half of an f32; f16: astype(float32).  Exact for both.
  add      numpy float32 additions, left to right: IEEE, subnormals kept.
  narrow   ONCE.  bf16: round to nearest even on the bit pattern, a NaN keeps its top 16 bits with the quiet bit set (the rounding
           tests/hard_inputs.py np_reduce2 spells for the two-operand sum); f16: astype(float16), round to nearest even.
  N == 1   the source, unchanged.
For every other dtype the operator IS XMPI_SUM: np_reduce_ranks.

Compare with hard_inputs.same_floats(got, want, dtype, xmpi.SUM): the same set of NaN positions, every other element bit for bit.
Arrays come in the suite's numpy types (bf16 as uint16 bit patterns)."""
from __future__ import annotations

import numpy as np

from mpi_amd import xmpi
from tests import hard_inputs as hi

WIDE_DTYPES = (xmpi.F16, xmpi.BF16)


def widen(a: np.ndarray, dtype: int) -> np.ndarray:
    if dtype == xmpi.BF16:
        return (np.ascontiguousarray(a).astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert dtype == xmpi.F16, dtype
    return np.ascontiguousarray(a).astype(np.float32)


def narrow(f: np.ndarray, dtype: int) -> np.ndarray:
    assert f.dtype == np.float32
    with np.errstate(all="ignore"):
        if dtype == xmpi.F16:
            return f.astype(np.float16)
        assert dtype == xmpi.BF16, dtype
        u = np.ascontiguousarray(f).view(np.uint32)
        nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
        rounded = (u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)
        return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rounded.astype(np.uint32)).astype(np.uint16)


def wide_sum(ins, dtype: int) -> np.ndarray:
    """XMPI_SUM_WIDE over the sources `ins`, in their order"""
    if dtype not in WIDE_DTYPES:
        return hi.np_reduce_ranks(list(ins), dtype, xmpi.SUM)
    if len(ins) == 1:
        return np.array(ins[0], copy=True)
    with np.errstate(all="ignore"):
        acc = widen(ins[0], dtype)
        for x in ins[1:]:
            acc = acc + widen(x, dtype)
    assert acc.dtype == np.float32
    return narrow(acc, dtype)


def differing(a: np.ndarray, b: np.ndarray, dtype: int) -> int:
    """elements whose bits differ, NaNs made one NaN first"""
    return int(np.sum(hi.nan_normalised(a, dtype) != hi.nan_normalised(b, dtype)))
