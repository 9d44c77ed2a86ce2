"""XMPI_BAND / XMPI_BOR / XMPI_BXOR restated in numpy, and the inputs the bitwise suites use.

The operators: element i of the result is np.bitwise_and / _or / _xor over the ranks' element i (U8, I32, I64; signedness plays no
part).  They are exact, associative and commutative, so there is ONE expectation per job, whatever schedule ran.

The inputs: per rank and seed, full-width random words.  The density of set bits is chosen per operator so that the RESULT is
neither nearly all zeros nor nearly all ones for any rank count the suites use -- an AND of sparse words or an OR of dense ones would
be a constant that any wrong answer matches:
  BAND  dense inputs, about 0.5 ** (1 / N) per bit        BOR  sparse inputs, about 1 - 0.5 ** (1 / N)        BXOR  1 / 2
"About": a word of density 1 - 2 ** -k is the OR of k fair words (2 ** -k: their AND), and k is the one for which the expected share
of set bits in the result, (1 - 2 ** -k) ** N, lies nearest 1 / 2 -- 0.56 / 0.42 / 0.60 for N = 2 / 3 / 8 (k = 2 / 2 / 4), within the
[1 / 4, 3 / 4] that tests/test_bitop_cpu.py asserts.  The sign bit is a fair coin of its own in every element of every rank (about
half the elements are negative as I32 / I64), whatever the operator."""
from __future__ import annotations

import numpy as np

from mpi_amd import xmpi

DTYPES = (xmpi.U8, xmpi.I32, xmpi.I64)
FLOAT_DTYPES = (xmpi.F16, xmpi.F32, xmpi.F64, xmpi.BF16)
OPS = (xmpi.BAND, xmpi.BOR, xmpi.BXOR)
OP_NAME = {xmpi.BAND: "BAND", xmpi.BOR: "BOR", xmpi.BXOR: "BXOR"}
_UNSIGNED = {xmpi.U8: np.uint8, xmpi.I32: np.uint32, xmpi.I64: np.uint64}
_UFUNC = {xmpi.BAND: np.bitwise_and, xmpi.BOR: np.bitwise_or, xmpi.BXOR: np.bitwise_xor}


def words_per_draw(size: int) -> int:
    """k: how many fair words are OR-ed (BAND's inputs) or AND-ed (BOR's) into one input word"""
    return min(range(1, 8), key=lambda k: abs((1.0 - 2.0 ** -k) ** size - 0.5))


def bit_density(op: int, size: int) -> float:
    """the share of set bits in one rank's input (the sign bit apart)"""
    k = words_per_draw(size)
    return {xmpi.BAND: 1.0 - 2.0 ** -k, xmpi.BOR: 2.0 ** -k, xmpi.BXOR: 0.5}[op]


def rank_inputs(dtype: int, count: int, seed: int, size: int, op: int):
    """[rank] -> `count` elements of `dtype` for a job of `size` ranks reducing with `op`"""
    u = _UNSIGNED[dtype]
    bits = 8 * np.dtype(u).itemsize
    top = u(1) << u(bits - 1)
    rng = np.random.default_rng([seed, dtype, op, size, count])
    fair = lambda: rng.integers(0, 1 << 64, size=count, dtype=np.uint64).astype(u)  # (the low bits of a fair 64-bit word)
    k = words_per_draw(size)
    out = []
    for _ in range(size):
        x = fair()
        if op != xmpi.BXOR:
            for _ in range(k - 1):
                x = (x | fair()) if op == xmpi.BAND else (x & fair())
        x = (x & ~top) | (fair() & top)
        out.append(x.view(xmpi.NUMPY_DTYPE[dtype]))
    return out


def reduce_ranks(arrays, op: int) -> np.ndarray:
    return _UFUNC[op].reduce(np.stack(arrays), axis=0)


def set_bit_share(x: np.ndarray) -> float:
    b = x.view(np.uint8)
    return float(np.unpackbits(b).mean()) if b.size else 0.0


def differing(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.count_nonzero(a != b))
