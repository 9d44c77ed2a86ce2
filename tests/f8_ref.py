"""XMPI_F8E4M3 / XMPI_F8E5M2 restated in numpy: what include/xmpi.h says about the two OCP 8-bit floating-point formats and their five
operators, without the library.  Elements are bytes (np.uint8) throughout.

  decode(dtype)        the 256 values of a format as float32, computed from its layout (S.EEEE.MMM bias 7 / S.EEEEE.MM bias 15)
  widen(x, dtype)      f32(x): exact
  narrow(f, dtype)     NaN -> a NaN of the type (0x7F | sign); +-inf -> +-inf (E5M2; E4M3 has none: saturates); anything else to the
                       nearest value, ties to even, gradual underflow, and a rounded magnitude above the largest finite one becomes
                       +-448 / +-57344 (saturate-to-finite)
  reduce_ranks(xs, dtype, op)   SUM / PROD: acc = narrow(f32(acc) op f32(x_r)) in rank order; MIN / MAX: the widened values compared
                       with the library's expressions, the chosen operand's own byte returned; SUM_WIDE: IEEE f32 additions in rank
                       order, narrowed once; one contribution: a copy

narrow() works on the integer grid of the format, not by table search: a magnitude is scaled by a power of two into units of the
last place of its binade (exact in float64), rounded half to even with np.rint, and scaled back."""
from __future__ import annotations

import numpy as np

from mpi_amd import xmpi

F8_DTYPES = (xmpi.F8E4M3, xmpi.F8E5M2)
# mantissa bits, exponent bias, the largest finite byte, the NaN narrow() returns (without its sign)
LAYOUT = {xmpi.F8E4M3: (3, 7, 0x7E, 0x7F), xmpi.F8E5M2: (2, 15, 0x7B, 0x7F)}


def _decode_table(dtype) -> np.ndarray:
    mb, bias, _, _ = LAYOUT[dtype]
    out = np.empty(256, dtype=np.float64)
    for b in range(256):
        sign = -1.0 if b & 0x80 else 1.0
        e, m = (b & 0x7F) >> mb, b & ((1 << mb) - 1)
        if dtype == xmpi.F8E4M3 and (b & 0x7F) == 0x7F:
            v = np.nan
        elif dtype == xmpi.F8E5M2 and e == 31:
            v = np.inf if m == 0 else np.nan
        elif e == 0:
            v = m * 2.0 ** (1 - bias - mb)
        else:
            v = (1.0 + m * 2.0 ** -mb) * 2.0 ** (e - bias)
        out[b] = sign * v  # (-1.0 * 0.0 is -0.0, -1.0 * nan a NaN)
    t = out.astype(np.float32)
    assert np.array_equal(t.astype(np.float64), out, equal_nan=True)  # every value of either format is a float32
    t.setflags(write=False)
    return t


_TABLES = {d: _decode_table(d) for d in F8_DTYPES}


def decode(dtype) -> np.ndarray:
    return _TABLES[dtype]


def max_finite(dtype) -> float:
    return float(_TABLES[dtype][LAYOUT[dtype][2]])


def min_subnormal(dtype) -> float:
    return float(_TABLES[dtype][1])


def is_nan(x: np.ndarray, dtype) -> np.ndarray:
    return np.isnan(_TABLES[dtype][np.asarray(x, dtype=np.uint8)])


def widen(x: np.ndarray, dtype) -> np.ndarray:
    return _TABLES[dtype][np.asarray(x, dtype=np.uint8)]


def narrow(f: np.ndarray, dtype) -> np.ndarray:
    mb, bias, maxb, nanb = LAYOUT[dtype]
    f = np.asarray(f, dtype=np.float32)
    sign = ((f.view(np.uint32) >> 24) & 0x80).astype(np.uint8)
    a = np.abs(f.astype(np.float64))
    emin = 1 - bias
    with np.errstate(all="ignore"):
        finite = np.isfinite(a)
        safe = np.where(finite & (a > 0), a, 1.0)
        e = np.maximum(np.floor(np.log2(safe)).astype(np.int64), emin)  # the binade; everything below the smallest normal shares one
        e = np.where(safe < 2.0 ** e.astype(np.float64), e - 1, e)       # (log2 of a value just below a power of two may round up)
        e = np.maximum(e, emin)
        q = np.rint(safe * 2.0 ** (mb - e).astype(np.float64)).astype(np.int64)  # units of 2^(e - mb): exact scaling, half to even
        # q in [0, 2^(mb+1)]: q < 2^mb a subnormal, q == 2^(mb+1) a carry into the next binade -- the byte arithmetic takes both
        byte = np.where(q < (1 << mb), q, ((e + bias - 1) << mb) + q)
        byte = np.minimum(byte, maxb)  # saturate
    byte = np.where(a == 0, 0, byte)
    if dtype == xmpi.F8E5M2:
        byte = np.where(np.isinf(a), 0x7C, byte)
    else:
        byte = np.where(np.isinf(a), maxb, byte)
    byte = np.where(np.isnan(a), nanb, byte)
    return (byte.astype(np.uint8) | sign).astype(np.uint8)


def combine(a: np.ndarray, b: np.ndarray, dtype, op) -> np.ndarray:
    """one step of SUM / PROD / MIN / MAX: the accumulator `a` and the next rank's `b`, both bytes"""
    x, y = widen(a, dtype), widen(b, dtype)
    with np.errstate(all="ignore"):
        if op == xmpi.SUM:
            return narrow(x + y, dtype)  # (float32 + float32 in numpy is one IEEE f32 addition)
        if op == xmpi.PROD:
            return narrow(x * y, dtype)
        if op == xmpi.MIN:
            return np.where(y < x, b, a).astype(np.uint8)
        if op == xmpi.MAX:
            return np.where(x < y, b, a).astype(np.uint8)
    raise ValueError(op)


def reduce_ranks(xs, dtype, op) -> np.ndarray:
    xs = [np.asarray(x, dtype=np.uint8) for x in xs]
    if len(xs) == 1:
        return xs[0].copy()
    if op == xmpi.SUM_WIDE:
        acc = widen(xs[0], dtype).copy()
        with np.errstate(all="ignore"):
            for x in xs[1:]:
                acc = (acc + widen(x, dtype)).astype(np.float32)
        return narrow(acc, dtype)
    acc = xs[0]
    for x in xs[1:]:
        acc = combine(acc, x, dtype, op)
    return acc.copy()


def same(got: np.ndarray, want: np.ndarray, dtype, what: str = "") -> None:
    """the same set of NaN positions, every other element bit for bit"""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    assert got.shape == want.shape, f"{what}: {got.shape} against {want.shape}"
    gn, wn = is_nan(got, dtype), is_nan(want, dtype)
    if not np.array_equal(gn, wn):
        i = int(np.flatnonzero(gn != wn)[0])
        raise AssertionError(f"{what}: NaN positions differ, first at {i}: got 0x{int(got[i]):02X}, expected 0x{int(want[i]):02X}")
    bad = np.flatnonzero((got != want) & ~wn)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at {i}: got 0x{int(got[i]):02X}, expected 0x{int(want[i]):02X}")


def differing(a: np.ndarray, b: np.ndarray, dtype) -> int:
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return int(np.count_nonzero((a != b) & ~(is_nan(a, dtype) & is_nan(b, dtype))))


def finite_sorted(dtype) -> np.ndarray:
    """the non-negative finite values in increasing order: bytes 0x00 .. the largest finite one, as float32"""
    return _TABLES[dtype][:LAYOUT[dtype][2] + 1]
