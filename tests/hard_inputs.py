"""Float inputs on which a kernel's fold ORDER and its handling of SPECIAL values show (helper module, no conftest).

oracle_fill's patterns are finite, normal, short-mantissa values: an f32 / f64 sum of 16 PAT_SIGNED values is exact in every
association, so a test on them that says "left to right" passes for any order, and no NaN, Inf, -0 or subnormal ever reaches a
kernel.  The inputs here are the complement:

  dense(dtype, n, seed, spread)          random sign, FULL random mantissa, biased exponent uniform in bias +- spread
  SPECIALS[dtype]                        16 bit patterns: zeros, infinities, quiet and signalling NaNs, subnormals, extremes
  special(dtype, n, seed, rank, size)    dense(seed + rank) with those planted so that every ordered pair meets
  same_floats(got, want, dtype, op)      the comparison that goes with them

Everything is a function of np_hash (tests/scenarios.py: the numpy restatement of oracle_hash), not of numpy's generators: every
rank rebuilds every rank's input, on any numpy.  Arrays come in the suite's numpy types (bf16 as uint16 bit patterns)."""
from __future__ import annotations

import numpy as np

from mpi_amd import xmpi

FLOATS = (xmpi.F16, xmpi.F32, xmpi.F64, xmpi.BF16)
# dtype -> (unsigned type of the bit pattern, mantissa bits, exponent bits)
LAYOUT = {xmpi.F16: (np.uint16, 10, 5), xmpi.BF16: (np.uint16, 7, 8), xmpi.F32: (np.uint32, 23, 8), xmpi.F64: (np.uint64, 52, 11)}
SPREAD_SUM, SPREAD_PROD = 6, 1  # 8 ranks of 2^+-6 cannot overflow f16 by a sum; 16 factors below 4 stay far inside every type but f16
PLANTED = 768  # elements [0, 768): the three blocks of 256 ordered pairs
STRIDE = 7     # beyond them every 7th element: against 16-byte packets and 8-byte LL line halves it visits every lane position
_PLANT_SALT = 0x5BD1E995


def _hash(seed: int, idx: np.ndarray) -> np.ndarray:
    from tests import scenarios  # (at call time: tests/scenarios.py imports this module)
    return scenarios.np_hash(seed, idx)


def _bias(dtype: int) -> int:
    return (1 << (LAYOUT[dtype][2] - 1)) - 1


def bits_of(a: np.ndarray, dtype: int) -> np.ndarray:
    """the elements' bit patterns as unsigned integers (a view)"""
    return np.ascontiguousarray(a).view(LAYOUT[dtype][0])


def from_bits(bits: np.ndarray, dtype: int) -> np.ndarray:
    return np.ascontiguousarray(bits, dtype=LAYOUT[dtype][0]).view(xmpi.NUMPY_DTYPE[dtype])


def is_nan(a: np.ndarray, dtype: int) -> np.ndarray:
    ut, mb, eb = LAYOUT[dtype]
    b = bits_of(a, dtype)
    return (b & ut((1 << (mb + eb)) - 1)) > ut(((1 << eb) - 1) << mb)


def dense(dtype: int, n: int, seed: int, spread: int = SPREAD_SUM) -> np.ndarray:
    """n normal values: sign = bit 63 of the hash, mantissa = its low 10 / 7 / 23 / 52 bits (all of them random), biased exponent
    = bias - spread + (bits 52..62 scaled to 0 .. 2 spread)"""
    ut, mb, eb = LAYOUT[dtype]
    h = _hash(seed, np.arange(n, dtype=np.uint64))
    u = np.uint64
    sign = h >> u(63)
    mant = h & u((1 << mb) - 1)
    step = (((h >> u(52)) & u(0x7FF)) * u(2 * spread + 1)) >> u(11)
    exp = u(_bias(dtype) - spread) + step
    bits = (sign << u(mb + eb)) | (exp << u(mb)) | mant
    return from_bits(bits.astype(ut), dtype)


def _specials(dtype: int) -> np.ndarray:
    ut, mb, eb = LAYOUT[dtype]
    sign = 1 << (mb + eb)
    inf = ((1 << eb) - 1) << mb
    quiet = 1 << (mb - 1)
    maxfin = inf - 1
    one = _bias(dtype) << mb
    small = (_bias(dtype) - (12 if dtype == xmpi.F16 else 24)) << mb  # 2^-12 (f16: 2^-24 is no normal there) / 2^-24
    return np.array([
        0, sign,                            # 0, 1: +0, -0
        inf, sign | inf,                    # 2, 3: +Inf, -Inf
        inf | quiet | 0x15,                 # 4: +qNaN with a payload
        sign | inf | quiet | 0x2A,          # 5: -qNaN with a payload
        inf | 0x01, sign | inf | 0x33,      # 6, 7: signalling NaNs (quiet bit clear, payload non-zero)
        1, sign | ((1 << mb) - 1),          # 8, 9: the smallest subnormal, the largest negative subnormal
        1 << mb,                            # 10: the smallest normal
        maxfin, sign | maxfin,              # 11, 12: +-max finite
        one, sign | one,                    # 13, 14: +-1
        small,                              # 15: a small normal
    ], dtype=ut)


SPECIALS = {d: _specials(d) for d in FLOATS}
NAN_SLOTS = (4, 5, 6, 7)


def plan(n: int, seed: int, size: int):
    """where the specials go, the same on every rank: (index, rank, slot of SPECIALS) triples as three arrays.
    [0, 256): SPECIALS[i // 16] on rank 0 and SPECIALS[i % 16] on rank 1 -- every ordered pair as the first two operands;
    [256, 512): the same pairs on the last two ranks -- a special meets an accumulated value; [512, 768): on the first and the last
    rank; beyond, every 7th element and the last one hold a hashed special on a hashed rank."""
    idx, rank, slot = [], [], []
    i = np.arange(min(n, PLANTED), dtype=np.int64)
    k = i % 256
    first = np.where(i < 256, 0, np.where(i < 512, max(0, size - 2), 0))
    second = np.where(i < 256, min(1, size - 1), size - 1)
    for who, which in ((first, k // 16), (second, k % 16)):  # (one rank only: the later entry wins, as in special())
        idx.append(i)
        rank.append(who)
        slot.append(which)
    if n > PLANTED:
        j = np.arange(-(-PLANTED // STRIDE) * STRIDE, n, STRIDE, dtype=np.int64)
        if j.size == 0 or j[-1] != n - 1:
            j = np.append(j, n - 1)  # the element tail behind the last full packet always holds one
        h = _hash(seed ^ _PLANT_SALT, j.astype(np.uint64))
        idx.append(j)
        rank.append((h % np.uint64(size)).astype(np.int64))
        slot.append(((h >> np.uint64(8)) % np.uint64(16)).astype(np.int64))
    return np.concatenate(idx), np.concatenate(rank), np.concatenate(slot)


def special(dtype: int, n: int, seed: int, rank: int, size: int) -> np.ndarray:
    """rank `rank`'s input of a `size`-rank job: dense(dtype, n, seed + rank) with this rank's share of plan(n, seed, size) planted"""
    out = bits_of(dense(dtype, n, seed + rank, SPREAD_SUM), dtype).copy()
    idx, who, slot = plan(n, seed, size)
    mine = who == rank
    out[idx[mine]] = SPECIALS[dtype][slot[mine]]  # (duplicates: in order, the last one stays)
    return from_bits(out, dtype)


def rank_inputs(dtype: int, n: int, seed: int, size: int, op: int, kind: str = "special"):
    """every rank's input for one call: special data for SUM / MIN / MAX, dense(spread 1) for PROD and for kind == "dense" the dense
    data of the operation's spread"""
    if op == xmpi.PROD:
        return [dense(dtype, n, seed + r, SPREAD_PROD) for r in range(size)]
    if kind == "dense":
        return [dense(dtype, n, seed + r, SPREAD_SUM) for r in range(size)]
    return [special(dtype, n, seed, r, size) for r in range(size)]


def nan_normalised(a: np.ndarray, dtype: int) -> np.ndarray:
    """the bit patterns with every NaN replaced by one quiet NaN (what two correct sums may differ in is gone)"""
    ut, mb, eb = LAYOUT[dtype]
    b = bits_of(a, dtype).copy()
    b[is_nan(a, dtype)] = ut((((1 << eb) - 1) << mb) | (1 << (mb - 1)))
    return b


def same_floats(got: np.ndarray, want: np.ndarray, dtype: int, op: int, what: str = "") -> None:
    """MIN / MAX select: every byte equal, NaN payloads and the sign of a zero included.  SUM / PROD: the same SET of NaN positions
    (which NaN an addition returns -- the sign of a generated one, whose payload survives -- is the hardware's, not the library's)
    and every other element byte for byte: infinities, signed zeros and subnormals included.  No element is left out."""
    assert got.size == want.size, f"{what}: {got.size} elements, expected {want.size}"
    g, w = bits_of(got, dtype), bits_of(want, dtype)
    if op in (xmpi.SUM, xmpi.PROD):
        gn, wn = is_nan(got, dtype), is_nan(want, dtype)
        if not np.array_equal(gn, wn):
            i = int(np.nonzero(gn != wn)[0][0])
            raise AssertionError(f"{what}: {int(np.sum(gn != wn))} elements are NaN on one side only, first at {i}: got {g[i]:#x} want {w[i]:#x}")
        bad = (g != w) & ~wn
    else:
        bad = g != w
    if np.any(bad):
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(np.sum(bad))} of {g.size} elements differ in their bits ({xmpi.DTYPE_NAME[dtype]} op={op}), "
                             f"first at {i}: got {g[i]:#x} want {w[i]:#x}")


def np_reduce2(a: np.ndarray, b: np.ndarray, dtype: int, op: int) -> np.ndarray:
    """the two-operand combine restated in numpy, independent of oracle/xmpi_oracle.c: native arithmetic for f32 / f64; f16 in
    float64 (sum and product of two halves are exact there) rounded once; bf16 in f32, rounded to nearest even.  MIN is
    (b < a) ? b : a and MAX (a < b) ? b : a on the values, returning the chosen operand's bits."""
    with np.errstate(all="ignore"):
        if dtype == xmpi.BF16:
            x, y = (a.astype(np.uint32) << 16).view(np.float32), (b.astype(np.uint32) << 16).view(np.float32)
        elif dtype == xmpi.F16:
            x, y = a.astype(np.float64), b.astype(np.float64)
        else:
            x, y = a, b
        if op == xmpi.MIN:
            return np.where(y < x, b, a)
        if op == xmpi.MAX:
            return np.where(x < y, b, a)
        r = x + y if op == xmpi.SUM else x * y
        if dtype == xmpi.F16:
            return r.astype(np.float16)
        if dtype == xmpi.BF16:
            u = r.astype(np.float32).view(np.uint32)
            nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
            rounded = (u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)
            return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rounded.astype(np.uint32)).astype(np.uint16)
        return r


def np_reduce_ranks(ins, dtype: int, op: int) -> np.ndarray:
    acc = ins[0]
    for x in ins[1:]:
        acc = np_reduce2(acc, x, dtype, op)
    return acc
