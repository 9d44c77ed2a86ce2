"""The inputs of tests/hard_inputs.py and the reference they are judged by, pinned on the CPU (no GPU involved).

Why these inputs exist: PAT_SIGNED -- the pattern behind nearly every "bit-exact, rank order" float case of the suite -- sums
exactly in every association in f32 and f64 (test_pat_signed_sums_the_same_in_every_order measures 0 differing elements), so
those cases pass for any fold order; and no NaN, Inf, -0 or subnormal ever reached a kernel."""
import numpy as np
import pytest

from mpi_amd import xmpi
from oracle import oracle
from tests import hard_inputs as hi

FLOATS = list(hi.FLOATS)
OPS = [xmpi.SUM, xmpi.PROD, xmpi.MIN, xmpi.MAX]
# every count the GPU tests and scenarios use these inputs at
COUNTS = [1, 17, 1003, 4099, 8209, 65536 + 3, 65536 + 5]


def test_dense_is_deterministic_normal_and_full_mantissa():
    for dtype in FLOATS:
        ut, mb, eb = hi.LAYOUT[dtype]
        a = hi.dense(dtype, 4096, 11, 6)
        assert a.dtype == np.dtype(xmpi.NUMPY_DTYPE[dtype])
        assert a.tobytes() == hi.dense(dtype, 4096, 11, 6).tobytes() and a.tobytes() != hi.dense(dtype, 4096, 12, 6).tobytes()
        b = hi.bits_of(a, dtype).astype(np.uint64)
        exp = ((b >> np.uint64(mb)) & np.uint64((1 << eb) - 1)).astype(np.int64) - ((1 << (eb - 1)) - 1)
        assert exp.min() == -6 and exp.max() == 6 and np.unique(exp).size == 13
        mant = b & np.uint64((1 << mb) - 1)
        for bit in range(mb):  # every mantissa bit is random: set in 35 .. 65 % of the elements
            share = float(np.mean((mant >> np.uint64(bit)) & np.uint64(1)))
            assert 0.35 < share < 0.65, (xmpi.DTYPE_NAME[dtype], bit, share)
        assert 0.4 < float(np.mean(b >> np.uint64(mb + eb))) < 0.6
        one = hi.bits_of(hi.dense(dtype, 4096, 11, 1), dtype).astype(np.uint64)
        e1 = ((one >> np.uint64(mb)) & np.uint64((1 << eb) - 1)).astype(np.int64) - ((1 << (eb - 1)) - 1)
        assert sorted(np.unique(e1)) == [-1, 0, 1]


def test_specials_are_what_their_slots_say():
    for dtype in FLOATS:
        s = hi.from_bits(hi.SPECIALS[dtype], dtype)
        with np.errstate(invalid="ignore"):  # (converting a signalling NaN raises the flag)
            v = oracle.as_float64(s, dtype)
        tiny, big, smallest_normal = {xmpi.F16: (2.0 ** -24, 65504.0, 2.0 ** -14), xmpi.BF16: (2.0 ** -133, float.fromhex("0x1.fep127"), 2.0 ** -126),
                                      xmpi.F32: (2.0 ** -149, float(np.finfo(np.float32).max), 2.0 ** -126),
                                      xmpi.F64: (5e-324, float(np.finfo(np.float64).max), 2.0 ** -1022)}[dtype]
        assert len(s) == 16 and np.unique(hi.SPECIALS[dtype]).size == 16
        assert v[0] == 0 and v[1] == 0 and not np.signbit(v[0]) and np.signbit(v[1])
        assert v[2] == np.inf and v[3] == -np.inf
        assert np.all(np.isnan(v[4:8])) and list(np.nonzero(hi.is_nan(s, dtype))[0]) == list(hi.NAN_SLOTS)
        ut, mb, eb = hi.LAYOUT[dtype]
        quiet = (hi.SPECIALS[dtype] >> ut(mb - 1)) & ut(1)
        assert list(quiet[4:8]) == [1, 1, 0, 0], "two quiet, two signalling"
        assert not np.signbit(v[4]) and np.signbit(v[5])
        assert v[8] == tiny and -smallest_normal < v[9] < 0 and v[9] == -(smallest_normal - tiny)
        assert v[10] == smallest_normal and v[11] == big and v[12] == -big and v[13] == 1 and v[14] == -1
        assert v[15] == (2.0 ** -12 if dtype == xmpi.F16 else 2.0 ** -24)


@pytest.mark.parametrize("size", [2, 3, 8, 16])
def test_planting_conditions(size):
    """at count >= 1003 all 256 ordered pairs meet (as the first two operands, on the last two ranks, on the first and the last);
    each special occurs at every element position of a 16-byte packet; at least one lies in the element tail behind the last full
    packet at every count in use; and a rank's planted input is its dense input everywhere else"""
    for dtype in FLOATS:
        es = xmpi.DTYPE_SIZE[dtype]
        per = 16 // es
        S = hi.SPECIALS[dtype]
        for n in COUNTS:
            ins = [hi.bits_of(hi.special(dtype, n, 77, r, size), dtype) for r in range(size)]
            planted = np.zeros((size, n), dtype=bool)
            idx, who, slot = hi.plan(n, 77, size)
            planted[who, idx] = True
            for r in range(size):
                base = hi.bits_of(hi.dense(dtype, n, 77 + r, 6), dtype)
                assert np.array_equal(ins[r][~planted[r]], base[~planted[r]])
                assert np.all(np.isin(ins[r][planted[r]], S))
            tail = np.arange((n // per) * per, n)
            assert any(np.any(np.isin(ins[r][tail], S) & planted[r][tail]) for r in range(size)), (xmpi.DTYPE_NAME[dtype], n, "no special in the tail")
            if n < 1003:
                continue
            for lo, ra, rb in ((0, 0, 1), (256, size - 2, size - 1), (512, 0, size - 1)):
                pairs = {(int(x), int(y)) for x, y in zip(ins[ra][lo:lo + 256], ins[rb][lo:lo + 256])}
                assert pairs == {(int(x), int(y)) for x in S for y in S}, (xmpi.DTYPE_NAME[dtype], n, lo)
            for k in range(16):
                seen = set()
                for r in range(size):
                    seen |= set((np.nonzero((ins[r] == S[k]) & planted[r])[0] % per).tolist())
                assert seen == set(range(per)), (xmpi.DTYPE_NAME[dtype], n, k, seen)


def test_nan_columns_are_a_minority():
    """what the stepped-schedule checks skip for MIN / MAX -- columns in which some rank's input is NaN -- is about 11 % at count 4099"""
    for size in (2, 3, 8):
        for dtype in FLOATS:
            ins = hi.rank_inputs(dtype, 4099, 5, size, xmpi.MIN)
            share = float(np.mean(np.any([hi.is_nan(x, dtype) for x in ins], axis=0)))
            assert 0.05 < share <= 0.25, (size, xmpi.DTYPE_NAME[dtype], share)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("op", OPS)
def test_oracle_against_a_numpy_restatement(dtype, op):
    """oracle_reduce2 / oracle_reduce_ranks against hard_inputs.np_reduce2 (native numpy arithmetic for f32 / f64, float64 rounded
    once for f16, f32 rounded to nearest even for bf16) under same_floats: all 256 pairs of specials, dense and special data at 2,
    3 and 8 ranks"""
    S = hi.from_bits(hi.SPECIALS[dtype], dtype)
    a, b = np.repeat(S, 16), np.tile(S, 16)
    hi.same_floats(oracle.reduce2(a, b, dtype, op), hi.np_reduce2(a, b, dtype, op), dtype, op, "all pairs of specials")
    for size in (2, 3, 8):
        for kind in ("dense", "special"):
            ins = hi.rank_inputs(dtype, 4099, 300 + size, size, op, kind)
            hi.same_floats(oracle.reduce_ranks(ins, dtype, op), hi.np_reduce_ranks(ins, dtype, op), dtype, op, f"{kind} data, {size} ranks")
        for spread in (hi.SPREAD_SUM, hi.SPREAD_PROD):
            ins = [hi.dense(dtype, 4099, 900 + r, spread) for r in range(size)]
            got, want = oracle.reduce_ranks(ins, dtype, op), hi.np_reduce_ranks(ins, dtype, op)
            assert got.tobytes() == want.tobytes(), "dense data: bit for bit, no NaN rule needed"


def _share(a: np.ndarray, b: np.ndarray, dtype: int) -> float:
    return float(np.mean(hi.bits_of(a, dtype) != hi.bits_of(b, dtype)))


def fold_order_shares(dtype, op, size, n=4096):
    ins = hi.rank_inputs(dtype, n, 1234, size, op, "dense")
    want = oracle.reduce_ranks(ins, dtype, op)
    return (_share(want, oracle.reduce_ranks(ins[::-1], dtype, op), dtype), _share(want, oracle.reduce_ranks(ins[1:] + ins[:1], dtype, op), dtype))


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("op", [xmpi.SUM, xmpi.PROD])
@pytest.mark.parametrize("size", [3, 8])
def test_the_fold_order_shows_on_dense_data(dtype, op, size):
    """the rank-order fold of dense inputs differs from the reversed and from the rotated fold in at least 10 % of 4096 elements.
    Measured (reversed / rotated, per cent of elements whose bits differ):
                 SUM, 3 ranks   SUM, 8 ranks   PROD, 3 ranks   PROD, 8 ranks
        f16      25.0 / 25.0    60.0 / 47.2    33.9 / 33.9     63.2 / 61.6
        f32      25.3 / 25.3    60.3 / 47.0    34.7 / 34.7     64.5 / 62.8
        f64      24.9 / 24.9    59.8 / 47.6    35.3 / 35.3     63.6 / 64.5
        bf16     23.1 / 23.1    56.7 / 43.1    33.6 / 33.6     62.8 / 64.3
    (at 3 ranks the two are one figure: (c + b) + a and (b + c) + a differ only by a commuted first addition)"""
    rev, rot = fold_order_shares(dtype, op, size)
    print(f"{xmpi.DTYPE_NAME[dtype]} op={op} size={size}: reversed {100 * rev:.1f} % rotated {100 * rot:.1f} %")
    assert rev >= 0.10 and rot >= 0.10, (rev, rot)


@pytest.mark.parametrize("dtype", [xmpi.F32, xmpi.F64])
@pytest.mark.parametrize("size", [3, 8, 16])
def test_pat_signed_sums_the_same_in_every_order(dtype, size):
    """the reason this module exists: on PAT_SIGNED (8-bit multiples of 2^-12 below 4) an f32 / f64 SUM of up to 16 ranks is exact
    in every association -- reversed, rotated and pairwise folds change 0 of 4096 elements -- so no test on it can tell rank order
    from any other"""
    ins = [oracle.fill(4096, dtype, xmpi.PAT_SIGNED, 100 + r) for r in range(size)]
    want = oracle.reduce_ranks(ins, dtype, xmpi.SUM)
    pairwise = list(ins)
    while len(pairwise) > 1:
        pairwise = [oracle.reduce2(pairwise[i], pairwise[i + 1], dtype, xmpi.SUM) if i + 1 < len(pairwise) else pairwise[i]
                    for i in range(0, len(pairwise), 2)]
    for other in (oracle.reduce_ranks(ins[::-1], dtype, xmpi.SUM), oracle.reduce_ranks(ins[1:] + ins[:1], dtype, xmpi.SUM), pairwise[0]):
        assert _share(want, other, dtype) == 0.0


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("op", [xmpi.MIN, xmpi.MAX])
def test_min_and_max_depend_on_operand_order_here(dtype, op):
    """(b < a) ? b : a keeps `a` when either is NaN and on +0 against -0: reduce2(a, b) != reduce2(b, a) on this data, so a
    commuted select -- or a hardware minimum that returns the number -- is visible"""
    a, b = hi.special(dtype, 1003, 9, 0, 2), hi.special(dtype, 1003, 9, 1, 2)
    ab, ba = oracle.reduce2(a, b, dtype, op), oracle.reduce2(b, a, dtype, op)
    differ = hi.bits_of(ab, dtype) != hi.bits_of(ba, dtype)
    assert np.sum(differ) >= 100, int(np.sum(differ))
    # ... among them a NaN first operand kept against a number, and the sign of the first zero kept
    S = hi.from_bits(hi.SPECIALS[dtype], dtype)
    assert oracle.reduce2(S[4:5], S[13:14], dtype, op).tobytes() == S[4:5].tobytes()
    assert oracle.reduce2(S[13:14], S[6:7], dtype, op).tobytes() == S[13:14].tobytes()
    assert oracle.reduce2(S[0:1], S[1:2], dtype, op).tobytes() == S[0:1].tobytes()
    assert oracle.reduce2(S[1:2], S[0:1], dtype, op).tobytes() == S[1:2].tobytes()


def test_same_floats_is_as_strict_as_it_says():
    for dtype in FLOATS:
        S = hi.from_bits(hi.SPECIALS[dtype], dtype)
        for op in (xmpi.MIN, xmpi.MAX):  # selection: a NaN's payload and a zero's sign count
            hi.same_floats(S, S.copy(), dtype, op)
            for i, j in ((4, 6), (0, 1), (4, 5)):
                other = S.copy()
                other[i] = S[j]
                with pytest.raises(AssertionError):
                    hi.same_floats(other, S, dtype, op)
        for op in (xmpi.SUM, xmpi.PROD):  # arithmetic: any NaN for any NaN, nothing else for anything
            other = S.copy()
            other[4], other[7] = S[7], S[5]
            hi.same_floats(other, S, dtype, op)
            for i, j in ((0, 1), (4, 2), (2, 4), (8, 0), (11, 2)):
                other = S.copy()
                other[i] = S[j]
                with pytest.raises(AssertionError):
                    hi.same_floats(other, S, dtype, op)
