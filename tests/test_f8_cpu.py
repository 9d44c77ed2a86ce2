"""XMPI_F8E4M3 / XMPI_F8E5M2 without a GPU: the numpy restatement (tests/f8_ref.py) against the formats' own structure and against
torch's CPU casts, and the two types as the built library, the header, xmpi.py, the Go shim and INTEGRATION.md name them."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpi_amd import xmpi
from tests import f8_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = {xmpi.F8E4M3: "float8_e4m3fn", xmpi.F8E5M2: "float8_e5m2"}


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def test_the_formats_as_the_header_states_them():
    e4, e5 = fr.decode(xmpi.F8E4M3), fr.decode(xmpi.F8E5M2)
    assert e4[0x7E] == 448.0 and e4[0xFE] == -448.0 and e4[0x01] == 2.0 ** -9 and e4[0x38] == 1.0
    assert np.isnan(e4[0x7F]) and np.isnan(e4[0xFF]) and np.count_nonzero(np.isnan(e4)) == 2 and not np.any(np.isinf(e4))
    assert e5[0x7B] == 57344.0 and e5[0x01] == 2.0 ** -16 and e5[0x3C] == 1.0 and e5[0x7C] == np.inf and e5[0xFC] == -np.inf
    assert np.all(np.isnan(e5[[0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]])) and np.count_nonzero(np.isnan(e5)) == 6
    assert np.signbit(e4[0x80]) and e4[0x80] == 0.0 and np.signbit(e5[0x80]) and e5[0x80] == 0.0
    for d in fr.F8_DTYPES:  # increasing with the byte over the non-negative finite values, E5M2 = the top byte of a float16
        assert np.all(np.diff(fr.finite_sorted(d)) > 0)
    assert np.array_equal(e5, (np.arange(256, dtype=np.uint16) << 8).view(np.float16).astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
def test_decode_then_narrow_is_the_identity(dtype):
    b = np.arange(256, dtype=np.uint8)
    keep = ~fr.is_nan(b, dtype)
    assert np.array_equal(fr.narrow(fr.decode(dtype), dtype)[keep], b[keep])
    assert np.all(fr.is_nan(fr.narrow(fr.decode(dtype), dtype)[~keep], dtype))  # a NaN gives a NaN, whichever


def _midpoints(dtype):
    v = fr.finite_sorted(dtype)
    lo, hi = v[:-1], v[1:]
    mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (lo.astype(np.float64) + hi.astype(np.float64)) / 2)  # exact: one more bit
    return np.arange(len(lo), dtype=np.uint8), mid  # (the lower neighbour's byte; the upper one's is that plus one)


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
def test_every_midpoint_goes_to_the_even_neighbour_and_its_neighbours_to_the_nearer(dtype):
    lob, mid = _midpoints(dtype)
    even = np.where(lob & 1, lob + 1, lob).astype(np.uint8)
    for sign, sb in ((1.0, 0x00), (-1.0, 0x80)):
        m = (sign * mid).astype(np.float32)
        assert np.array_equal(fr.narrow(m, dtype), even | sb)
        towards_zero = np.nextafter(m, np.float32(0)).astype(np.float32)
        away = np.nextafter(m, np.float32(sign * np.inf)).astype(np.float32)
        assert np.array_equal(fr.narrow(towards_zero, dtype), lob | sb)
        assert np.array_equal(fr.narrow(away, dtype), (lob + 1).astype(np.uint8) | sb)
    # below half the smallest subnormal: a zero of the same sign; exactly half: the tie goes to the (even) zero
    tiny = np.float32(fr.min_subnormal(dtype) / 2)
    assert list(fr.narrow(np.array([tiny, -tiny, np.nextafter(tiny, np.float32(1)), np.float32(1e-40), np.float32(-1e-40)], dtype=np.float32), dtype)) == \
        [0x00, 0x80, 0x01, 0x00, 0x80]


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
def test_saturation_infinities_and_nan(dtype):
    mx = fr.max_finite(dtype)
    maxb = fr.LAYOUT[dtype][2]
    big = np.array([mx, np.nextafter(np.float32(mx), np.float32(np.inf)), mx * 1.5, 3e38, -mx * 2, -3e38], dtype=np.float32)
    assert list(fr.narrow(big, dtype)) == [maxb, maxb, maxb, maxb, 0x80 | maxb, 0x80 | maxb]
    inf = fr.narrow(np.array([np.inf, -np.inf], dtype=np.float32), dtype)
    assert list(inf) == ([0x7C, 0xFC] if dtype == xmpi.F8E5M2 else [maxb, 0x80 | maxb])
    assert np.all(fr.is_nan(fr.narrow(np.array([np.nan, -np.nan], dtype=np.float32), dtype), dtype))
    # a sum of finite inputs never turns into inf or NaN: max + max, narrowed after each of 16 contributions and once
    xs = [np.array([maxb], dtype=np.uint8)] * 16
    assert fr.reduce_ranks(xs, dtype, xmpi.SUM)[0] == maxb and fr.reduce_ranks(xs, dtype, xmpi.SUM_WIDE)[0] == maxb


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
def test_narrow_is_torch_s_cast_up_to_the_largest_finite_value_and_saturates_beyond(dtype):
    import torch
    tdt = getattr(torch, TORCH[dtype])
    mx = fr.max_finite(dtype)
    rng = np.random.default_rng(88)
    _, mid = _midpoints(dtype)
    near = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)), fr.finite_sorted(dtype)]).astype(np.float32)
    bits = rng.integers(0, 1 << 32, size=400000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    spread = (rng.standard_normal(200000) * rng.choice([1e-5, 1e-3, 0.1, 1.0, 30.0, mx / 3], size=200000)).astype(np.float32)
    x = np.concatenate([near, -near, bits, spread, np.array([0.0, -0.0, mx, -mx], dtype=np.float32)])
    x = x[np.isfinite(x) & (np.abs(x) <= mx)]
    assert x.size > 250000
    want = torch.from_numpy(x.copy()).to(tdt).view(torch.uint8).numpy()
    fr.same(fr.narrow(x, dtype), want, dtype, f"narrow against torch.{TORCH[dtype]}")
    # the decode table is torch's too
    back = torch.arange(256, dtype=torch.uint8).view(tdt).to(torch.float32).numpy()
    assert np.array_equal(back, fr.decode(dtype), equal_nan=True)
    # past the largest finite value torch leaves the format's finite range, this definition saturates
    first = np.array([465.0 if dtype == xmpi.F8E4M3 else 61440.0], dtype=np.float32)
    t = torch.from_numpy(first).to(tdt).to(torch.float32).numpy()[0]
    assert (np.isnan(t) if dtype == xmpi.F8E4M3 else np.isinf(t)), t
    assert fr.narrow(first, dtype)[0] == fr.LAYOUT[dtype][2]


def test_the_operators_by_hand():
    e4 = lambda *bs: [np.array([b], dtype=np.uint8) for b in bs]
    one, half_ulp = 0x38, 0x18  # 1 and 2^-4: half an ulp of 1 with 3 mantissa bits (exponent field 3: 2^(3 - 7))
    assert fr.decode(xmpi.F8E4M3)[half_ulp] == 0.0625
    # 1 + 2^-4 + 2^-4: narrowed after each contribution the tie goes to even twice and stays 1; accumulated wide it is 1.125
    assert fr.reduce_ranks(e4(one, half_ulp, half_ulp), xmpi.F8E4M3, xmpi.SUM)[0] == one
    assert fr.reduce_ranks(e4(one, half_ulp, half_ulp), xmpi.F8E4M3, xmpi.SUM_WIDE)[0] == one + 1
    # 448 + 448 - 448: saturates at 448 after the first step, then 0; wide: 448
    assert fr.reduce_ranks(e4(0x7E, 0x7E, 0xFE), xmpi.F8E4M3, xmpi.SUM)[0] == 0x00
    assert fr.reduce_ranks(e4(0x7E, 0x7E, 0xFE), xmpi.F8E4M3, xmpi.SUM_WIDE)[0] == 0x7E
    # zeros: -0 + -0 = -0, -0 + +0 = +0, x - x = +0; min / max return the operand's own byte, NaN and zeros as the expressions make them
    assert fr.reduce_ranks(e4(0x80, 0x80), xmpi.F8E4M3, xmpi.SUM)[0] == 0x80
    assert fr.reduce_ranks(e4(0x80, 0x00), xmpi.F8E4M3, xmpi.SUM)[0] == 0x00
    assert fr.reduce_ranks(e4(0x45, 0xC5), xmpi.F8E4M3, xmpi.SUM)[0] == 0x00
    assert fr.reduce_ranks(e4(0x00, 0x80), xmpi.F8E4M3, xmpi.MIN)[0] == 0x00 and fr.reduce_ranks(e4(0x80, 0x00), xmpi.F8E4M3, xmpi.MAX)[0] == 0x80
    assert fr.reduce_ranks(e4(0x7F, 0x38), xmpi.F8E4M3, xmpi.MIN)[0] == 0x7F and fr.reduce_ranks(e4(0x38, 0xFF), xmpi.F8E4M3, xmpi.MAX)[0] == 0x38
    # E5M2: inf - inf is NaN, inf + finite stays inf, a product of the two largest saturates
    e5 = e4
    assert fr.is_nan(fr.reduce_ranks(e5(0x7C, 0xFC), xmpi.F8E5M2, xmpi.SUM), xmpi.F8E5M2)[0]
    assert fr.reduce_ranks(e5(0x7C, 0xFB), xmpi.F8E5M2, xmpi.SUM)[0] == 0x7C
    assert fr.reduce_ranks(e5(0x7B, 0x7B), xmpi.F8E5M2, xmpi.PROD)[0] == 0x7B
    assert fr.reduce_ranks(e5(0x01, 0x01), xmpi.F8E5M2, xmpi.PROD)[0] == 0x00  # 2^-32: far below half the smallest subnormal
    x = np.arange(256, dtype=np.uint8)
    for d in fr.F8_DTYPES:
        for op in (xmpi.SUM, xmpi.PROD, xmpi.MIN, xmpi.MAX, xmpi.SUM_WIDE):
            assert fr.reduce_ranks([x], d, op).tobytes() == x.tobytes()  # one contribution: a copy, NaN bits included


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
def test_with_two_contributions_wide_is_sum_and_with_three_it_is_not(dtype):
    a, b = np.repeat(np.arange(256, dtype=np.uint8), 256), np.tile(np.arange(256, dtype=np.uint8), 256)
    fr.same(fr.reduce_ranks([a, b], dtype, xmpi.SUM_WIDE), fr.reduce_ranks([a, b], dtype, xmpi.SUM), dtype, "two contributions")
    c = np.full(65536, 0x01, dtype=np.uint8)
    d = fr.differing(fr.reduce_ranks([a, b, c], dtype, xmpi.SUM_WIDE), fr.reduce_ranks([a, b, c], dtype, xmpi.SUM), dtype)
    print(f"{xmpi.DTYPE_NAME[dtype]}: SUM and SUM_WIDE of every pair plus the smallest subnormal differ in {d} of 65536 elements")
    assert d > 0


# ---- the library, the header, the bindings, the documents ------------------------------------------------------------------------------
def test_the_element_size_through_the_built_library():
    lib = ctypes.CDLL(xmpi.LIB_PATH)
    lib.xmpi_dtype_size.restype = ctypes.c_size_t
    lib.xmpi_dtype_size.argtypes = [ctypes.c_int]
    assert [lib.xmpi_dtype_size(d) for d in range(11)] == [1, 4, 8, 2, 4, 8, 2, 1, 1, 0, 0]
    assert lib.xmpi_dtype_size(-1) == 0


def test_the_constants_agree():
    assert (xmpi.U8, xmpi.I32, xmpi.I64, xmpi.F16, xmpi.F32, xmpi.F64, xmpi.BF16, xmpi.F8E4M3, xmpi.F8E5M2) == tuple(range(9))
    assert xmpi.DTYPE_SIZE[xmpi.F8E4M3] == xmpi.DTYPE_SIZE[xmpi.F8E5M2] == 1
    assert xmpi.NUMPY_DTYPE[xmpi.F8E4M3] is np.uint8 and xmpi.NUMPY_DTYPE[xmpi.F8E5M2] is np.uint8
    text = open(os.path.join(ROOT, "include", "xmpi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(XMPI_[A-Z0-9_]+)\s*=\s*(\d+)\s*,", hdr[hdr.index("XMPI_U8 = 0"):hdr.index("} xmpi_dtype;")]))
    assert enum == {"XMPI_U8": 0, "XMPI_I32": 1, "XMPI_I64": 2, "XMPI_F16": 3, "XMPI_F32": 4, "XMPI_F64": 5, "XMPI_BF16": 6, "XMPI_F8E4M3": 7,
                    "XMPI_F8E5M2": 8, "XMPI_DTYPE_COUNT": 9}
    for word in ("OCP", "448", "57344", "SATURATES", "ties to even"):
        assert word in text[:text.index("} xmpi_dtype;")], word
    go = open(os.path.join(ROOT, "go", "xgmi", "xgmi.go")).read()
    block = re.sub(r"//[^\n]*", "", go[go.index("U8 DType = iota"):])
    names = [ln.split()[0] for ln in block[:block.index(")")].splitlines() if ln.strip()]
    assert names == ["U8", "I32", "I64", "F16", "F32", "F64", "BF16", "F8E4M3", "F8E5M2"], names
    assert "F8E4M3" in open(os.path.join(ROOT, "go", "mpi_collectives", "collectives.go")).read()
    kdev = open(os.path.join(ROOT, "mpi_amd", "csrc", "kdev.h")).read()
    assert "DT_F8E4M3 = 7, DT_F8E5M2 = 8" in kdev


def test_the_documents_list_the_types():
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md", "CHANGELOG.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "XMPI_F8E4M3" in text and "XMPI_F8E5M2" in text, name
