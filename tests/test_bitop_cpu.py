"""XMPI_BAND / XMPI_BOR / XMPI_BXOR without a GPU and without the virtual devices.

First the conditions that make the other bitwise suites meaningful, asserted on the reference alone (tests/bitop_ref.py) -- they are
conditions on the INPUTS, not measurements of the library: the three results differ from one another and from SUM / MIN / MAX of the
same inputs in at least half of the elements (a kernel that ran another operator cannot pass), XOR with any one rank's contribution
applied twice differs from the correct XOR in at least half of the elements (a schedule that folds a chunk twice cannot pass), and
the share of set bits in every result lies within [1 / 4, 3 / 4] (no result is nearly a constant).  Then the constants of xmpi.py,
the header and the Go shim, and mpi::Network on three loopback ranks (tests/tcp_bitop_check.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

from mpi_amd import xmpi
from tests import bitop_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4099
SIZES = [2, 3, 8]


def _others(ins):
    """numpy's wrapping SUM, and MIN / MAX, of the same inputs"""
    stack = np.stack(ins)
    with np.errstate(over="ignore"):
        return {"SUM": np.add.reduce(stack, axis=0, dtype=stack.dtype), "MIN": stack.min(axis=0), "MAX": stack.max(axis=0)}


@pytest.mark.parametrize("dtype", br.DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_the_inputs_tell_the_operators_apart(size, dtype):
    results = {}
    for op in br.OPS:
        ins = br.rank_inputs(dtype, N, 4000, size, op)
        want = br.reduce_ranks(ins, op)
        assert want.dtype == xmpi.NUMPY_DTYPE[dtype] and want.shape == (N,)
        # every rank's array is distinct, full width, about half of the elements negative as a signed type
        assert len({x.tobytes() for x in ins}) == size
        top = np.stack(ins).view(np.uint8).reshape(size, N, -1)[:, :, -1] >> 7
        assert 0.4 < top.mean() < 0.6, f"sign bits set: {top.mean():.3f}"
        share = br.set_bit_share(want)
        assert 0.25 <= share <= 0.75, f"{br.OP_NAME[op]}, {size} ranks: {share:.3f} of the result's bits are set"
        assert abs(br.set_bit_share(np.stack(ins)) - br.bit_density(op, size)) < 0.08
        # the other two bitwise operators and SUM / MIN / MAX on the SAME inputs give something else nearly everywhere
        for other in br.OPS:
            if other != op:
                d = br.differing(want, br.reduce_ranks(ins, other))
                assert d >= N // 2, f"{br.OP_NAME[op]} against {br.OP_NAME[other]} on {br.OP_NAME[op]}'s inputs: {d} of {N} differ"
        for name, x in _others(ins).items():
            d = br.differing(want, x)
            assert d >= N // 2, f"{br.OP_NAME[op]} against {name}: {d} of {N} differ"
        # one contribution is not the answer, nor is the fold of all but one
        for r in range(size):
            assert br.differing(want, ins[r]) >= N // 2
            if size > 2:
                assert br.differing(want, br.reduce_ranks(ins[:r] + ins[r + 1:], op)) >= (N // 2 if op == xmpi.BXOR else N // 8)
        results[op] = want
    # the three results of a job (each on its own inputs) differ from one another
    for a in br.OPS:
        for b in br.OPS:
            if a < b:
                assert br.differing(results[a], results[b]) >= N // 2


@pytest.mark.parametrize("dtype", br.DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_xor_shows_a_contribution_applied_twice(size, dtype):
    ins = br.rank_inputs(dtype, N, 4000, size, xmpi.BXOR)
    want = br.reduce_ranks(ins, xmpi.BXOR)
    for r in range(size):
        twice = br.reduce_ranks(ins + [ins[r]], xmpi.BXOR)
        assert br.differing(want, twice) >= N // 2, f"rank {r}'s contribution applied twice goes unnoticed"
        assert twice.tobytes() == br.reduce_ranks(ins[:r] + ins[r + 1:], xmpi.BXOR).tobytes()  # x ^ x = 0: it cancels


def test_the_reference_on_hand_computed_words():
    a, b, c = (np.array([x], dtype=np.int32) for x in (0x0FF0_F0F0, -0x0F0F_0F10, 0x3333_3333))  # (b = 0xF0F0F0F0)
    assert br.reduce_ranks([a, b, c], xmpi.BAND).view(np.uint32)[0] == 0x0030_3030
    assert br.reduce_ranks([a, b, c], xmpi.BOR).view(np.uint32)[0] == 0xFFF3_F3F3
    assert br.reduce_ranks([a, b, c], xmpi.BXOR).view(np.uint32)[0] == 0xCC33_3333
    x = np.array([-1, 0, -2 ** 63], dtype=np.int64)
    assert br.reduce_ranks([x], xmpi.BXOR).tobytes() == x.tobytes()  # one contribution: a copy
    assert br.reduce_ranks([x, x], xmpi.BXOR).tobytes() == np.zeros(3, dtype=np.int64).tobytes()
    assert br.reduce_ranks([x, x], xmpi.BAND).tobytes() == x.tobytes() == br.reduce_ranks([x, x], xmpi.BOR).tobytes()
    u = [np.array([v], dtype=np.uint8) for v in (0xF0, 0x3C)]
    assert [int(br.reduce_ranks(u, op)[0]) for op in br.OPS] == [0x30, 0xFC, 0xCC]


def test_small_counts_and_both_seeds_differ():
    for dtype in br.DTYPES:
        for count in (1, 7):
            ins = br.rank_inputs(dtype, count, 4000, 3, xmpi.BOR)
            assert len(ins) == 3 and all(x.shape == (count,) and x.dtype == xmpi.NUMPY_DTYPE[dtype] for x in ins)
        a, b = br.rank_inputs(dtype, N, 4000, 3, xmpi.BXOR), br.rank_inputs(dtype, N, 4100, 3, xmpi.BXOR)
        assert a[0].tobytes() != b[0].tobytes()
        assert a[0].tobytes() == br.rank_inputs(dtype, N, 4000, 3, xmpi.BXOR)[0].tobytes()  # (every rank process computes the same job)


def test_the_constants_agree():
    """xmpi.py, include/xmpi.h and the Go shim name the same eight operators in the same order"""
    assert (xmpi.SUM, xmpi.PROD, xmpi.MIN, xmpi.MAX, xmpi.SUM_WIDE, xmpi.BAND, xmpi.BOR, xmpi.BXOR) == tuple(range(8))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xmpi.h")).read(), flags=re.S)
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(XMPI_[A-Z_]+)\s*=\s*(\d+)\s*,", hdr[hdr.index("XMPI_SUM = 0"):hdr.index("} xmpi_op;")]))
    assert enum == {"XMPI_SUM": 0, "XMPI_PROD": 1, "XMPI_MIN": 2, "XMPI_MAX": 3, "XMPI_SUM_WIDE": 4, "XMPI_BAND": 5, "XMPI_BOR": 6, "XMPI_BXOR": 7,
                    "XMPI_OP_COUNT": 8}
    text = open(os.path.join(ROOT, "include", "xmpi.h")).read()
    for word in ("XMPI_BAND / XMPI_BOR / XMPI_BXOR", "XMPI_U8", "every schedule", "integer type"):
        assert word in text[text.index("XMPI_SUM .. XMPI_MAX"):text.index("} xmpi_op;")], word
    for path, first in ((os.path.join(ROOT, "go", "xgmi", "xgmi.go"), "Sum Op = iota"), (os.path.join(ROOT, "go", "mpi_collectives", "collectives.go"), "OpSum = iota")):
        go = open(path).read()
        block = re.sub(r"//[^\n]*", "", go[go.index(first):])
        block = block[:block.index(")")]
        names = [ln.split()[0] for ln in block.splitlines() if ln.strip()]
        assert [n.replace("Op", "", 1) if n.startswith("Op") else n for n in names] == ["Sum", "Prod", "Min", "Max", "SumWide", "BAnd", "BOr", "BXor"], names
    kdev = open(os.path.join(ROOT, "mpi_amd", "csrc", "kdev.h")).read()
    assert "OP_BAND = 5, OP_BOR = 6, OP_BXOR = 7" in kdev


def test_network_backend(tmp_path):
    """mpi::Network, 3 loopback ranks: allreduce and reduce of int32 / int64 by each operator against a host loop; float64 and
    float32 refused before anything is exchanged; operator 8 refused; XMPI_SUM afterwards"""
    exe = str(tmp_path / "tcp_bitop_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "mpi_amd", "host"), os.path.join(ROOT, "tests", "tcp_bitop_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "mpi_amd"), "-lxmpi_host", "-lxmpi", "-Wl,-rpath," + os.path.join(ROOT, "mpi_amd"),
                           "-lpthread"])
    out = subprocess.run([exe, "8181"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
