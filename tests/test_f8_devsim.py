"""XMPI_F8E4M3 / XMPI_F8E5M2 on virtual devices (tests/devsim: the library's host and kernel sources compiled for the CPU over a HIP
runtime with N virtual devices -- see tests/test_devsim.py), one process per device, then the other layouts and the clean errors.
Scenarios: tests/f8_scenarios.py; every result is held to the numpy restatement of the two types (tests/f8_ref.py), the same set of
NaN positions and every other element bit for bit.  Here the kernels' plain C++ conversions run -- the definition, written once in
kdev.h; the packed gfx950 instructions are held to it by tests/test_gpu_f8*.py.  No GPU involved."""
import os

import pytest

from mpi_amd import xmpi
from tests.f8_harness import run_ranks, run_threads

SIZES = [2, 3, 8]


@pytest.fixture(scope="module", autouse=True)
def devsim_lib():
    from tests.devsim import build
    path = build.build_lib()
    old = os.environ.get("XMPI_DEVSIM_LIB")
    os.environ["XMPI_DEVSIM_LIB"] = path  # (the harness hands the environment on to the rank processes)
    yield path
    if old is None:
        del os.environ["XMPI_DEVSIM_LIB"]
    else:
        os.environ["XMPI_DEVSIM_LIB"] = old


# ---- one process per virtual device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_every_pair_of_encodings_under_every_operator(size):
    """65536 elements: rank 0 holds byte i >> 8, rank 1 byte i & 255, the further ranks a fixed small set; SUM, PROD, MIN, MAX and
    SUM_WIDE, both types, allreduce by AUTO and ZCOPY and xmpi_reduce_local; with 3 ranks or more SUM and SUM_WIDE differ"""
    outs = run_ranks("pairs", size, timeout=240)
    assert "f8 pairs" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_every_algorithm_name_at_every_count(size):
    """AUTO | ZCOPY | ZPUSH | LL | DIRECT x {1, 7, 8, 9, 15, 16, 17, 1000, 4099, 32768, 32769, 65536 + 5} elements x both types x
    {allreduce out of and in place, reduce at the first and the last rank, reduce-scatter}: the same bits by every name"""
    run_ranks("names", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_every_form_forced_and_confirmed_by_the_launch_counters(size):
    """one kernel (unroll 1 and 2), meet / body / done, its system-scope body, LL launched (never by the agent), ZPUSH, DIRECT; buffers
    one element behind a 16-byte boundary; AUTO with ll_bytes = 0"""
    outs = run_ranks("forms", size, timeout=240)
    assert "each with its form confirmed by the counters" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_host_slices_unregistered_memory_streams_iallreduce_and_repeat(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_captured_graph_replayed_with_new_inputs(size):
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_table_row_naming_a_stepped_schedule_runs_the_fold(size):
    """`tuned` = 1 and a hand-written row naming RING / RHD_PUSH / TREE: XMPI_U8 takes the stepped kernel, the 8-bit floats the fold"""
    run_ranks("table", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_stepped_name_and_a_bitwise_operator_are_refused_on_every_rank(size):
    """RING, RHD, TREE and their PUSH forms named by the caller, every operator: XMPI_ERR_UNSUPPORTED; BAND / BOR / BXOR: XMPI_ERR_ARG;
    nothing launched, the communicator usable"""
    run_ranks("refused", size, timeout=240)


@pytest.mark.parametrize("dtypes", [(xmpi.F8E4M3, xmpi.F8E5M2), (xmpi.F8E4M3, xmpi.U8), (xmpi.U8, xmpi.F8E5M2)])
@pytest.mark.parametrize("size", SIZES)
def test_the_two_types_and_u8_are_different_calls(size, dtypes):
    """above the LL limit the kernels compare their call signatures: XMPI_ERR_ARG on every rank, nothing moved"""
    outs = run_ranks("mismatch", size, {"dtypes": list(dtypes)}, timeout=120)
    assert all("f8 mismatch: ok" in o for o in outs), outs


@pytest.mark.parametrize("size", SIZES)
def test_everything_without_an_operator_moves_them_as_bytes(size):
    """bcast, allgather, all-to-all, alltoallv, Send / Receive / probe of all 256 encodings by every name those accept; a Receive naming
    the other 8-bit type is refused"""
    outs = run_ranks("moves", size, timeout=240)
    assert "f8 moves" in outs[0]


# ---- the other layouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 4])
def test_rank_threads_in_one_process(size):
    run_threads("layout", size, {"expect_host_fold": 1}, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_ranks_that_meet_on_the_host(size):
    """XMPI_DSYNC=0: zcopy.cpp's rendezvous and its one fold launch"""
    run_ranks("layout", size, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", SIZES)
def test_staged_tables(size):
    """XMPI_DSYNC=0 XMPI_ZERO_COPY=0: the one-hop tables of plan.cpp -- allreduce, reduce-scatter, and a reduce short enough that
    staged AUTO would pick the TREE table (DIRECT runs instead)"""
    run_ranks("layout", size, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})


# ---- the local kernels, on the CPU build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [xmpi.F8E4M3, xmpi.F8E5M2])
def test_local_kernels(dtype):
    """every pair of encodings with 2, 3, 8 and 16 sources; midpoints +- the smallest subnormal; xmpi_reduce_local_n / _multi / _batch
    at every count and both alignments; every cache policy"""
    outs = run_ranks("kernels", 1, {"dtype": dtype}, timeout=240)
    assert "launches checked" in outs[0]
