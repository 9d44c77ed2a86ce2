"""XMPI_BAND / XMPI_BOR / XMPI_BXOR on virtual devices (tests/devsim: the library's host and kernel sources compiled for the CPU over a
HIP runtime with N virtual devices -- see tests/test_devsim.py), one process per device, then the other layouts, the clean errors and
the local kernels.  Scenarios: tests/bitop_scenarios.py; every result is compared bit for bit with the numpy restatement of the
operator (tests/bitop_ref.py).  No GPU involved."""
import os

import pytest

from mpi_amd import xmpi
from tests import bitop_ref as br
from tests.bitop_harness import run_ranks, run_threads

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
@pytest.mark.parametrize("dtype", br.DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_algorithm_name_at_every_count(size, dtype):
    """AUTO | ZCOPY | ZPUSH | LL | DIRECT | RING | RHD | RING_PUSH | RHD_PUSH (allreduce, out of and in place), TREE | TREE_PUSH | DIRECT |
    ZCOPY | AUTO (reduce, first and last root), ZCOPY | ZPUSH | LL | DIRECT | AUTO (reduce-scatter) x three operators x
    {1, 7, 8, 9, 1000, 4099, 65536 + 5} elements: the same bits by every name"""
    outs = run_ranks("names", size, {"dtype": dtype}, timeout=240)
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("dtype", br.DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_form_forced_and_confirmed_by_the_launch_counters(size, dtype):
    """one kernel (unroll 1 and 2), meet / body / done, its system-scope body, LL launched and by the agent, ZPUSH, DIRECT, the stepped
    kernels in pull and push form; buffers one element behind a 16-byte boundary"""
    outs = run_ranks("forms", size, {"dtype": dtype}, timeout=240)
    assert "each with its form confirmed by the counters" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_host_slices_unregistered_memory_streams_and_nonblocking(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_captured_graph_replayed_with_new_inputs(size):
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_float_type_is_refused_at_every_entry(size):
    """XMPI_ERR_ARG on every rank, nothing launched, the receive buffer untouched, a following XMPI_SUM succeeds"""
    outs = run_ranks("float_refused", size, timeout=240)
    assert "calls refused" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_operators_8_and_minus_1_are_refused(size):
    run_ranks("bad_op", size, timeout=120)


@pytest.mark.parametrize("dtype", [xmpi.I32, xmpi.I64])
@pytest.mark.parametrize("size", SIZES)
def test_different_bitwise_operators_are_different_calls(size, dtype):
    """above the LL limit the kernels compare their call signatures: XMPI_ERR_ARG on every rank, nothing moved"""
    outs = run_ranks("mismatch", size, {"dtype": dtype}, timeout=120)
    assert all("bitop mismatch: ok" in o for o in outs), outs


# ---- the other layouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 4])
def test_rank_threads_in_one_process(size):
    run_threads("layout", size, {"expect_host_fold": 1}, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_ranks_that_meet_on_the_host(size):
    """XMPI_DSYNC=0: zcopy.cpp's rendezvous and its one fold launch; the stepped names as host-driven step tables"""
    run_ranks("layout", size, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", SIZES)
def test_staged_tables(size):
    """XMPI_DSYNC=0 XMPI_ZERO_COPY=0: the step tables of plan.cpp, whose reductions are reduce2 and its batch"""
    run_ranks("layout", size, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})


# ---- the local kernels, on the CPU build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", br.DTYPES)
def test_local_kernels(dtype):
    """xmpi_reduce_local, _local_n (1..9 and 16 sources), _local_multi (1 / 2 / 8 destinations), _local_batch: every count, both
    alignments, every cache policy"""
    outs = run_ranks("local", 1, {"dtype": dtype}, timeout=240)
    assert "launches checked" in outs[0]
