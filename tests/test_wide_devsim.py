"""XMPI_SUM_WIDE on virtual devices (tests/devsim: the library's host and kernel sources compiled for the CPU over a HIP runtime with N
virtual devices -- see tests/test_devsim.py), one process per device, then the other layouts and the clean errors.  Scenarios:
tests/wide_scenarios.py; every result is held to the numpy restatement of the operator (tests/wide_ref.py), the same set of NaN
positions and every other element bit for bit.  No GPU involved."""
import os

import pytest

from mpi_amd import xmpi
from tests.wide_harness import run_ranks, run_threads

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
def test_every_algorithm_name_at_every_count(size):
    """AUTO | ZCOPY | ZPUSH | LL | DIRECT x {1, 7, 8, 9, 1000, 4099, 65536 + 5} elements x f16 / bf16 x {allreduce out of and in
    place, reduce at the first and the last rank, reduce-scatter}: the same bits by every name; with 3 ranks or more, not XMPI_SUM's"""
    run_ranks("names", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_every_form_forced_and_confirmed_by_the_launch_counters(size):
    """one kernel (unroll 1 and 2), meet / body / done, its system-scope body, LL launched and by the agent, ZPUSH, DIRECT; buffers one
    element behind a 16-byte boundary; AUTO with ll_bytes = 0"""
    outs = run_ranks("forms", size, timeout=240)
    assert "each with its form confirmed by the counters" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_host_slices_unregistered_memory_streams_and_iallreduce(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_captured_graph_replayed_with_new_inputs(size):
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_on_other_types_it_is_the_plain_sum_and_the_same_call(size):
    """f32 and i32: SUM_WIDE gives SUM's bits by every name, and ranks passing the one match ranks passing the other"""
    run_ranks("other_types", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_table_row_naming_a_stepped_schedule_runs_the_fold(size):
    """`tuned` = 1 and a hand-written row naming RING / RHD_PUSH / TREE: XMPI_SUM takes the stepped kernel, XMPI_SUM_WIDE the fold"""
    run_ranks("table", size, timeout=240)


@pytest.mark.parametrize("size", SIZES)
def test_a_stepped_name_is_refused_on_every_rank(size):
    """RING, RHD, TREE and their PUSH forms named by the caller: XMPI_ERR_UNSUPPORTED, nothing launched, the communicator usable"""
    run_ranks("refused", size, timeout=240)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_sum_against_sum_wide_are_different_calls(size, bf16):
    """above the LL limit the kernels compare their call signatures: XMPI_ERR_ARG on every rank, nothing moved"""
    outs = run_ranks("mismatch", size, {"bf16": bf16}, timeout=120)
    assert all("wide mismatch: ok" in o for o in outs), outs


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
    staged AUTO picks the TREE table for XMPI_SUM (DIRECT runs instead)"""
    run_ranks("layout", size, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})


# ---- the local kernels, on the CPU build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [xmpi.F16, xmpi.BF16])
def test_local_kernels(dtype):
    """xmpi_reduce_local_n / _multi: 1..9 and 16 sources, 1 / 2 / 8 destinations, every count, both alignments, every cache policy"""
    run_ranks("kernels", 1, {"dtype": dtype}, timeout=240)
