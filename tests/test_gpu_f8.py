"""XMPI_F8E4M3 / XMPI_F8E5M2 on the MI355X: one process per rank sharing the GPU (the real multi-process hipIpc path, the ranks meeting
on the device), then the other layouts at one size each.  Scenarios: tests/f8_scenarios.py, every result held to the numpy
restatement of the two types (tests/f8_ref.py): here the packed gfx950 conversion instructions do the widening and the narrowing,
and the exhaustive-pair jobs are what holds them to the definition.  What stays with the virtual devices
(tests/test_f8_devsim.py): ranks in different calls -- an error path, run where nothing can wedge a GPU.  (The refusals of a stepped
name and of a bitwise operator are decided on the host before any launch: they run here too.)

Every job of ranks runs in child processes (tests/f8_worker.py): the test runner itself never opens the GPU."""
import pytest

from tests import f8_ref as fr
from tests.f8_harness import run_ranks, run_threads

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 8]


def _args(size, **kw):
    """8 processes share ONE GPU here and take turns on it -- a collective costs tens of milliseconds --, so the jobs of 8 run the
    covering subsets of tests/f8_scenarios.py (sc_names says what they cover); the products run with 2 and 3 processes here and at
    every size on the virtual devices"""
    return dict(kw, cover=1) if size == 8 else kw


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_pair_of_encodings_under_every_operator(size, dtype):
    outs = run_ranks("pairs", size, {"dtype": dtype}, timeout=120)
    assert "f8 pairs" in outs[0]


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_algorithm_name_at_every_count(size, dtype):
    outs = run_ranks("names", size, _args(size, dtype=dtype), timeout=120)
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_form_forced_and_confirmed_by_the_launch_counters(size, dtype):
    outs = run_ranks("forms", size, _args(size, dtype=dtype), timeout=120)
    assert "each with its form confirmed by the counters" in outs[0]


@pytest.mark.parametrize("dtype", fr.F8_DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_host_slices_unregistered_memory_streams_iallreduce_and_repeat(size, dtype):
    run_ranks("memory", size, _args(size, dtype=dtype), timeout=120)


@pytest.mark.parametrize("size", SIZES)
def test_a_captured_graph_replayed_with_new_inputs(size):
    run_ranks("graph", size, timeout=120)


@pytest.mark.parametrize("size", SIZES)
def test_a_table_row_naming_a_stepped_schedule_runs_the_fold(size):
    run_ranks("table", size, timeout=120)


@pytest.mark.parametrize("size", SIZES)
def test_a_stepped_name_and_a_bitwise_operator_are_refused_on_every_rank(size):
    run_ranks("refused", size, timeout=120)


@pytest.mark.parametrize("size", SIZES)
def test_everything_without_an_operator_moves_them_as_bytes(size):
    outs = run_ranks("moves", size, _args(size), timeout=120)
    assert "f8 moves" in outs[0]


def test_rank_threads_in_one_process():
    run_threads("layout", 4, {"expect_host_fold": 1}, timeout=120)


def test_ranks_that_meet_on_the_host():
    run_ranks("layout", 3, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=120, env={"XMPI_DSYNC": "0"})


def test_staged_tables():
    run_ranks("layout", 3, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=120,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})
