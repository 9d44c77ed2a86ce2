"""XMPI_BAND / XMPI_BOR / XMPI_BXOR on the MI355X: one process per rank sharing the GPU (the real multi-process hipIpc path, the ranks
meeting on the device), the other layouts at one size each, and the local kernels.  Scenarios: tests/bitop_scenarios.py, every result
compared bit for bit with the numpy restatement of the operator (tests/bitop_ref.py).  What stays with the virtual devices
(tests/test_bitop_devsim.py): ranks in different calls -- an error path, run where nothing can wedge a GPU.  (The refusal of a float
type or of an unknown operator is decided on the host before any launch: it runs here too.)

Every job of ranks runs in child processes (tests/bitop_worker.py): the test runner itself never opens the GPU."""
import pytest

from tests import bitop_ref as br
from tests.bitop_harness import run_ranks, run_threads

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 8]


def _args(size, **kw):
    """8 processes share ONE GPU here and take turns on it -- a collective costs tens of milliseconds --, so the jobs of 8 run the
    covering subsets of tests/bitop_scenarios.py (sc_names says what they cover); the products run with 2 and 3 processes here and at
    every size on the virtual devices"""
    return dict(kw, cover=1) if size == 8 else kw


@pytest.mark.parametrize("dtype", br.DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_algorithm_name_at_every_count(size, dtype):
    outs = run_ranks("names", size, _args(size, dtype=dtype), timeout=120)
    assert "calls checked" in outs[0]


@pytest.mark.parametrize("dtype", br.DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_every_form_forced_and_confirmed_by_the_launch_counters(size, dtype):
    outs = run_ranks("forms", size, _args(size, dtype=dtype), timeout=120)
    assert "each with its form confirmed by the counters" in outs[0]


@pytest.mark.parametrize("size", SIZES)
def test_host_slices_unregistered_memory_streams_and_nonblocking(size):
    run_ranks("memory", size, _args(size), timeout=120)


@pytest.mark.parametrize("size", SIZES)
def test_a_captured_graph_replayed_with_new_inputs(size):
    run_ranks("graph", size, timeout=120)


@pytest.mark.parametrize("size", SIZES)
def test_a_float_type_is_refused_at_every_entry(size):
    outs = run_ranks("float_refused", size, timeout=120)
    assert "calls refused" in outs[0]


def test_operators_8_and_minus_1_are_refused():
    run_ranks("bad_op", 3, timeout=120)


def test_rank_threads_in_one_process():
    run_threads("layout", 4, {"expect_host_fold": 1}, timeout=120)


def test_ranks_that_meet_on_the_host():
    run_ranks("layout", 3, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=120, env={"XMPI_DSYNC": "0"})


def test_staged_tables():
    run_ranks("layout", 3, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=120,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})


@pytest.mark.parametrize("dtype", br.DTYPES)
def test_local_kernels(dtype):
    outs = run_ranks("local", 1, {"dtype": dtype}, timeout=120)
    assert "launches checked" in outs[0]
