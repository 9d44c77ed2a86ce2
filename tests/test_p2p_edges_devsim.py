"""Send / Receive at every alignment and path boundary on virtual devices (tests/devsim: the library's host and kernel sources compiled
for the CPU over a HIP runtime with N virtual devices -- see tests/test_devsim.py): the layouts of tests/test_gpu_p2p_edges.py, plus 3
and 8 ranks for the concurrent Receives.  What this shows is that the scenario (tests/scenarios.py sc_p2p_edges) and copy_span's index
arithmetic hold before either reaches a GPU; the compiled packet stores, the loads in flight and the block striding are the GPU
suite's.  No GPU."""
import os

import pytest

from tests.gpu_harness import run_ranks, run_threads

LENGTHS, PAIRS = 14, 5  # tests/scenarios.py EDGE_LENGTHS x EDGE_RESIDUES


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


def every_form_ran(out, forms):
    """rank 1 printed one line per form, with the number of messages: lengths x residue pairs, nothing sampled"""
    for form in forms:
        assert f"p2p_edges {form}: {LENGTHS * PAIRS} messages" in out, f"form {form} did not report {LENGTHS * PAIRS} messages\n{out}"


BLOCKING = ["default", "pull cap=0", "pull cap=1", "pull cap=3", "copy", "slots engine=0", "slots engine=1"]
STREAM = ["stream cap=0", "stream cap=1", "stream cap=3"]
HOST_LEGS = ["host->device: 48 messages", "device->host: 48 messages"]


def test_every_cell_in_every_form_between_two_processes():
    out = run_ranks("p2p_edges", 2, {"expect_params": {"dsync": 1}}, timeout=240)[1]
    every_form_ran(out, BLOCKING + STREAM)
    assert all(f"p2p_edges {leg}" in out for leg in HOST_LEGS), out


def test_ranks_that_meet_on_the_host():
    """XMPI_DSYNC=0: the stream-ordered kernels belong to ranks that meet on the device -- that form is absent here by design"""
    out = run_ranks("p2p_edges", 2, {"dsync": 0, "expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})[1]
    every_form_ran(out, BLOCKING)
    assert "stream" not in out, out


def test_the_copy_kernel_as_transport():
    out = run_ranks("p2p_edges", 2, {"expect_params": {"dsync": 1, "copy_engine": 1}}, timeout=240, env={"XMPI_COPY_ENGINE": "1"})[1]
    every_form_ran(out, BLOCKING + STREAM)


def test_two_rank_threads_of_one_process():
    """(rank threads meet on the host: no stream form)"""
    out = run_threads("p2p_edges", 2, {"dsync": 0}, timeout=240)
    every_form_ran(out, BLOCKING)


@pytest.mark.parametrize("size", [3, 4, 8])
def test_concurrent_receives_beside_the_agent(size):
    out = run_ranks("p2p_edges", size, timeout=240)[0]
    assert f"p2p_edges concurrent: {9 * (size - 1)} messages" in out, out
