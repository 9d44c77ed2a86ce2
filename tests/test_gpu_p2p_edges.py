"""Send / Receive copies at every alignment and path boundary, on real hardware (tests/scenarios.py sc_p2p_edges): U8 payloads at the
lengths where copy_span (mpi_amd/csrc/kdev.h) or one of its callers changes paths -- packet or tail, one 16 KiB tile, the agent's
alone_bytes, the agent's limit, more tiles than blocks -- times five (source, destination) residue pairs modulo 16, every cell through
the receive agent, the pull kernel (also capped to 1 and 3 blocks), the plain copy, the mail slots by both transports and the
stream-ordered kernels (also capped, and once more into a 4 MiB capacity); then host -> device and device -> host around the lane's piece
and ring sizes and the pinned bounce.  Source and destination sit inside frames with different pad bytes; both sides compare the whole
frame on the device, so a byte written in front of or behind a destination shows like a wrong byte inside it.  The receiver's counters
confirm each form's transport.  A copy is exact: no tolerance anywhere."""
import pytest

from tests.gpu_harness import run_ranks, run_threads

pytestmark = pytest.mark.gpu

LENGTHS, PAIRS = 14, 5  # tests/scenarios.py EDGE_LENGTHS x EDGE_RESIDUES
BLOCKING = ["default", "pull cap=0", "pull cap=1", "pull cap=3", "copy", "slots engine=0", "slots engine=1"]
STREAM = ["stream cap=0", "stream cap=1", "stream cap=3"]
HOST_LEGS = ["host->device: 48 messages", "device->host: 48 messages"]


def every_form_ran(out, forms):
    """rank 1 printed one line per form, with the number of messages: lengths x residue pairs, nothing sampled"""
    for form in forms:
        assert f"p2p_edges {form}: {LENGTHS * PAIRS} messages" in out, f"form {form} did not report {LENGTHS * PAIRS} messages\n{out}"
    assert all(f"p2p_edges {leg}" in out for leg in HOST_LEGS), out
    print("\n".join(ln for ln in out.splitlines() if ln.startswith("p2p_edges")))


def test_every_cell_in_every_form_between_two_processes():
    out = run_ranks("p2p_edges", 2, {"expect_params": {"dsync": 1}}, timeout=300)[1]
    every_form_ran(out, BLOCKING + STREAM)


def test_ranks_that_meet_on_the_host():
    """XMPI_DSYNC=0: the stream-ordered kernels belong to ranks that meet on the device -- that form is absent here by design, and the
    scenario asserts dsync == 0 rather than skipping it quietly"""
    out = run_ranks("p2p_edges", 2, {"dsync": 0, "expect_params": {"dsync": 0}}, timeout=300, env={"XMPI_DSYNC": "0"})[1]
    every_form_ran(out, BLOCKING)
    assert "stream" not in out, out


def test_the_copy_kernel_as_transport():
    """XMPI_COPY_ENGINE=1: the plain copy and the slots' default transport are the copy kernel"""
    out = run_ranks("p2p_edges", 2, {"expect_params": {"dsync": 1, "copy_engine": 1}}, timeout=300, env={"XMPI_COPY_ENGINE": "1"})[1]
    every_form_ran(out, BLOCKING + STREAM)


def test_two_rank_threads_of_one_process():
    """the receiver reads the sender's frame through its own pointer; rank threads meet on the host (dsync == 0, asserted): no
    stream form"""
    out = run_threads("p2p_edges", 2, {"dsync": 0}, timeout=300)
    every_form_ran(out, BLOCKING)
    assert "stream" not in out, out


def test_concurrent_receives_beside_the_agent():
    """4 processes: rank 0 receives 65537, 70001 and 524289 bytes from ranks 1..3 at once (one thread each, one tag, destination
    residue = source rank, source residue 2r + 1) under p2p_grid_cap 0, 1 and 3: the agent serves one Receive of a round, the others
    launch the pull kernel beside it"""
    out = run_ranks("p2p_edges", 4, timeout=300)[0]
    assert "p2p_edges concurrent: 27 messages" in out, out
    print("\n".join(ln for ln in out.splitlines() if ln.startswith("p2p_edges")))
