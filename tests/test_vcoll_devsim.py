"""xmpi_alltoallv on virtual devices (tests/devsim: the library's host and kernel sources compiled for the CPU over a HIP runtime
with N virtual devices -- see tests/test_devsim.py): one process per device, the layouts whose ranks meet on the host, the error
paths -- which run here only, where nothing can wedge a GPU -- and the new kernel and the v-box protocol under ThreadSanitizer and
UBSan in a stand-alone driver.  Scenarios: tests/vcoll_scenarios.py; every result is compared whole, byte for byte.  No GPU."""
import os
import subprocess

import pytest

from tests.vcoll_harness import run_ranks, run_threads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "devsim")
HOST = {"expect_host": 1, "expect_params": {"dsync": 0}}


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
@pytest.mark.parametrize("size", [2, 3, 8])
def test_every_layout_dtype_and_algorithm_name(size):
    """packed, slotted with gaps, odd base (head + packets + tail), residues that differ (one element per lane), skewed -- on U8,
    F16, I64 by AUTO / ZCOPY / DIRECT; dsync_v_launches says which path ran"""
    run_ranks("layouts", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_equal_counts_give_what_alltoall_gives(size):
    run_ranks("equal", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_host_slices_unregistered_memory_and_the_stream_form(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_a_captured_graph_replays_with_new_counts(size):
    """captured once, replayed 3 times with a different count matrix written into the device arrays before each replay"""
    run_ranks("graph", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_forty_calls_back_to_back_between_other_collectives(size):
    run_ranks("back_to_back", size, timeout=240)


# ---- ranks that meet on the host ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 3, 8])
def test_ranks_that_meet_on_the_host(size):
    """XMPI_DSYNC=0: the pairs through xmpi_alltoall, the blocks over Send / Receive in N rounds"""
    run_ranks("layouts", size, HOST, timeout=240, env={"XMPI_DSYNC": "0"})
    run_ranks("memory", size, {"expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", [2, 4, 7])
def test_rank_threads_in_one_process(size):
    run_threads("layouts", size, {"expect_host": 1}, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_without_zero_copy(size):
    """XMPI_DSYNC=0 XMPI_ZERO_COPY=0; and XMPI_ZERO_COPY=0 alone, where ZCOPY by name still runs the kernel"""
    run_ranks("layouts", size, {"expect_host": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})
    run_ranks("layouts", size, {"expect_params": {"zero_copy": 0}}, timeout=240, env={"XMPI_ZERO_COPY": "0"})


@pytest.mark.parametrize("size", [9, 12])
def test_more_ranks_than_the_device_side_serves(size):
    """9 and 12 ranks on 8 devices: they meet on the host"""
    run_ranks("layouts", size, dict(HOST, algos=[0, 3]), timeout=300, env={"DEVSIM_DEVICES": "8"})
    run_ranks("errors", size, {"expect_params": {"dsync": 0}}, timeout=300, env={"DEVSIM_DEVICES": "8"})


# ---- error paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 3, 8])
def test_truncation_bounds_overlap_and_bad_algorithm_names(size):
    """a pair over capacity: XMPI_ERR_TRUNCATE on exactly its two ranks, the offered count reported, the slot untouched, every other
    block delivered, the next call clean; a row out of its extents: XMPI_ERR_ARG on that rank, nothing written outside; overlapping
    buffers; an algorithm the collective does not have -- by the kernel, and by the form for ranks that meet on the host"""
    run_ranks("errors", size, timeout=120)
    run_ranks("errors", size, {"algo": 3}, timeout=120)
    run_ranks("errors", size, {"expect_params": {"dsync": 0}}, timeout=120, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", [2, 3, 8])
def test_the_stream_form_reports_through_stream_sync(size):
    """XMPI_ERR_TRUNCATE / XMPI_ERR_ARG of an enqueued call arrive with the xmpi_stream_sync behind it, on the ranks concerned only,
    the other blocks delivered; pageable host arrays are refused from the arguments"""
    run_ranks("stream_errors", size, timeout=120)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_a_rank_in_xmpi_alltoall_instead(size):
    outs = run_ranks("mismatch", size, timeout=120)
    assert all("vcoll mismatch: ok" in o for o in outs), outs


# ---- sanitizers: a stand-alone driver, nothing sanitised is loaded into python ------------------------------------------------------
def _driver(tag, flags, link_flags):
    from mpi_amd import build as b
    from tests.devsim import build
    objs, rebuilt = build._objects(tag, flags, [os.path.join(HERE, "driver_vcoll.cpp")], False)
    out = os.path.join(HERE, f"vcoll_{tag}_bin")
    link = b._digest(objs, f"devsim vcoll driver link {tag}")
    if rebuilt or b._stale(out, link):
        b._run([build._clang(), *link_flags, *objs, "-o", out, "-lpthread", "-lrt", "-ldl"])
        b._record(out, link)
    return out


def _run(binp, *args, **env):
    e = dict(os.environ, TSAN_OPTIONS="exitcode=66 halt_on_error=0 report_signal_unsafe=0", **{k: str(v) for k, v in env.items()})
    e.pop("XMPI_DEVSIM_LIB", None)
    return subprocess.run([binp, *args], capture_output=True, text=True, timeout=600, env=e, cwd="/tmp")


@pytest.fixture(scope="module")
def tsan_bin():
    from tests.devsim import build
    return _driver("tsan", build._flags("-O1", "-fsanitize=thread"), ["-fsanitize=thread"])


@pytest.mark.parametrize("args,fuzz", [(("2", "1"), 0), (("5", "1"), 5), (("8", "1"), 9), (("--shared", "4", "1"), 3)])
def test_the_kernel_and_the_box_protocol_are_race_free(tsan_bin, args, fuzz):
    r = _run(tsan_bin, *args, DEVSIM_FUZZ=fuzz)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0 and "vcoll driver ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


@pytest.mark.parametrize("ranks,fuzz", [("3", 2), ("8", 5)])
def test_the_undefined_behaviour_sanitizer_finds_nothing(ranks, fuzz):
    from tests.devsim import build
    binp = _driver("ubsan", build._flags("-O1", "-fsanitize=undefined,bounds", "-fno-omit-frame-pointer"), ["-fsanitize=undefined"])
    r = _run(binp, ranks, "1", DEVSIM_FUZZ=fuzz, UBSAN_OPTIONS="print_stacktrace=1")
    assert r.returncode == 0 and "vcoll driver ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_example_program_under_the_launcher(devsim_lib, tmp_path):
    """examples/alltoallv under xmpirun at 4 ranks, one process per virtual GPU: what the reference's hello-world prints, the
    message a rank sends itself being of another length than the one it sends a peer (mpi::Alltoallv re-sizes the destination)"""
    os.symlink(devsim_lib, tmp_path / "libxmpi.so")  # (LD_LIBRARY_PATH comes before the binaries' RUNPATH: tests/test_devsim.py `stage`)
    binp = os.path.join(ROOT, "mpi_amd", "bin")
    e = dict(os.environ, LD_LIBRARY_PATH=str(tmp_path), XMPI_TIMEOUT_S="60", XMPI_NGPUS="4", DEVSIM_DEVICES="4", XMPI_BASEPORT="7490")
    e.pop("XMPI_DEVSIM_LIB", None)
    r = subprocess.run([os.path.join(binp, "xmpirun"), "4", os.path.join(binp, "alltoallv")], capture_output=True, text=True, timeout=120,
                       cwd=ROOT, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = [f"Hello world, I'm node {k} in a land with 4 nodes" for k in range(4)]
    for me in range(4):
        for frm in range(4):
            text = f"\"I'm just node {me} talking to myself\"" if frm == me else f"\"Hello node {me}, I'm node {frm}\""
            want.append(f"I, node {me}, received a message: {text}")
    assert sorted(r.stdout.splitlines()) == sorted(want), r.stdout
