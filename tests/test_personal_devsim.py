"""xmpi_reduce_scatter and xmpi_alltoall on virtual devices (tests/devsim: the library's host and kernel sources compiled for the
CPU over a HIP runtime with N virtual devices -- see tests/test_devsim.py): one process per device, the other layouts and the
clean errors, and the new kernels and plans under ThreadSanitizer and UBSan.  Scenarios: tests/personal_scenarios.py; every result
is held to the oracle bit for bit.  No GPU involved."""
import os
import subprocess

import pytest

from tests.personal_harness import run_ranks, run_threads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "devsim")


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
@pytest.mark.parametrize("size", [2, 3, 5, 8])
def test_every_algorithm_name(size):
    """ZCOPY | ZPUSH | LL | DIRECT | AUTO (all-to-all: without ZPUSH) below and above the LL limit, and a count large enough for
    meet / body / done (dsync_split_bytes, as for the allreduce): the same bits by every name"""
    run_ranks("algos", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 5, 8])
def test_every_dtype_and_operation_at_every_count(size):
    """7 dtypes x 4 operations at {1, 3, 17, 1000, 4099, 65536 + 5} elements per block"""
    run_ranks("sweep", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 5, 8])
def test_host_slices_unregistered_memory_and_streams(size):
    run_ranks("memory", size, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 5, 8])
def test_a_captured_graph_replayed(size):
    """{alltoall, reduce_scatter, allreduce} captured once, replayed 3 times with new inputs"""
    run_ranks("graph", size, timeout=240)


# ---- other layouts and clean errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 5, 8])
def test_slot_parity_across_kinds_of_collective(size):
    """50 calls back to back: LL all-to-all / LL allreduce / fold reduce-scatter / LL reduce-scatter, no barrier between them"""
    run_ranks("parity", size, timeout=240)


@pytest.mark.parametrize("size", [2, 4, 7])
def test_rank_threads_in_one_process(size):
    run_threads("layout", size, {"expect_host_fold": 1}, timeout=240)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_ranks_that_meet_on_the_host(size):
    """XMPI_DSYNC=0: zcopy.cpp's rendezvous -- one fold kernel with a single destination, one batch of N copies"""
    run_ranks("layout", size, {"expect_host_fold": 1, "expect_params": {"dsync": 0}}, timeout=240, env={"XMPI_DSYNC": "0"})


@pytest.mark.parametrize("size", [2, 3, 8])
def test_staged_tables(size):
    """XMPI_DSYNC=0 XMPI_ZERO_COPY=0: the step tables of plan.cpp through the windows"""
    run_ranks("layout", size, {"expect_staged": 1, "expect_params": {"dsync": 0, "zero_copy": 0}}, timeout=240,
              env={"XMPI_DSYNC": "0", "XMPI_ZERO_COPY": "0"})


@pytest.mark.parametrize("size", [9, 12])
def test_more_ranks_than_the_device_side_serves(size):
    """9 and 12 ranks on 8 devices: they meet on the host"""
    run_ranks("layout", size, {"counts": [17, 4099], "expect_params": {"dsync": 0}}, timeout=300, env={"DEVSIM_DEVICES": "8"})


@pytest.mark.parametrize("size", [3, 8, 9])
def test_reduce_scatter_on_hard_floats(size):
    """tests/hard_inputs.py data (full mantissas; NaNs, infinities, signed zeros, subnormals planted in every block) through
    reduce-scatter by every name and form and through all-to-all; 9 ranks on 8 devices meet on the host"""
    run_ranks("hard", size, {"expect_params": {"dsync": 0}} if size > 8 else None, timeout=300, env={"DEVSIM_DEVICES": "8"} if size > 8 else None)


@pytest.mark.parametrize("size", [2, 3, 8])
def test_ranks_in_different_calls_all_get_an_error(size):
    """an all-to-all against a reduce-scatter over the same bytes, above the LL limit: XMPI_ERR_ARG on every rank, nothing moved"""
    outs = run_ranks("mismatch", size, timeout=120)
    assert all("personal mismatch: ok" in o for o in outs), outs


# ---- sanitizers and the example program ---------------------------------------------------------------------------------------------
def _driver(tag, flags, link_flags):
    from mpi_amd import build as b
    from tests.devsim import build
    objs, rebuilt = build._objects(tag, flags, [os.path.join(HERE, "driver_personal.cpp")], False)
    out = os.path.join(HERE, f"personal_{tag}_bin")
    link = b._digest(objs, f"devsim personal driver link {tag}")
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
def test_the_new_kernels_and_plans_are_race_free(tsan_bin, args, fuzz):
    """ranks as threads, every rank on a device of its own (--shared: all on device 0, meeting on the host), under ThreadSanitizer
    with the kernels' data stores as plain stores: zero reports"""
    r = _run(tsan_bin, *args, DEVSIM_FUZZ=fuzz)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0 and "personal driver ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


@pytest.mark.parametrize("ranks,fuzz", [("3", 2), ("8", 5)])
def test_the_undefined_behaviour_sanitizer_finds_nothing(ranks, fuzz):
    from tests.devsim import build
    binp = _driver("ubsan", build._flags("-O1", "-fsanitize=undefined,bounds", "-fno-omit-frame-pointer"), ["-fsanitize=undefined"])
    r = _run(binp, ranks, "1", DEVSIM_FUZZ=fuzz, UBSAN_OPTIONS="print_stacktrace=1")
    assert r.returncode == 0 and "personal driver ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_example_program_under_the_launcher(devsim_lib, tmp_path):
    """examples/alltoall under xmpirun at 4 ranks, one process per virtual GPU: `ok` from every rank"""
    os.symlink(devsim_lib, tmp_path / "libxmpi.so")  # (LD_LIBRARY_PATH comes before the binaries' RUNPATH: tests/test_devsim.py `stage`)
    binp = os.path.join(ROOT, "mpi_amd", "bin")
    e = dict(os.environ, LD_LIBRARY_PATH=str(tmp_path), XMPI_TIMEOUT_S="60", XMPI_NGPUS="4", DEVSIM_DEVICES="4", XMPI_BASEPORT="7480")
    e.pop("XMPI_DEVSIM_LIB", None)
    for n in ("1000", "7"):
        r = subprocess.run([os.path.join(binp, "xmpirun"), "4", os.path.join(binp, "alltoall"), n], capture_output=True, text=True, timeout=120,
                           cwd=ROOT, env=e)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(ln for ln in r.stdout.splitlines() if ln.endswith(": ok")) == [f"rank {k} of 4: ok" for k in range(4)], r.stdout
