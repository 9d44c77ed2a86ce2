"""xmpi_reduce_scatter and xmpi_alltoall without a GPU: the symbols and their bindings, the staged step tables of both (run on the
CPU by tests/plan_sim.py against a numpy expectation), the argument errors, and the two functions of the C++ host mirror."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mpi_amd import xmpi
from tests import plan_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xmpi_reduce_scatter", "xmpi_alltoall", "xmpi_reduce_scatter_on_stream", "xmpi_alltoall_on_stream")


def test_every_new_symbol_is_exported_and_bound():
    L = xmpi.lib()
    bound = {name: args for name, _, args in xmpi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), f"{name} is not exported by libxmpi.so"
        assert name in bound, f"{name} has no ctypes prototype in mpi_amd/xmpi.py"
    assert len(bound["xmpi_reduce_scatter"]) == 7 and len(bound["xmpi_alltoall"]) == 6
    assert len(bound["xmpi_reduce_scatter_on_stream"]) == 7 and len(bound["xmpi_alltoall_on_stream"]) == 6
    assert (xmpi.COLL_REDUCE_SCATTER, xmpi.COLL_ALLTOALL) == (4, 5)
    for m in ("reduce_scatter", "alltoall", "reduce_scatter_on_stream", "alltoall_on_stream"):
        assert callable(getattr(xmpi.Comm, m))


def test_the_header_says_where_the_reference_stands():
    text = open(os.path.join(ROOT, "include", "xmpi.h")).read()
    for name in NEW[:2]:
        comment = text[:text.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "absent from the reference, mpi.go:130" in comment, name
    assert "helloworld.go:53-81" in text[:text.index("int xmpi_alltoall(")].rsplit("/*", 1)[1]


def _inputs(size, count, dt, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dt, np.floating):
        return [rng.standard_normal(size * count).astype(dt) for _ in range(size)]
    return [rng.integers(-1000, 1000, size * count).astype(dt) for _ in range(size)]


@pytest.mark.parametrize("size", [2, 3, 4, 7, 8, 16])
@pytest.mark.parametrize("count,piece", [(1, 64), (5, 4), (1003, 256), (4099, 1 << 20)])
def test_staged_tables_against_numpy(size, count, piece):
    """xmpi_plan_dump of collectives 4 and 5 -- DIRECT, and AUTO, which means DIRECT -- through plan_sim.simulate: ragged counts
    (blocks that start at no multiple of 16 bytes), pieces smaller and larger than a block, shallow FIFOs, random schedules"""
    for dt, op in ((np.float32, xmpi.SUM), (np.int64, xmpi.MAX), (np.float64, xmpi.PROD)):
        es = np.dtype(dt).itemsize
        ins = _inputs(size, count, dt, 17 * size + count)
        for algo in ((xmpi.ALGO_DIRECT, xmpi.ALGO_AUTO) if dt is np.float32 else (xmpi.ALGO_DIRECT,)):
            plans = plan_sim.get_plans(xmpi.COLL_REDUCE_SCATTER, algo, size, 0, count, es, 1, piece)
            assert all(p.algo == xmpi.ALGO_DIRECT and p.temp_bytes == 0 for p in plans)
            got = plan_sim.simulate(plans, ins, count, dt, op, fifo_depth=2, seed=size + count)
            for me in range(size):
                want = ins[0][me * count:(me + 1) * count].copy()
                for r in range(1, size):  # rank order 0..N-1, left to right
                    want = plan_sim.np_combine(want, ins[r][me * count:(me + 1) * count], op)
                assert got[me].tobytes() == want.tobytes(), f"reduce_scatter rank {me}/{size} count {count}"
            plans = plan_sim.get_plans(xmpi.COLL_ALLTOALL, algo, size, 0, count, es, 1, piece)
            got = plan_sim.simulate(plans, ins, size * count, dt, op, fifo_depth=2, seed=size * count)
            for me in range(size):
                want = np.concatenate([ins[r][me * count:(me + 1) * count] for r in range(size)])
                assert got[me].tobytes() == want.tobytes(), f"alltoall rank {me}/{size} count {count}"


def test_staged_tables_have_no_other_schedule():
    for coll in (xmpi.COLL_REDUCE_SCATTER, xmpi.COLL_ALLTOALL):
        for algo in (xmpi.ALGO_RING, xmpi.ALGO_RHD, xmpi.ALGO_TREE):
            with pytest.raises(xmpi.XmpiError) as ei:
                xmpi.plan_text(coll, algo, 4, 0, 0, 100, 4, 1, 64, 2, 0)
            assert ei.value.code == xmpi.ERR_UNSUPPORTED


_WORKER = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from mpi_amd import xmpi
if len(sys.argv) > 2:
    xmpi.LIB_PATH = sys.argv[2]
c = xmpi.Comm(0, 1, -1, "personal-args")
L = xmpi.lib()
buf = c.alloc(4096)
a, b = buf.ptr, buf.ptr + 2048
def err(rc, code, text):
    assert rc == code, (rc, code, L.xmpi_last_error())
    assert text in L.xmpi_last_error().decode(), L.xmpi_last_error()
# in place, overlapping
err(L.xmpi_reduce_scatter(c.handle, a, a, 16, xmpi.F32, xmpi.SUM, xmpi.ALGO_AUTO), xmpi.ERR_ARG, "out of place")
err(L.xmpi_alltoall(c.handle, a, a, 16, xmpi.F32, xmpi.ALGO_AUTO), xmpi.ERR_ARG, "out of place")
err(L.xmpi_alltoall(c.handle, a, a + 60, 16, xmpi.F32, xmpi.ALGO_ZCOPY), xmpi.ERR_ARG, "overlap")
err(L.xmpi_reduce_scatter(c.handle, a + 60, a, 16, xmpi.F32, xmpi.SUM, xmpi.ALGO_LL), xmpi.ERR_ARG, "overlap")
err(L.xmpi_alltoall_on_stream(c.handle, a, a + 4, 16, xmpi.F32, None), xmpi.ERR_ARG, "overlap")
err(L.xmpi_reduce_scatter_on_stream(c.handle, a, a, 16, xmpi.F32, xmpi.SUM, None), xmpi.ERR_ARG, "out of place")
assert L.xmpi_alltoall(c.handle, a, a + 64, 16, xmpi.F32, xmpi.ALGO_AUTO) == 0  # (adjacent is not overlapping)
# an algorithm the collective does not have: from the arguments alone, with a text -- even for count == 0
for algo in (xmpi.ALGO_RING, xmpi.ALGO_RHD, xmpi.ALGO_TREE, xmpi.ALGO_RING_PUSH, xmpi.ALGO_RHD_PUSH, xmpi.ALGO_TREE_PUSH):
    err(L.xmpi_reduce_scatter(c.handle, a, b, 16, xmpi.F32, xmpi.SUM, algo), xmpi.ERR_UNSUPPORTED, "reduce_scatter has no")
    err(L.xmpi_alltoall(c.handle, a, b, 16, xmpi.F32, algo), xmpi.ERR_UNSUPPORTED, "alltoall has no")
    err(L.xmpi_alltoall(c.handle, a, b, 0, xmpi.F32, algo), xmpi.ERR_UNSUPPORTED, "alltoall has no")
err(L.xmpi_alltoall(c.handle, a, b, 16, xmpi.F32, xmpi.ALGO_ZPUSH), xmpi.ERR_UNSUPPORTED, "zcopy | ll | direct | auto")
assert L.xmpi_reduce_scatter(c.handle, a, b, 16, xmpi.F32, xmpi.SUM, 99) == xmpi.ERR_ARG
assert L.xmpi_alltoall(c.handle, a, b, 16, 99, xmpi.ALGO_AUTO) == xmpi.ERR_ARG
assert L.xmpi_reduce_scatter(c.handle, a, b, 16, xmpi.F32, 9, xmpi.ALGO_AUTO) == xmpi.ERR_ARG
assert L.xmpi_reduce_scatter(c.handle, None, b, 16, xmpi.F32, xmpi.SUM, xmpi.ALGO_AUTO) == xmpi.ERR_ARG
# count == 0: nothing to do, whatever the buffers
for algo in (xmpi.ALGO_AUTO, xmpi.ALGO_ZCOPY, xmpi.ALGO_LL, xmpi.ALGO_DIRECT):
    assert L.xmpi_reduce_scatter(c.handle, a, a, 0, xmpi.F32, xmpi.SUM, algo) == 0
    assert L.xmpi_alltoall(c.handle, None, None, 0, xmpi.F32, algo) == 0
assert L.xmpi_reduce_scatter(c.handle, a, a, 0, xmpi.F32, xmpi.SUM, xmpi.ALGO_ZPUSH) == 0
assert L.xmpi_reduce_scatter_on_stream(c.handle, a, a, 0, xmpi.F32, xmpi.SUM, None) == 0
assert L.xmpi_alltoall_on_stream(c.handle, None, None, 0, xmpi.F32, None) == 0
assert L.xmpi_alltoall(None, a, b, 16, xmpi.F32, xmpi.ALGO_AUTO) == xmpi.ERR_STATE
# a job of one: the result is the input
x = np.arange(16, dtype=np.float32)
buf.upload(x)
c.reduce_scatter(a, b, 16, xmpi.F32, xmpi.SUM)
assert buf.download(np.float32, 16, byte_offset=2048).tobytes() == x.tobytes()
c.memset(b, 0, 64)
c.alltoall(a, b, 16, xmpi.F32, xmpi.ALGO_DIRECT)
assert buf.download(np.float32, 16, byte_offset=2048).tobytes() == x.tobytes()
c.finalize()
print("ok")
"""


def test_argument_errors(tmp_path):
    """in place, overlap, an algorithm the collective does not have, count == 0 -- on a communicator of one rank on a virtual device
    (tests/devsim: the checks sit in front of everything that would need a GPU, a communicator needs a device to exist)"""
    from tests.devsim import build
    lib = build.build_lib()
    script = tmp_path / "args.py"
    script.write_text(_WORKER)
    env = dict(os.environ, DEVSIM_DEVICES="1", XMPI_TIMEOUT_S="30")
    r = subprocess.run([os.sys.executable, str(script), ROOT, lib], capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def test_host_mirror(tmp_path):
    """mpi::ReduceScatter / mpi::Alltoall: probe of the backend, the default of a backend that lacks them, block arithmetic"""
    exe = str(tmp_path / "personal_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "mpi_amd", "host"), os.path.join(ROOT, "tests", "personal_host_check.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "mpi_amd"), "-lxmpi_host", "-lxmpi",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpi_amd"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_go_sources_call_the_new_entry_points():
    """(held to the header's parameter counts by tests/test_abi.py; here: that they are there at all)"""
    go = open(os.path.join(ROOT, "go", "xgmi", "xgmi.go")).read()
    for name in NEW:
        assert f"C.{name}(" in go, name
    coll = open(os.path.join(ROOT, "go", "mpi_collectives", "collectives.go")).read()
    assert "func ReduceScatter(" in coll and "func Alltoall(" in coll
