"""xmpi_alltoallv without a GPU: the symbols and their bindings, the header's citations, the round schedule of the form for ranks
that meet on the host, the argument errors (on a communicator of one rank on a virtual device), the Go sources."""
import os
import subprocess

from mpi_amd import xmpi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xmpi_alltoallv", "xmpi_alltoallv_on_stream")


def test_symbols_and_bindings():
    L = xmpi.lib()
    bound = {name: args for name, _, args in xmpi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), name
        assert len(bound[name]) == 12, name
    for m in ("alltoallv", "alltoallv_on_stream"):
        assert callable(getattr(xmpi.Comm, m))
    assert L.xmpi_alltoallv(None, None, 0, None, None, None, 0, None, None, None, xmpi.U8, xmpi.ALGO_AUTO) == xmpi.ERR_STATE
    assert L.xmpi_alltoallv_on_stream(None, None, 0, None, None, None, 0, None, None, None, xmpi.U8, None) == xmpi.ERR_STATE


def test_the_header_cites_the_exchange_and_the_resizing_receive():
    text = open(os.path.join(ROOT, "include", "xmpi.h")).read()
    for name in NEW:
        comment = text[:text.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "helloworld.go:53-81" in comment and "network.go:594-601" in comment, name


def test_the_rounds_are_perfect_matchings():
    """ranks that meet on the host move the blocks in N rounds: in every round the partner's partner is the rank itself, and
    over the rounds every rank meets every rank -- itself included -- exactly once"""
    L = xmpi.lib()
    for n in range(2, 13):
        met = {r: [] for r in range(n)}
        for rnd in range(n):
            for r in range(n):
                p = L.xmpi_alltoallv_partner(rnd, r, n)
                assert 0 <= p < n and L.xmpi_alltoallv_partner(rnd, p, n) == r, (n, rnd, r, p)
                met[r].append(p)
        for r in range(n):
            assert sorted(met[r]) == list(range(n)), (n, r, met[r])
    assert L.xmpi_alltoallv_partner(0, 3, 3) == -1 and L.xmpi_alltoallv_partner(0, 0, 0) == -1


_WORKER = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from mpi_amd import xmpi
if len(sys.argv) > 2:
    xmpi.LIB_PATH = sys.argv[2]
c = xmpi.Comm(0, 1, -1, "vcoll-args")
L = xmpi.lib()
buf = c.alloc(4096)
a, b = buf.ptr, buf.ptr + 2048
one = lambda v: np.array([v], dtype=np.uint64)
def call(send, se, sc, sd, recv, re_, cap, rd, dtype=xmpi.F32, algo=xmpi.ALGO_AUTO, stream=False):
    got = np.full(1, 77, dtype=np.uint64)
    arrs = [one(sc), one(sd), one(cap), one(rd)]
    ptrs = [None if x is None else x.ctypes.data for x in arrs]
    if stream:
        rc = L.xmpi_alltoallv_on_stream(c.handle, send, se, ptrs[0], ptrs[1], recv, re_, ptrs[2], ptrs[3], got.ctypes.data, dtype, None)
    else:
        rc = L.xmpi_alltoallv(c.handle, send, se, ptrs[0], ptrs[1], recv, re_, ptrs[2], ptrs[3], got.ctypes.data, dtype, algo)
    return rc, int(got[0]), L.xmpi_last_error().decode()
def err(res, code, text):
    assert res[0] == code and text in res[2], res
# overlapping extents, decided from the arguments
err(call(a, 16, 16, 0, a, 16, 16, 0), xmpi.ERR_ARG, "overlap")
err(call(a, 16, 16, 0, a + 60, 16, 16, 0), xmpi.ERR_ARG, "overlap")
err(call(a, 16, 16, 0, a + 4, 16, 16, 0, stream=True), xmpi.ERR_ARG, "overlap")
# an algorithm the collective does not have: from the arguments alone, before anything else is looked at
for algo in (xmpi.ALGO_RING, xmpi.ALGO_RHD, xmpi.ALGO_TREE, xmpi.ALGO_ZPUSH, xmpi.ALGO_LL, xmpi.ALGO_RING_PUSH, 99, -1):
    err(call(a, 16, 16, 0, a, 16, 16, 0, algo=algo), xmpi.ERR_UNSUPPORTED, "alltoallv has no")
assert call(a, 16, 16, 0, b, 16, 16, 0, dtype=99)[0] == xmpi.ERR_ARG
assert call(None, 16, 16, 0, b, 16, 16, 0)[0] == xmpi.ERR_ARG
assert L.xmpi_alltoallv(c.handle, a, 16, None, None, b, 16, None, None, None, xmpi.F32, xmpi.ALGO_AUTO) == xmpi.ERR_ARG
# the stream form needs ranks that meet on the device
err(call(a, 16, 16, 0, b, 16, 16, 0, stream=True), xmpi.ERR_UNSUPPORTED, "meet on the device")
# a job of one: the own block goes through the same rules -- adjacent extents, zero extents, truncation, a row out of its extent
x = np.arange(16, dtype=np.float32)
buf.upload(x)
c.memset(b, 0xA5, 128)
assert call(a, 16, 16, 0, a + 64, 16, 16, 0)[:2] == (0, 16)
assert buf.download(np.float32, 16, byte_offset=64).tobytes() == x.tobytes()
assert call(None, 0, 0, 0, None, 0, 0, 0)[:2] == (0, 0)
c.memset(b, 0xA5, 128)
err(call(a, 16, 16, 0, b, 16, 15, 0), xmpi.ERR_TRUNCATE, "rank 0")
assert call(a, 16, 16, 0, b, 16, 15, 0)[1] == 16  # (the offered count)
err(call(a, 16, 16, 1, b, 16, 16, 0), xmpi.ERR_ARG, "rank 0")
err(call(a, 16, 4, 0, b, 16, 16, 1), xmpi.ERR_ARG, "rank 0")
assert np.all(buf.download(np.uint8, 128, byte_offset=2048) == 0xA5)
got = c.alltoallv(a, 16, [5], [2], b, 16, [9], [3], xmpi.F32, xmpi.ALGO_DIRECT)
assert list(got) == [5] and buf.download(np.float32, 5, byte_offset=2048 + 12).tobytes() == x[2:7].tobytes()
# the tag the host form keeps to itself is refused to callers
assert L.xmpi_send(c.handle, a, 1, xmpi.F32, 0, -2**31) == xmpi.ERR_ARG
c.finalize()
print("ok")
"""


def test_argument_errors(tmp_path):
    from tests.devsim import build
    lib = build.build_lib()
    script = tmp_path / "args.py"
    script.write_text(_WORKER)
    env = dict(os.environ, DEVSIM_DEVICES="1", XMPI_TIMEOUT_S="30")
    r = subprocess.run([os.sys.executable, str(script), ROOT, lib], capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def test_go_sources_call_the_new_entry_points():
    """(held to the header's parameter counts by tests/test_abi.py; here: that they are there at all)"""
    go = open(os.path.join(ROOT, "go", "xgmi", "xgmi.go")).read()
    for name in NEW:
        assert f"C.{name}(" in go, name
    coll = open(os.path.join(ROOT, "go", "mpi_collectives", "collectives.go")).read()
    assert "func Alltoallv(" in coll
