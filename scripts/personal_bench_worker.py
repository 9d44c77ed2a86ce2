"""One rank of the reduce-scatter / all-to-all measurement (profiles/personal/README.md), started by scripts/personal_bench.py:
  python scripts/personal_bench_worker.py <tree root> <rank> <size> <key> <plan> <reps>
plan: new (both collectives by LL / ZCOPY / AUTO at 1 ... 32 KiB per block, the fold and push-only at 1 and 32 MiB), parent (what
a build without them offers: allgather, allreduce), newold (parent's rows on a build that has them, the two at 1 MiB beside them),
pair (old and new interleaved in one set of processes).  Blocking calls back to back, host clock, a barrier before and behind;
rank 0 prints one JSON row per repetition."""
import json, os, sys, time
root, rank, size, key, plan, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], int(sys.argv[6])
sys.path.insert(0, root)
from mpi_amd import xmpi
if os.environ.get("XMPI_DEVSIM_LIB"):  # rehearsal only
    xmpi.LIB_PATH = os.environ["XMPI_DEVSIM_LIB"]
c = xmpi.Comm(rank, size, -1, key)
A = {"ll": xmpi.ALGO_LL, "zcopy": xmpi.ALGO_ZCOPY, "auto": xmpi.ALGO_AUTO, "zpush": xmpi.ALGO_ZPUSH}
KiB, MiB = 1 << 10, 1 << 20
maxblock = int(os.environ.get('PBENCH_MAXBLOCK', 32 * MiB))
BIG = [b for b in (1 * MiB, 32 * MiB) if b <= maxblock] or [maxblock]
send, recv = c.alloc(size * maxblock), c.alloc(size * maxblock)
c.fill(send, size * maxblock // 4, xmpi.F32, xmpi.PAT_SIGNED, 7 + rank)
c.memset(recv, 0, size * maxblock)

def timed(call, iters, warm):
    for _ in range(warm):
        call()
    c.barrier()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    dt = (time.perf_counter() - t0) / iters * 1e6
    c.barrier()
    return dt

def iters_for(b):
    return (3, 1) if os.environ.get('XMPI_DEVSIM_LIB') else (300, 20) if b <= 64 * KiB else (60, 5) if b <= 4 * MiB else (12, 3)

rows = []
def row(name, algo, block, call):
    it, warm = iters_for(block)
    for rep in range(reps):
        us = timed(call, it, warm)
        rows.append({"what": name, "algo": algo, "block_bytes": block, "ranks": size, "rep": rep, "us_per_call": round(us, 2), "iters": it})

if plan == "pair":  # one set of processes, old and new collectives interleaved: same placement, same clock state
    for rep in range(reps):
        for b in BIG:
            n = b // 4
            it, warm = iters_for(b)
            for name, algo, blk, call in (
                ("allgather", "zcopy", b, lambda: c.allgather(send, recv, n, xmpi.F32, A["zcopy"])),
                ("alltoall", "zcopy", b, lambda: c.alltoall(send, recv, n, xmpi.F32, A["zcopy"])),
                ("allreduce", "zcopy", size * b, lambda: c.allreduce(send, recv, size * n, xmpi.F32, xmpi.SUM, A["zcopy"])),
                ("reduce_scatter", "zcopy", b, lambda: c.reduce_scatter(send, recv, n, xmpi.F32, xmpi.SUM, A["zcopy"])),
                ("reduce_scatter", "zpush", b, lambda: c.reduce_scatter(send, recv, n, xmpi.F32, xmpi.SUM, A["zpush"]))):
                rows.append({"what": name, "algo": algo, "block_bytes": blk, "ranks": size, "rep": rep, "us_per_call": round(timed(call, it, warm), 2), "iters": it})
        for name, algo, call in (
            ("allgather", "zcopy", lambda: c.allgather(send, recv, 256, xmpi.F32, A["zcopy"])),
            ("alltoall", "zcopy", lambda: c.alltoall(send, recv, 256, xmpi.F32, A["zcopy"])),
            ("alltoall", "ll", lambda: c.alltoall(send, recv, 256, xmpi.F32, A["ll"])),
            ("allreduce", "zcopy", lambda: c.allreduce(send, recv, 256, xmpi.F32, xmpi.SUM, A["zcopy"])),
            ("reduce_scatter", "zcopy", lambda: c.reduce_scatter(send, recv, 256, xmpi.F32, xmpi.SUM, A["zcopy"])),
            ("reduce_scatter", "ll", lambda: c.reduce_scatter(send, recv, 256, xmpi.F32, xmpi.SUM, A["ll"]))):
            rows.append({"what": name, "algo": algo, "block_bytes": 1024, "ranks": size, "rep": rep, "us_per_call": round(timed(call, 300, 20), 2), "iters": 300})
elif plan == "new":
    for b in (1 * KiB, 4 * KiB, 8 * KiB, 16 * KiB, 32 * KiB):
        n = b // 4
        for algo in ("ll", "zcopy", "auto"):
            row("alltoall", algo, b, lambda: c.alltoall(send, recv, n, xmpi.F32, A[algo]))
            row("reduce_scatter", algo, b, lambda: c.reduce_scatter(send, recv, n, xmpi.F32, xmpi.SUM, A[algo]))
    for b in BIG:
        n = b // 4
        row("alltoall", "zcopy", b, lambda: c.alltoall(send, recv, n, xmpi.F32, A["zcopy"]))
        row("reduce_scatter", "zcopy", b, lambda: c.reduce_scatter(send, recv, n, xmpi.F32, xmpi.SUM, A["zcopy"]))
        row("reduce_scatter", "zpush", b, lambda: c.reduce_scatter(send, recv, n, xmpi.F32, xmpi.SUM, A["zpush"]))
    rows.append({"ll_bytes": c.get_param("ll_bytes"), "ranks": size})
else:
    n = KiB // 4
    row("allgather", "ll", KiB, lambda: c.allgather(send, recv, n, xmpi.F32, A["ll"]))
    row("allgather", "zcopy", KiB, lambda: c.allgather(send, recv, n, xmpi.F32, A["zcopy"]))
    for b in BIG:
        n = b // 4
        row("allgather", "zcopy", b, lambda: c.allgather(send, recv, n, xmpi.F32, A["zcopy"]))
    n = size * maxblock // 4
    row("allreduce", "zcopy", size * maxblock, lambda: c.allreduce(send, recv, n, xmpi.F32, xmpi.SUM, A["zcopy"]))
    n = size * BIG[0] // 4
    row("allreduce", "zcopy", size * BIG[0], lambda: c.allreduce(send, recv, n, xmpi.F32, xmpi.SUM, A["zcopy"]))
if plan == "newold":  # the four older collectives' rows on the NEW build, and the two new ones at 1 MiB beside them
    for b in BIG[:1]:
        n = b // 4
        row("alltoall", "zcopy", b, lambda: c.alltoall(send, recv, n, xmpi.F32, A["zcopy"]))
        row("reduce_scatter", "zcopy", b, lambda: c.reduce_scatter(send, recv, n, xmpi.F32, xmpi.SUM, A["zcopy"]))
c.barrier()
if rank == 0:
    for r in rows:
        print(json.dumps(dict(r, build=plan)))
c.finalize()
