"""python scripts/vcoll_bench.py <ranks> <reps> <out file>: the xmpi_alltoallv measurement (profiles/vcoll/README.md) -- one process
per rank on the visible GPU(s), rank 0's rows appended to the file.  In ONE set of processes, interleaved per repetition:
  equal    xmpi_alltoallv with equal counts against xmpi_alltoall (ZCOPY) of the same bytes, at 1 KiB, 64 KiB, 1 MiB, 32 MiB per block
  skewed   a count matrix with one block 64 x the others against the equal matrix of the same total bytes
Blocking calls back to back, host clock, a barrier before and behind; one JSON row per repetition.
(python scripts/vcoll_bench.py --worker <rank> <size> <key> <reps>: one rank of it.)"""
import json, os, subprocess, sys, time, uuid

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(here)


def launcher():
    size, reps, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
    key = f"vb{os.getpid()}-{uuid.uuid4().hex[:6]}"
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", XMPI_TIMEOUT_S="60")
    ps = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(r), str(size), key, reps], env=e, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True) for r in range(size)]
    rc = 0
    for r, p in enumerate(ps):
        try:
            o, _ = p.communicate(timeout=280)
        except subprocess.TimeoutExpired:
            p.kill(); o = p.communicate()[0] + "\n[killed after timeout]"
        if p.returncode != 0:
            rc = 1
            print(f"--- rank {r} exit {p.returncode}\n{o[-3000:]}")
        elif r == 0:
            with open(out, "a") as f:
                f.write(o)
            print(o)
    sys.exit(rc)


def worker():
    rank, size, key, reps = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
    sys.path.insert(0, root)
    import numpy as np
    from mpi_amd import xmpi
    rehearsal = bool(os.environ.get("XMPI_DEVSIM_LIB"))
    if rehearsal:
        xmpi.LIB_PATH = os.environ["XMPI_DEVSIM_LIB"]
    c = xmpi.Comm(rank, size, -1, key)
    KiB, MiB = 1 << 10, 1 << 20
    maxblock = int(os.environ.get("VBENCH_MAXBLOCK", 32 * MiB))
    blocks = [b for b in (1 * KiB, 64 * KiB, 1 * MiB, 32 * MiB) if b <= maxblock]
    send, recv = c.alloc(size * maxblock), c.alloc(size * maxblock)
    c.fill(send, size * maxblock // 4, xmpi.F32, xmpi.PAT_SIGNED, 7 + rank)
    c.memset(recv, 0, size * maxblock)
    u64 = lambda x: np.asarray(x, dtype=np.uint64)

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
        return (3, 1) if rehearsal else (300, 20) if b <= 64 * KiB else (60, 5) if b <= 4 * MiB else (12, 3)

    def v_call(counts_out, counts_in):
        """packed both ways; counts in f32 elements"""
        sd = [sum(counts_out[:j]) for j in range(size)]
        rd = [sum(counts_in[:r]) for r in range(size)]
        a = (u64(counts_out), u64(sd), u64(counts_in), u64(rd))
        se, re_ = sum(counts_out), sum(counts_in)
        return lambda: c.alltoallv(send, se, a[0], a[1], recv, re_, a[2], a[3], xmpi.F32, xmpi.ALGO_ZCOPY)

    rows = []
    v0 = c.get_param("dsync_v_launches")
    for rep in range(reps):
        for b in blocks:
            n = b // 4
            it, warm = iters_for(b)
            for name, call in (("alltoall zcopy", lambda: c.alltoall(send, recv, n, xmpi.F32, xmpi.ALGO_ZCOPY)),
                               ("alltoallv equal", v_call([n] * size, [n] * size))):
                rows.append({"plan": "equal", "what": name, "block_bytes": b, "ranks": size, "rep": rep, "us_per_call": round(timed(call, it, warm), 2), "iters": it})
        # one block (rank 0 -> rank size - 1) 64 x the others; the equal matrix of the same total bytes
        small = min(128 * KiB, maxblock // 64) // 4
        cnt = lambda f, t: 64 * small if (f, t) == (0, size - 1) else small
        total = (size * size - 1 + 64) * small
        eq = total // (size * size)
        it, warm = iters_for(64 * small * 4)
        for name, call in (("alltoallv skewed", v_call([cnt(rank, j) for j in range(size)], [cnt(r, rank) for r in range(size)])),
                           ("alltoallv equal total", v_call([eq] * size, [eq] * size))):
            rows.append({"plan": "skewed", "what": name, "block_bytes": small * 4, "total_bytes": total * 4, "ranks": size, "rep": rep,
                         "us_per_call": round(timed(call, it, warm), 2), "iters": it})
    rows.append({"dsync_v_launches": c.get_param("dsync_v_launches") - v0, "dsync": c.get_param("dsync"), "ranks": size})
    c.barrier()
    if rank == 0:
        for r in rows:
            print(json.dumps(r))
    c.finalize()


if __name__ == "__main__":
    worker() if sys.argv[1] == "--worker" else launcher()
