"""python scripts/personal_bench.py <plan> <ranks> <reps> <out file> [tree root]: one process per rank on the visible GPU(s), rank 0's
rows appended to the file.  tree root: the checkout whose mpi_amd is measured (default: this one) -- a build of the parent commit
for the `parent` plan.  Plans: scripts/personal_bench_worker.py."""
import os, subprocess, sys, uuid
plan, size, reps, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
here = os.path.dirname(os.path.abspath(__file__))
root = sys.argv[5] if len(sys.argv) > 5 else os.path.dirname(here)
key = f"pb{os.getpid()}-{uuid.uuid4().hex[:6]}"
e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", XMPI_TIMEOUT_S="60")
ps = [subprocess.Popen([sys.executable, os.path.join(here, "personal_bench_worker.py"), root, str(r), str(size), key, plan, reps], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(size)]
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
