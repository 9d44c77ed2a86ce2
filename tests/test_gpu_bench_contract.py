"""bench.py prints exactly one JSON line with the keys the driver reads, and smoke() passes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


def test_bench_json_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--size-mib", "16",
                        "--full", "--no-extras", "--cpu-count", "65536"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().split("\n")[-1] == lines[0]
    assert len(lines[0]) < 4096, len(lines[0])  # the driver's parser must see the whole line (round 2's 20 KB line was lost)
    d = json.loads(lines[0])
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "GB/s" and d["value"] > 0 and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["dtype"] == "f32" and "workload" in d["config"] and "model" not in d["config"]
    # the value IS BASELINE.json's metric: algbw = bytes per rank / time per step (GB = 1e9 B), no rank multiplier
    assert "algbw" in d["metric"] and "aggregate" not in d["metric"]
    assert abs(d["value"] - d["config"]["bytes_per_rank"] / d["ms_per_step"] / 1e6) < 1e-6 * d["value"]
    r = d["config"]["ranks"]
    assert abs(d["busbw_GBps"] - d["value"] * 2 * (r - 1) / r) < 1e-6 * d["value"]
    assert "xGMI" not in d["config"]["transport"]  # eight ranks on one GPU never cross a link
    ro = d["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-9 and ro["launches"] > 0
    # box against code: the spread of the sampled launches, the fold against what a streaming kernel achieves on this part, and against
    # THIS box on THESE buffers -- the fold's access pattern without the arithmetic, run right behind the timed region
    assert 0 < ro["kernel_us_min"] <= ro["avg_launch_us"] <= ro["kernel_us_max"]
    assert abs(ro["frac_of_achievable"] - ro["achieved"] / 6300.0) < 1e-9
    assert ro["box_copy_us"] > 0 and abs(ro["frac_of_box"] - ro["box_copy_us"] / ro["avg_launch_us"]) < 1e-9
    assert ro["frac_of_box"] >= 0.9, ro  # (16 MiB per rank lives in the caches; the 256 MiB line is held to 0.97 by scripts/r06_profile.sh's reader)
    # HBM traffic of the dominant kernel MEASURED IN THIS RUN where rocprofv3 is installed (two --pmc child passes of the same workload,
    # separate, --kernel-trace only; the guide's gfx950 correction) -- the committed profile only as the fallback, and the line says which
    import shutil
    if shutil.which("rocprofv3"):
        assert ro["traffic_from_profile"] is False and ro["traffic"] > 0 and ro["traffic_over_algorithmic"] > 0, ro
    cb = d["cpu_baseline"]
    assert sorted(cb["by_ranks"]) == ["2", "4", "8"] and all(v["algbw_GBps"] > 0 for v in cb["by_ranks"].values()), cb
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert abs(cb["value"] - 65536 * 4 / cb["seconds_per_allreduce"] / 1e9) < 1e-6 * cb["value"]  # algbw too, not x ranks
    assert d["parity"]["checked"] and d["parity"]["ok"] and d["parity"]["bit_identical"] and "whole buffer" in d["parity"]["coverage"]
    assert d["parity_failures"] == 0
    # the same workload with one OS process per rank: the kernels of the production layout, ranks meeting on the device
    rp = d["roofline_production"]
    assert rp["exact"] is True and "device" in rp["layout"] and rp["ms_per_step"] > 0 and rp["avg_launch_us"] > 0, rp
    assert 0 < rp["frac"] < 1.2 and abs(rp["frac"] - rp["achieved_all_ranks"] / rp["peak"]) < 1e-9
    assert rp["fused_ms_per_step"] > 0 and rp["split_ms_per_step"] > 0
    # ... whose algbw is a first-class figure of the line (the layout a real node runs), exact like `value`
    assert d["value_production_exact"] is True
    assert abs(d["value_production"] - d["config"]["bytes_per_rank"] / rp["ms_per_step"] / 1e6) < 1e-3 * d["value_production"]
    with open(os.path.join(ROOT, d["extras_file"])) as f:
        slots = json.load(f)["timed_buffer_slots"]
    assert len(slots) == r and all(0 <= v["send"] < 16 and 0 <= v["recv"] < 16 for v in slots.values())
    assert os.path.exists(os.path.join(ROOT, d["extras_file"]))


def test_bench_extras_tables():
    """the untimed extras at a small size (bench_extras.json): busbw against message size at 1 / 2 / 4 / 8 ranks, cfg 3 at its
    4 ranks, and the one-process-per-rank sweep (ranks meeting on the device)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--size-mib", "16",
                        "--full", "--no-cpu", "--no-production", "--no-pmc"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("{")][0]
    assert len(line) < 6000
    d = json.loads(line)
    assert set(d["busbw_at_size"]) == {"1", "2", "4", "8"} and all(v["bytes"] == 16 << 20 for v in d["busbw_at_size"].values())
    with open(os.path.join(ROOT, d["extras_file"])) as f:
        ex = json.load(f)["extras"]
    rows = ex["busbw_table"]["rows"]
    assert {x["ranks"] for x in rows} == {1, 2, 4, 8}
    for x in rows:
        assert x["us"] > 0 and abs(x["busbw_GBps"] - x["algbw_GBps"] * 2 * (x["ranks"] - 1) / x["ranks"]) < 1e-9
    assert {x["bytes"] for x in rows if x["ranks"] == 8} == {1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24}
    c3 = ex["cfg3_allgather_i64_16MiB_4ranks"]
    assert c3["ranks"] == 4 and c3["auto"]["ms"] > 0 and c3["ring"]["ms"] > 0
    # the headline's call on HOST slices (what a caller of the reference passes): buffers up and results down over PCIe inside the call --
    # the PCIe-inclusive rate beside `value`, never as `value`; right to the line's tolerance, and far below the HBM-resident figure
    hs, pi = ex["host_slices_allreduce"], d["pcie_inclusive"]
    assert hs["parity_ok"] is True and hs["ranks"] == 8 and hs["bytes_per_rank"] == 16 << 20 and hs["max_abs_err"] <= 8e-6, hs
    assert pi["parity_ok"] is True and abs(pi["algbw_GBps"] - hs["algbw_GBps"]) < 0.01 and 0 < hs["algbw_GBps"] < d["value"], (pi, d["value"])
    mp = ex["multiprocess_sweep"]  # eight PROCESSES on this GPU, meeting on the device
    assert mp["ranks"] == 8 and mp["exact"] is True and "device" in mp["meet"], mp
    assert mp["rows"][0]["bytes"] == 1024 and mp["rows"][0]["queued_us"] < 1000, mp["rows"][0]


@pytest.mark.parametrize("nproc", [2, 4, 8])
def test_bench_multi_process_launch_rehearsal(nproc):
    """the driver's SCALE launch (torch.distributed.run, one process per GPU) rehearsed on this box's one GPU: the line
    must come out whole whatever N is (N = 8: one rank per process, ranks meet on the device, the library tunes itself)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, XMPI_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "3", "--warmup", "1",
           "--size-mib", "16", "--full", "--no-extras", "--no-probe"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("{\"metric\"")]
    assert len(lines) == 1 and len(lines[0]) < 6000
    d = json.loads(lines[0])
    assert d["n_gpus"] == nproc and d["value"] > 0 and d["parity"]["ok"] and d["parity_failures"] == 0
    assert d["config"]["ranks"] == 8 and d["config"]["ranks_per_gpu"] == 8 // nproc
    if nproc == 8:
        assert d["ranks_meet"].startswith("on the device") and d["config"]["schedule_by"].startswith("xmpi_tune")
        assert d["roofline"]["kernel"].startswith("dsync_")


def test_bench_probe_rules_out_a_schedule():
    """a multi-process run first tries EVERY schedule the library may choose in jobs of its own (child processes); one that
    does not work on the machine (here: forced) is left out of the library's tuning instead of killing the run"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, XMPI_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", XMPI_BENCH_FAIL_RING="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1",
           "--size-mib", "16", "--full", "--no-extras"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.strip().split("\n") if ln.startswith("{\"metric\"")][0])
    assert d["zero_copy_probe"].startswith("ok") and d["parity"]["ok"]
    with open(os.path.join(ROOT, d["extras_file"])) as f:
        tune = json.load(f)["autotune"]
    assert tune["probe_ok"] == ["fused", "rhd", "rhd_push", "ring_push", "split", "zpush"], tune
    assert 1 not in tune["table_algo"]  # XMPI_ALGO_RING never made it into the table


def test_cfg3_and_cfg5_in_the_production_layout():
    """BASELINE cfg 3 (allgather int64, 4 ranks, ring) and cfg 5 (fp16 allreduce, halving vs ring) with one process per rank:
    ring and halving are the stepped kernels; every result bit-exact (cfg 5: exactly summable inputs)"""
    env = dict(os.environ, XMPI_TIMEOUT_S="60", XMPI_NGPUS="1", XMPI_BASEPORT="7480")
    run = os.path.join(ROOT, "mpi_amd", "bin", "xmpirun")
    r = subprocess.run([run, "4", os.path.join(ROOT, "mpi_amd", "bin", "cfg3_allgather"), "2097152", "5"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(r.stdout.strip().split("\n")[-1])
    assert d["exact"] is True and d["ranks"] == 4 and d["bytes_per_rank"] == 16 << 20 and "stepped kernel" in d["meet"]
    assert d["ring"]["bit_exact_and_in_place"] and d["auto"]["bit_exact_and_in_place"] and d["ring"]["blocking_us"] > 0
    r = subprocess.run([run, "8", os.path.join(ROOT, "mpi_amd", "bin", "cfg5_sweep"), str(16 << 20), "3"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=dict(env, XMPI_BASEPORT="7520"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(r.stdout.strip().split("\n")[-1])
    assert d["all_bit_identical"] is True and [x["bytes"] for x in d["rows"]] == [1 << 20, 4 << 20, 16 << 20]
    assert all(x[k]["bit_identical_to_rank_order"] and x[k]["us"] > 0 for x in d["rows"] for k in ("ring", "rhd", "auto"))


def test_coll_sweep_one_process_per_rank():
    """examples/coll_sweep under the launcher: 4 processes, blocking and stream-queued allreduce, exact results"""
    env = dict(os.environ, XMPI_TIMEOUT_S="60", XMPI_NGPUS="1", XMPI_BASEPORT="7400")
    r = subprocess.run([os.path.join(ROOT, "mpi_amd", "bin", "xmpirun"), "4", os.path.join(ROOT, "mpi_amd", "bin", "coll_sweep"),
                        str(1 << 20), "50"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(r.stdout.strip().split("\n")[-1])
    assert d["ranks"] == 4 and d["exact"] is True and "device" in d["meet"]
    assert [x["bytes"] for x in d["rows"]] == [1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20]
    assert all(x["blocking_us"] > 0 and x["queued_us"] > 0 for x in d["rows"])


def test_smoke_entry():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "__graft_entry__.py"), "--smoke"], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "smoke ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
