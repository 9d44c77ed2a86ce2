"""xmpi_set_param, xmpi_get_param and the environment, held to what the commit before the one table (mpi_amd/csrc/params.cpp)
answered: tests/golden/params_parent.json was recorded from that commit by `python tests/test_params.py --record` (one rank on one
virtual device of tests/devsim, no GPU), and the same probes are replayed here.  What may differ is listed below, each with its
reason, and computed from the table (xmpi_param_info) -- never from the setter under test."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "params_parent.json")

VALUES = [-2, -1, 0, 1, 2, 3, 32, 33, 4095, 4096, 4097, 32768, 32769, 1 << 20, 1 << 40]
STRINGS = ["unset", "-1", "0", "1", "3", "70000", "junk"]
# beside the names INTEGRATION.md section 5 lists as settable: a cell of each tuned table, a name nobody knows, a read-only one
EXTRA_SET = ["tune_algo_0_0", "tune_split_3_7", "tune_unroll_1_2", "no_such_knob", "dsync_launches"]
EXTRA_GET = ["lanes", "fifo_depth", "slot_bytes", "p2p_slot_bytes", "watchdog_ms", "selfcheck"]
# every variable of the table, set to the same string at once (the process-wide ones that are read where they are used stay out)
ENV_VARS = ["XMPI_TIMEOUT_S", "XMPI_WATCHDOG_MS", "XMPI_SELFCHECK", "XMPI_ZERO_COPY", "XMPI_DSYNC", "XMPI_HOST_LANES", "XMPI_LL_BYTES",
            "XMPI_AGENT_LL", "XMPI_AGENT_LL_BYTES", "XMPI_LL_AGENT_US", "XMPI_P2P_AGENT_US", "XMPI_P2P_KERNEL_ACK", "XMPI_P2P_DIRECT_BYTES",
            "XMPI_P2P_GRID_CAP", "XMPI_DSYNC_SPLIT_BYTES", "XMPI_DSYNC_UNROLL", "XMPI_DSYNC_TILES", "XMPI_DSYNC_GRID", "XMPI_SCHED_CHANNELS",
            "XMPI_SCHED_GRID", "XMPI_TREE_PIECE_BYTES", "XMPI_ZC_BCAST_PUSH_BYTES", "XMPI_BODY_SYS", "XMPI_XCD_CHECK", "XMPI_CHANNELS",
            "XMPI_PIECE_BYTES", "XMPI_COPY_ENGINE", "XMPI_BATCH_COPIES", "XMPI_ONESHOT_BYTES", "XMPI_ZC_GROUP_LAUNCH", "XMPI_SHARED_STREAM",
            "XMPI_LANES", "XMPI_FIFO_DEPTH", "XMPI_SLOT_BYTES", "XMPI_P2P_DEPTH", "XMPI_P2P_SLOT_BYTES", "XMPI_KERNEL_MODE", "XMPI_GRID_CAP",
            "XMPI_TEST_EPOCH_BASE", "XMPI_TEST_P2P_SEQ0"]  # (tests only; one rank never meets on the device: nothing to see)

# ---- what may differ from the parent, and why ---------------------------------------------------------------------------------------
# xmpi_get_param answered -1 for these on the parent (they could only be set); they are rows like any other now
ONCE_WRITE_ONLY = ["prof_every", "batch_copies", "oneshot_bytes", "zc_bcast_push_bytes", "zc_group_launch"]
# the parent took these raw from the environment while its setter clamped them (XMPI_SELFCHECK has no setter; any value but 0 and the
# -1 of "decide later" ran the check, as 1 does): a row has one range, and both paths apply it
ENV_WAS_UNCLAMPED = ["channels", "piece_bytes", "copy_engine", "dsync_unroll", "body_sys", "ll_bytes", "selfcheck"]
# the parent's setter stored a negative limit as it came, its environment path max(0, .): the row carries the latter
SETTER_WAS_UNCLAMPED = ["timeout_s"]

WRITABLE, BOOLEAN, LAYOUT_DEFAULT, READ_ONLY, PATTERN, ENV_AUTO = 1, 2, 4, 8, 16, 32


def settable_names():
    from tests.test_abi import knob_rows
    return sorted({n for _, names, _ in knob_rows() for n in names}) + EXTRA_SET


# ---- one rank on one virtual device, in a process of its own ------------------------------------------------------------------------
def worker(kind):
    from mpi_amd import xmpi
    xmpi.LIB_PATH = os.environ["XMPI_DEVSIM_LIB"]
    L = xmpi.lib()
    names = json.loads(sys.argv[3])
    try:
        comm = xmpi.Comm(0, 1, -1, f"params{os.getpid()}")
    except xmpi.XmpiError as e:  # (an all-at-once combination that cannot initialise: that is the outcome)
        print(json.dumps({"init": e.code}))
        return
    h, out = comm.handle, {"init": 0}
    if kind == "env":
        out["get"] = {n: L.xmpi_get_param(h, n.encode()) for n in names}
    else:
        keep = {n: L.xmpi_get_param(h, n.encode()) for n in ("kernel_mode", "grid_cap")}  # process-wide
        out["set"] = {}
        for n in names:
            out["set"][n] = [[L.xmpi_set_param(h, n.encode(), v), L.xmpi_get_param(h, n.encode())] for v in VALUES]
        for n, v in keep.items():
            L.xmpi_set_param(h, n.encode(), v)
        L.xmpi_set_param(h, b"timeout_s", 0)
    comm.finalize()
    print(json.dumps(out))


def run_worker(root, lib, kind, names, string="unset"):
    env = {k: v for k, v in os.environ.items() if not k.startswith("XMPI_")}
    env.update(XMPI_DEVSIM_LIB=lib, DEVSIM_DEVICES="1")
    if string != "unset":
        env.update({v: string for v in ENV_VARS})
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", kind, json.dumps(names)], cwd=root, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        out, err = p.communicate(timeout=120)
    finally:
        p.kill()
        for f in glob.glob(f"/dev/shm/devsim.{p.pid}.*") + glob.glob(f"/dev/shm/xmpi-*-params{p.pid}*"):
            os.unlink(f)
    assert p.returncode == 0, f"{kind} probe ({string}) exited {p.returncode}\n{out}\n{err[-3000:]}"
    return json.loads(out.strip().splitlines()[-1])


def record(root, commit):
    """run by hand on a checkout of the commit BEFORE the table: python tests/test_params.py --record <that checkout> <its hash>"""
    subprocess.run([sys.executable, "-m", "tests.devsim.build"], cwd=root, check=True)
    lib = os.path.join(root, "tests", "devsim", "libxmpi_devsim.so")
    names = settable_names()
    gold = {"parent": commit, "values": VALUES, "set": run_worker(root, lib, "set", names)["set"], "env": {}}
    for s in STRINGS:
        gold["env"][s] = run_worker(root, lib, "env", names[:-len(EXTRA_SET)] + EXTRA_GET, s)
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")


# ---- the replay ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def devsim_lib():
    from tests.devsim import build
    return build.build_lib()


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def table():
    """name -> (environment variable, default, lo, hi, flags) of every row of the library's table"""
    import ctypes as C
    from mpi_amd import xmpi
    L, rows, i = xmpi.lib(), {}, 0
    while True:
        name, env, d, lo, hi, fl = C.c_char_p(), C.c_char_p(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        if L.xmpi_param_info(i, C.byref(name), C.byref(env), C.byref(d), C.byref(lo), C.byref(hi), C.byref(fl)) != xmpi.OK:
            return rows
        if name.value or env.value:  # (a row without a name: a variable of the window layout that nothing reads back)
            rows[(name.value or env.value).decode()] = (env.value.decode() if env.value else None, d.value, lo.value, hi.value, fl.value)
        i += 1


def in_range(row, v):
    """what the row makes of v on the way in from xmpi_set_param"""
    _, _, lo, hi, fl = row
    return (1 if v else 0) if fl & BOOLEAN else min(max(v, lo), hi)


def from_env(row, string):
    """... and of a string on the way in from the environment (the C library's strtol with base 0; no digits: the default);
    None: the value is decided later, where the job's layout is known"""
    _, dflt, lo, _, fl = row
    try:
        v = int(string, 0)
    except ValueError:
        v = dflt if not fl & LAYOUT_DEFAULT else None
    if v is None or (fl & ENV_AUTO and v < lo):
        return None
    return in_range(row, v)


def test_the_probes_cover_the_table(table):
    envs = {r[0] for r in table.values() if r[0]}
    assert envs <= set(ENV_VARS), f"a table row's variable the environment probes leave out: {sorted(envs - set(ENV_VARS))}"
    for n in ONCE_WRITE_ONLY + ENV_WAS_UNCLAMPED + SETTER_WAS_UNCLAMPED:
        assert n in table, n


def test_the_setter_answers_what_the_parent_answered(devsim_lib, gold, table):
    """every settable name of section 5 and five more, each at 15 values: the return code of xmpi_set_param and what
    xmpi_get_param says afterwards"""
    assert gold["values"] == VALUES
    names = settable_names()
    assert sorted(gold["set"]) == sorted(names), "the names the golden file was recorded for are not section 5's"
    now = run_worker(ROOT, devsim_lib, "set", names)["set"]
    bad = []
    for n in names:
        for v, was, got in zip(VALUES, gold["set"][n], now[n]):
            want = list(was)
            if n in ONCE_WRITE_ONLY:
                assert was == [0, -1], (n, v, was)  # (accepted, and unreadable)
                want = [0, in_range(table[n], v)]
            elif n in SETTER_WAS_UNCLAMPED and not table[n][2] <= v <= table[n][3]:
                want = [0, in_range(table[n], v)]
            if got != want:
                bad.append(f"{n} = {v}: (rc, value) = {got}, expected {want} (the parent: {was})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("string", STRINGS)
def test_the_environment_gives_what_it_gave_the_parent(devsim_lib, gold, table, string):
    """every variable of the table set to `string` at once in a fresh process: what xmpi_get_param answers after xmpi_init"""
    names = settable_names()[:-len(EXTRA_SET)] + EXTRA_GET
    was, now = gold["env"][string], run_worker(ROOT, devsim_lib, "env", names, string)
    assert now["init"] == was["init"]
    if was["init"] != 0:
        return
    assert sorted(was["get"]) == sorted(names)
    bad = []
    for n in names:
        want = was["get"][n]
        s = string if table[n][0] and string != "unset" else "junk"  # (no variable, or not set: the default)
        if n in ONCE_WRITE_ONLY:
            assert want == -1, (n, want)
            want = from_env(table[n], s)
        elif n in ENV_WAS_UNCLAMPED:
            v = from_env(table[n], s)
            try:
                if v is not None and v != int(s, 0):  # outside the row's range: the row's answer, whatever the parent's was
                    want = v
            except ValueError:
                pass
        if now["get"][n] != want:
            bad.append(f"{n} with {table[n][0]}={string}: {now['get'][n]}, expected {want} (the parent: {was['get'][n]})")
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    if sys.argv[1] == "--worker":  # (started in the checkout whose library it probes)
        sys.path.insert(0, os.getcwd())
        worker(sys.argv[2])
    elif sys.argv[1] == "--record":
        sys.path.insert(0, ROOT)
        record(os.path.abspath(sys.argv[2]), sys.argv[3])
