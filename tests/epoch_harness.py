"""Launch the ranks of a tests/epoch_scenarios.py scenario and wait: tests/personal_harness.py with tests/epoch_worker.py for the
worker (personal_harness names its worker in a module variable, read when a job starts)."""
import os
import threading

from tests import personal_harness as ph

WORKER = os.path.join(ph.ROOT, "tests", "epoch_worker.py")
_lock = threading.Lock()
SEQ0 = 2 ** 32 - 16  # XMPI_TEST_P2P_SEQ0 of the message-number jobs: a multiple of kP2PBoxes, 40 messages cross 2^32


def env(base=None, seq0=None):
    e = {"XMPI_TIMEOUT_S": "8", "XMPI_SELFCHECK": "0"}  # (xmpi_init's self-check would spend the epochs below the edge)
    if base is not None:
        e["XMPI_TEST_EPOCH_BASE"] = str(base)
    if seq0 is not None:
        e["XMPI_TEST_P2P_SEQ0"] = str(seq0)
    return e


def _with_worker(fn, *a, **kw):
    with _lock:
        old, ph.WORKER = ph.WORKER, WORKER
        try:
            return fn(*a, **kw)
        finally:
            ph.WORKER = old


def run_ranks(scenario, size, args=None, timeout=300.0, env=None):
    return _with_worker(ph.run_ranks, scenario, size, args, timeout, env)


def run_threads(scenario, size, args=None, timeout=300.0, env=None):
    return _with_worker(ph.run_threads, scenario, size, args, timeout, env)
