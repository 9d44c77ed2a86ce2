"""Launch the ranks of a tests/f8_scenarios.py scenario and wait: tests/personal_harness.py with tests/f8_worker.py for the worker
(personal_harness names its worker in a module variable, read when a job starts)."""
import os
import threading

from tests import personal_harness as ph

WORKER = os.path.join(ph.ROOT, "tests", "f8_worker.py")
_lock = threading.Lock()


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
