"""tests/devsim (TEST INFRASTRUCTURE): with this directory on PYTHONPATH and XMPI_DEVSIM_LIB set, every Python process -- bench.py as
the driver launches it, the `--probe` children it starts, torch.distributed.run's workers -- binds mpi_amd.xmpi to the CPU stand-in
instead of libxmpi.so.  The product has no such switch: this file is the switch, and only the CPU suite puts it on the path.

A sitecustomize, not a usercustomize: Python skips the latter when user site-packages are disabled (PYTHONNOUSERSITE, `-s`), as
they are where the suite runs with nothing but the checkout.  It shadows the interpreter's own sitecustomize, which it runs first."""
import os
import sys


def _run_shadowed():
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    for d in sys.path:
        d = os.path.abspath(d or os.curdir)
        f = os.path.join(d, "sitecustomize.py")
        if d != here and os.path.isfile(f):
            spec = importlib.util.spec_from_file_location("_shadowed_sitecustomize", f)
            spec.loader.exec_module(importlib.util.module_from_spec(spec))
            return


try:
    _run_shadowed()
except Exception:  # noqa: BLE001  (what the interpreter's own hook does is not this file's business)
    pass

if os.environ.get("XMPI_DEVSIM_LIB"):
    _root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    if _root not in sys.path:
        sys.path.insert(0, _root)
    from mpi_amd import xmpi as _xmpi
    _xmpi.LIB_PATH = os.environ["XMPI_DEVSIM_LIB"]
