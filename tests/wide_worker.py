"""One rank of an XMPI_SUM_WIDE scenario (tests/wide_scenarios.py); tests/personal_worker.py wired to that module:
  python tests/wide_worker.py <scenario> <rank> <size> <key> [json]      one process per rank
  python tests/wide_worker.py --threads <scenario> <size> [json]         every rank a thread of this process"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import personal_worker, wide_scenarios
    sys.modules["tests.personal_scenarios"] = wide_scenarios  # (what personal_worker's `from tests import personal_scenarios` finds)
    import tests
    tests.personal_scenarios = wide_scenarios
    personal_worker.main()


if __name__ == "__main__":
    main()
