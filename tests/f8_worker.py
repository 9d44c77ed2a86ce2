"""One rank of an XMPI_F8E4M3 / XMPI_F8E5M2 scenario (tests/f8_scenarios.py); tests/personal_worker.py wired to that module:
  python tests/f8_worker.py <scenario> <rank> <size> <key> [json]      one process per rank
  python tests/f8_worker.py --threads <scenario> <size> [json]         every rank a thread of this process"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import f8_scenarios, personal_worker
    sys.modules["tests.personal_scenarios"] = f8_scenarios  # (what personal_worker's `from tests import personal_scenarios` finds)
    import tests
    tests.personal_scenarios = f8_scenarios
    personal_worker.main()


if __name__ == "__main__":
    main()
