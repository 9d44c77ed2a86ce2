"""One rank of an XMPI_BAND / _BOR / _BXOR scenario (tests/bitop_scenarios.py); tests/personal_worker.py wired to that module:
  python tests/bitop_worker.py <scenario> <rank> <size> <key> [json]      one process per rank
  python tests/bitop_worker.py --threads <scenario> <size> [json]         every rank a thread of this process"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import personal_worker, bitop_scenarios
    sys.modules["tests.personal_scenarios"] = bitop_scenarios  # (what personal_worker's `from tests import personal_scenarios` finds)
    import tests
    tests.personal_scenarios = bitop_scenarios
    personal_worker.main()


if __name__ == "__main__":
    main()
