"""One rank of an epoch-edge scenario (tests/epoch_scenarios.py); tests/personal_worker.py wired to that module:
  python tests/epoch_worker.py <scenario> <rank> <size> <key> [json]      one process per rank
  python tests/epoch_worker.py --threads <scenario> <size> [json]         every rank a thread of this process"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import personal_worker, epoch_scenarios
    sys.modules["tests.personal_scenarios"] = epoch_scenarios  # (what personal_worker's `from tests import personal_scenarios` finds)
    import tests
    tests.personal_scenarios = epoch_scenarios
    personal_worker.main()


if __name__ == "__main__":
    main()
