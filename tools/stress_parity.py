#!/usr/bin/env python3
"""Randomised parity sweep (GPU box): resident pair pipeline vs the CPU oracle chain on random image sizes (strip and tile
boundaries of the streaming kernels), block sizes 1..45, corner budgets and every odd window size; everything compared bit for bit.
The cases come from tests/param_ranges.py, which tests/test_gpu_param_ranges.py runs at a bounded size.
  python tools/stress_parity.py [cases] [seed]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    load_package()
    import of_amd.ofk as ofk
    import param_ranges as pr
    t0 = time.time()
    bad = 0
    for c in pr.sweep_cases(n_cases, seed):
        failure = pr.run_sweep_case(c, ofk)
        bad += failure is not None
        print(failure or f"{pr.describe(c)}: ok", flush=True)
    print(f"{n_cases} cases, {bad} failures, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
