"""Regenerates tests/golden/attitude_growth.npz: the growth of a 1e-10 perturbation over the real case's 25 rows under the aided
attitude rule (tests/attitude_cases.py, measure_growth), measured on the host.
usage: python tests/golden/attitude_growth.py"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TESTS)
import conftest  # noqa: E402,F401  (it puts the repository on the path)
import attitude_cases as A  # noqa: E402

if __name__ == "__main__":
    g = A.measure_growth()
    np.savez(A.GROWTH_NPZ, growth=np.float64(g), eps=np.float64(1e-10))
    print("growth over the real case's 25 rows under the aided rule", g)
