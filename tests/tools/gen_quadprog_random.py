#!/usr/bin/env python3
"""Generate tests/golden/quadprog_random.npz: the REFERENCE's own compiled QuadProg++ (oracle/_ref) on the 300 seeded
random QPs of tests/test_oracle_quadprog.py::random_problems (2..12 variables, 0..20 inequalities, an all-zero or random
equality column or none), so that the test pins the oracle on them where the reference tree is absent.

Runs only in the build container (needs oracle/_ref: make -C oracle ref).  Stored per problem: status, x (zero-padded to
12), f, and the sum of every input entry (the test checks it regenerated the same problems).  Nothing of the reference's
source text is stored.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
from test_oracle_quadprog import input_sum, random_problems  # noqa: E402


def main():
    assert O.ref_lib() is not None, "build oracle/_ref first: make -C oracle ref"
    probs = list(random_problems())
    x, f = np.zeros((len(probs), 12)), np.zeros(len(probs))
    st, sums = np.zeros(len(probs), dtype=np.int32), np.zeros(len(probs))
    for k, (G, g0, CE, CI, ci0) in enumerate(probs):
        r = O.ref_solve_quadprog(G, g0, CE, np.zeros(CE.shape[1]), CI, ci0)
        x[k, :len(g0)], f[k], st[k], sums[k] = r["x"], r["f"], r["status"], input_sum(G, g0, CE, CI, ci0)
    path = os.path.join(ROOT, "tests", "golden", "quadprog_random.npz")
    np.savez_compressed(path, x=x, f=f, status=st, input_sum=sums)
    print(path, "%d problems, %d solved" % (len(probs), int((st == 0).sum())))


if __name__ == "__main__":
    main()
