#!/usr/bin/env python3
"""Search for a board whose ONLY failing unit is a box (tests/check_inputs.py SINGLE_BOX).

The checker's rule per unit is `sum == 45 and 9 distinct`.  A board in which 26 units pass and box (0,0)
fails lets the tests notice a checker that leaves out one box's test; the row/column twin is known
(check_inputs.SINGLE_ROW).  All 26 passing units cover every cell, so every value is in 0..17, and the
nine box sums add up to 9 * 45, so the failing box has sum 45 and a repeated value w.  Up to row and
column permutations inside band 0 / stack 0 the two equal cells are (0,0) and (1,1).

Formulation (scipy.optimize.milp, HiGHS): binaries x[cell, value], one value per cell; per passing unit
each value at most once and sum(value * x) = 45; x[(0,0), w] = x[(1,1), w] = 1.  One process per w in
0..17, at most 16 at a time, each bounded by --seconds of wall time; the objective is a seeded random
weight vector (any feasible point will do; the seed varies the branch order).  CPU only.

    python tools/find_check_cases.py --seconds 300 --seed 1

prints, per w, `infeasible`, `time limit` or the board, verified by plain Python.  The tests never run
this; a found board is pasted into check_inputs.SINGLE_BOX by hand.  Outcome: DESIGN.md, "checker pin".
"""
import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NV = 18


def solve_for(args):
    w, seconds, seed = args
    from scipy.optimize import milp, LinearConstraint, Bounds
    from scipy.sparse import lil_matrix
    import check_inputs as I
    units = I.unit_cells()
    passing = [u for u in range(27) if u != 18]
    nvar = 81 * NV
    rows = 81 + len(passing) * (NV + 1)
    a = lil_matrix((rows, nvar))
    lo, hi = np.zeros(rows), np.zeros(rows)
    r = 0
    for c in range(81):                                   # one value per cell
        a[r, c * NV:(c + 1) * NV] = 1
        lo[r] = hi[r] = 1
        r += 1
    for u in passing:
        for v in range(NV):                               # each value at most once
            for c in units[u]:
                a[r, c * NV + v] = 1
            hi[r] = 1
            r += 1
        for c in units[u]:                                # sum 45
            a[r, c * NV:(c + 1) * NV] = np.arange(NV)
        lo[r] = hi[r] = 45
        r += 1
    lb, ub = np.zeros(nvar), np.ones(nvar)
    lb[0 * NV + w] = lb[10 * NV + w] = 1
    cost = np.random.default_rng([seed, w]).random(nvar)
    res = milp(cost, constraints=LinearConstraint(a.tocsr(), lo, hi), integrality=np.ones(nvar), bounds=Bounds(lb, ub),
               options={"time_limit": float(seconds), "mip_rel_gap": 1.0})
    if res.x is None:
        return w, ("infeasible" if res.status == 2 else f"time limit (status {res.status})"), None
    board = np.rint(res.x).reshape(81, NV).argmax(axis=1)
    ok = I.failing_units(board) == [18]
    return w, "found" if ok else "solver point fails the plain check", board.tolist()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=300, help="wall time per value of w")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--values", type=int, nargs="*", default=list(range(NV)), help="the repeated values w to try")
    a = ap.parse_args()
    with mp.Pool(min(16, a.threads)) as pool:
        for w, what, board in pool.imap_unordered(solve_for, [(w, a.seconds, a.seed) for w in a.values]):
            print(f"w={w}: {what}", flush=True)
            if board is not None:
                print(" / ".join(" ".join(str(v) for v in board[9 * i:9 * i + 9]) for i in range(9)), flush=True)


if __name__ == "__main__":
    main()
