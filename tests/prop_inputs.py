"""The boards the propagation-pass model tests share (test_prop_model.py on the CPU,
test_gpu_prop32_model.py against the kernel), built once per process."""
import functools

import numpy as np

from distributed_sudoku_solver_amd import synth
from test_gpu_prop32 import edge_boards  # noqa: F401  (the edge batch, as the end-to-end tests build it)

DEFAULT_LC = 5 | (3 << 8)
STEP_CAP = 48     # no compared board may come near the kernel's max_steps = 96
SNAPSHOT_STEPS = (0, 1, 2, 3, 4, 6, 9, 14)     # SDK_OPT_PROP32_TAIL = 64 | step << 8


def wrong_given(boards, seed):
    """Each board with one given changed to a digit that no given of its row, column or box holds: no
    duplicated given (the pass takes the board as exact), and mostly no completion."""
    rng = np.random.default_rng(seed)
    out = boards.copy()
    for b in out:
        for c in rng.permutation(np.flatnonzero(b)):
            r, k = divmod(int(c), 9)
            box = b.reshape(9, 9)[3 * (r // 3):3 * (r // 3) + 3, 3 * (k // 3):3 * (k // 3) + 3]
            seen = set(b[9 * r:9 * r + 9].tolist()) | set(b[k::9].tolist()) | set(box.ravel().tolist())
            free = [d for d in range(1, 10) if d not in seen]
            if free:
                b[c] = free[rng.integers(len(free))]
                break
    return out


def broken_boards(n=1000, pool=16384):
    """37-clue boards (the naive oracle stays quick on them) with a wrong given (wrong_given): the
    refuted class, well populated.  A stuck board with a digit closed twice in a unit (refuted at
    handover only) is rare among them, so the model picks every such board of a larger pool and they
    are appended to the first n."""
    import prop_model as M
    p = wrong_given(synth.make_30clue(pool, seed=8, extra=20)[0], seed=1)
    reason = M.propagate_batch(p)[3]
    keep = np.zeros(pool, dtype=bool)
    keep[:n] = True
    keep |= reason == M.R_DUP_CLOSED
    return p[keep]


@functools.lru_cache(maxsize=None)
def named_set(kind):
    """(boards, solutions or None) of a named input set; read-only arrays."""
    if kind == "minimal":
        p, s = synth.make_minimal_sym(1500, seed=5)
    elif kind == "hard":
        p, s, _ = synth.load_hard(1500)
    elif kind == "17clue":
        p, s = synth.make_17clue(1200, seed=3)
    elif kind == "30clue":
        p, s = synth.make_30clue(1000, seed=4)
    elif kind == "edge":
        p, s = edge_boards(1024), None
    elif kind == "broken":
        p, s = broken_boards(), None
    else:
        raise KeyError(kind)
    p = np.ascontiguousarray(p, dtype=np.uint8)
    p.setflags(write=False)
    if s is not None:
        s = np.ascontiguousarray(s, dtype=np.uint8)
        s.setflags(write=False)
    return p, s


@functools.lru_cache(maxsize=None)
def model_of(kind, lc=DEFAULT_LC, handover=True, tail_step=None):
    """The model's (cls, grids, steps, reason) for a named set at a schedule; read-only arrays."""
    import prop_model as M
    first, every = M.schedule(lc)
    res = M.propagate_batch(named_set(kind)[0], first, every, handover, tail_step=tail_step)
    for a in res:
        a.setflags(write=False)
    return res
