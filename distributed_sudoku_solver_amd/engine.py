"""SudokuEngine: numpy-level batch API over libsudoku_hip.so.

This is the host side of the drop-in boundary.  Every method
ends in a HIP kernel launched by the C library; nothing here computes a
solution or a verdict.
"""
import ctypes
import numbers
import threading

import numpy as np

from . import _lib as L
from . import synth

ALL_DIGITS_MASK = 0x3FE  # bits 1..9: range(1, 10)
INERT_VALUE = 10         # any given that is never equal to a digit 1..9


# ----------------------------------------------------------------- encoding
def _as_int(v):
    """The reference compares cells with `==` (utils.py:22,36,44,53): 5.0 == 5, True == 1."""
    if isinstance(v, numbers.Integral):
        return int(v)
    if isinstance(v, numbers.Real) and float(v).is_integer():
        return int(v)
    return None


def encode_solve_grid(grid):
    """9x9 (or flat 81) Python grid -> uint8[81] for the solver.

    0 -> empty; a value equal to a digit 1..9 -> that digit; anything else is a
    given that never equals a guess 1..9 (the reference never rejects it) and
    is encoded as the inert value 10."""
    flat = [v for row in grid for v in row] if len(grid) == 9 else list(grid)
    if len(flat) != 81:
        raise ValueError("a Sudoku grid has 81 cells")
    out = np.empty(81, dtype=np.uint8)
    for i, v in enumerate(flat):
        iv = _as_int(v)
        if iv == 0:
            out[i] = 0
        elif iv is not None and 1 <= iv <= 9:
            out[i] = iv
        else:
            out[i] = INERT_VALUE
    return out


CHECK_I64_LIMIT = 1 << 59   # sdk_check_batch_i64: |v| below this keeps a unit's sum exact


def encode_check_grid(grid):
    """9x9 grid -> uint8[81] (every value an integer 0..255) or int64[81] (any integer with
    |v| < 2^59) for the checker: the literal `sum == 45 and len(set) == 9` rule needs the exact
    values (5.0 counts as 5, like the reference's `==`).  Non-integral numbers raise ValueError."""
    flat = [v for row in grid for v in row] if len(grid) == 9 else list(grid)
    if len(flat) != 81:
        raise ValueError("a Sudoku grid has 81 cells")
    vals = []
    for i, v in enumerate(flat):
        iv = _as_int(v)
        if iv is None or not -CHECK_I64_LIMIT < iv < CHECK_I64_LIMIT:
            raise ValueError(f"cell {i} = {v!r}: the HIP checker takes integers with |v| < 2^59")
        vals.append(iv)
    if all(0 <= v <= 255 for v in vals):
        return np.array(vals, dtype=np.uint8)
    return np.array(vals, dtype=np.int64)


def range_to_mask(arr):
    """TASK digit range (a `range` from split_array_in_middle, utils.py:1-9) -> first-cell mask.

    bit d = digit d may be guessed at the lowest empty cell.  Guess 0 is never
    valid in the reference (the empty cell itself holds 0, utils.py:36), so it
    is dropped.  Order matters to the reference (`for guess in arr`), so only
    ascending digit sequences in 0..9 are representable."""
    vals = [_as_int(v) for v in arr]
    if any(v is None or v < 0 or v > 9 for v in vals):
        raise ValueError(f"digit range {arr!r} has values outside 0..9")
    if any(b <= a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"digit range {arr!r} is not strictly ascending")
    m = 0
    for v in vals:
        if v >= 1:
            m |= 1 << v
    return m


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


# ------------------------------------------------------------------- device
class DeviceBuffer:
    """A device allocation owned by an engine context (for resident-input benchmarks)."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        L.check(engine.lib.sdk_dev_alloc(engine.ctx, self.nbytes, ctypes.byref(p)), "sdk_dev_alloc")
        self.ptr = p

    def upload(self, host, offset=0):
        """Copy `host` to this buffer at byte `offset`."""
        host = np.ascontiguousarray(host)
        if offset < 0 or offset + host.nbytes > self.nbytes:
            raise ValueError("upload out of bounds")
        dst = ctypes.c_void_p(self.ptr.value + int(offset))
        L.check(self.engine.lib.sdk_memcpy_h2d(self.engine.ctx, dst, _ptr(host), host.nbytes), "h2d")

    def download(self, host):
        assert host.flags.c_contiguous and host.nbytes <= self.nbytes
        L.check(self.engine.lib.sdk_memcpy_d2h(self.engine.ctx, _ptr(host), self.ptr, host.nbytes), "d2h")
        return host

    def free(self):
        if self.ptr is not None and self.engine.ctx is not None:
            L.check(self.engine.lib.sdk_dev_free(self.engine.ctx, self.ptr), "sdk_dev_free")
        self.ptr = None


class SudokuEngine:
    """One HIP device + stream.  Thread-safe (the C library serialises per context)."""

    def __init__(self, device=0, order=None, node_budget=None, waves_per_cu=None):
        self._tls = threading.local()
        self.lib = L.load()
        ctx = ctypes.c_void_p()
        L.check(self.lib.sdk_create(int(device), ctypes.byref(ctx)), f"sdk_create(device={device})")
        self.ctx = ctx
        self.device = device
        if order is not None:
            self.set_option(L.SDK_OPT_ORDER, order)
        if node_budget is not None:
            self.set_option(L.SDK_OPT_NODE_BUDGET, node_budget)
        if waves_per_cu is not None:
            self.set_option(L.SDK_OPT_WAVES_PER_CU, waves_per_cu)

    @classmethod
    def open_clique(cls, devices):
        """One engine per device of `devices`, joined by ONE RCCL communicator made
        in this process (sdk_comm_init_all = ncclCommInitAll); engine k is rank k.
        Collectives must then be issued from one host thread per engine."""
        lib = L.load()
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        ctxs = (ctypes.c_void_p * len(devices))()
        L.check(lib.sdk_comm_init_all(devs, len(devices), ctxs), f"sdk_comm_init_all({list(devices)})")
        engines = []
        for k, d in enumerate(devices):
            e = cls.__new__(cls)
            e.lib, e.ctx, e.device = lib, ctypes.c_void_p(ctxs[k]), int(d)
            e._tls = threading.local()
            engines.append(e)
        return engines

    # options a forked engine takes over (everything a caller sets that shapes a solve)
    _FORK_OPTIONS = (L.SDK_OPT_ORDER, L.SDK_OPT_NODE_BUDGET, L.SDK_OPT_WAVES_PER_CU, L.SDK_OPT_WORK_COUNTER,
                     L.SDK_OPT_SOLVER, L.SDK_OPT_WAVES_PER_CU2, L.SDK_OPT_SOLVE_CHUNK, L.SDK_OPT_LOCKED,
                     L.SDK_OPT_XCD_HEADS, L.SDK_OPT_DONATE, L.SDK_OPT_DONATE_MODE, L.SDK_OPT_DONATE_MAX,
                     L.SDK_OPT_DONATE_HELPERS, L.SDK_OPT_DONATE_RESUME, L.SDK_OPT_PROP32, L.SDK_OPT_PROP32_LC,
                     L.SDK_OPT_PROP32_MIN, L.SDK_OPT_PROP32_HANDOVER, L.SDK_OPT_PROP32_TAIL, L.SDK_OPT_GEN_CAP)

    def fork(self):
        """A second engine on the same device with its own context and stream (same options):
        its launches never queue behind this one's, and the GPU runs both at once.  A node
        gives its new batches and its long searches one each (node.py)."""
        e = SudokuEngine(self.device)
        for k in self._FORK_OPTIONS:
            e.set_option(k, self.get_option(k))
        return e

    # -------------------------------------------------------------- plumbing
    def close(self):
        if getattr(self, "ctx", None) is not None:
            self.lib.sdk_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key, value):
        L.check(self.lib.sdk_set_option(self.ctx, key, int(value)), "sdk_set_option")

    def get_option(self, key):
        v = ctypes.c_int64()
        L.check(self.lib.sdk_get_option(self.ctx, key, ctypes.byref(v)), "sdk_get_option")
        return v.value

    def synchronize(self):
        L.check(self.lib.sdk_synchronize(self.ctx), "sdk_synchronize")

    def timer_reset(self):
        """Start (or restart) kernel timing: turns SDK_OPT_TIMING on and drops old events."""
        self.set_option(L.SDK_OPT_TIMING, 1)
        L.check(self.lib.sdk_timer_reset(self.ctx), "sdk_timer_reset")

    def timer_stop(self):
        """Stop recording kernel events (the pairs already made are kept for reuse)."""
        self.set_option(L.SDK_OPT_TIMING, 0)

    def timer_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        L.check(self.lib.sdk_timer_read(self.ctx, ctypes.byref(ms), ctypes.byref(n)), "sdk_timer_read")
        return ms.value, n.value

    def debug_p32_list(self, cap):
        """What the last solve's propagation pass left to the search (sdk_debug_p32_list, a
        diagnostic): (count, uint32[k] board indices, uint8[k,81] the grids the search was given),
        k = min(count, cap), in the pass's list order (not deterministic: sort by index).  count is 0
        when the last solve did not run the pass."""
        cap = max(0, int(cap))
        index = np.zeros(max(cap, 1), dtype=np.uint32)
        grids = np.zeros((max(cap, 1), 81), dtype=np.uint8)
        count = ctypes.c_int64()
        L.check(self.lib.sdk_debug_p32_list(self.ctx, _ptr(index), _ptr(grids), cap, ctypes.byref(count)),
                "sdk_debug_p32_list")
        k = min(count.value, cap)
        return count.value, index[:k].copy(), grids[:k].copy()

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # ----------------------------------------------------------- host batch
    def check_batch(self, boards):
        """uint8[n,81] (or int64[n,81]: sdk_check_batch_i64) -> uint8[n] verdict bits
        (SDK_CHECK_OK | SDK_CHECK_RAW_NAMEERROR)."""
        wide = np.asarray(boards).dtype == np.int64
        boards = np.ascontiguousarray(boards, dtype=np.int64 if wide else np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        verdict = np.empty(n, dtype=np.uint8)
        fn = self.lib.sdk_check_batch_i64 if wide else self.lib.sdk_check_batch
        L.check(fn(self.ctx, _ptr(boards), _ptr(verdict), n), "sdk_check_batch_i64" if wide else "sdk_check_batch")
        return verdict

    def solve_batch(self, boards, masks=None, want_work=False, budget=None, donate=None):
        """uint8[n,81] (+ optional uint16[n] first-cell masks) -> (out uint8[n,81], status int8[n], work).

        budget: search nodes per board for this call (0 = unlimited), None = the context's
        SDK_OPT_NODE_BUDGET.  A board that runs out is SDK_BUDGET_HIT.
        donate: SDK_OPT_DONATE for this call only (0 = one launch, one slot per board: what a
        bounded slice of search.LexSearch or a node's batch wants), None = the context's.
        Both are arguments of the one sdk_solve_batch_ex call: the shared context options are
        never touched, so threads sharing an engine cannot see each other's settings."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint16).reshape(n)
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        work = np.empty(n, dtype=np.uint64) if want_work else None
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        if donate is not None and not 0 <= int(donate) <= (1 << 30):
            raise ValueError("donate must be 0, 1 or a split budget >= 2")
        if not hasattr(self.lib, "sdk_solve_batch_ex"):
            # an older library named by SDK_LIB_PATH (dev A/B builds): per-call donate by the option
            return self._solve_batch_old(boards, masks, out, status, work, budget, donate)
        L.check(self.lib.sdk_solve_batch_ex(self.ctx, _ptr(boards), _ptr(masks), _ptr(out), _ptr(status), _ptr(work),
                                            n, L.SDK_BUDGET_CONTEXT if budget is None else int(budget),
                                            L.SDK_DONATE_CONTEXT if donate is None else int(donate)),
                "sdk_solve_batch_ex")
        return out, status, work

    def _solve_batch_old(self, boards, masks, out, status, work, budget, donate):
        old = self.get_option(L.SDK_OPT_DONATE)
        if donate is not None:
            self.set_option(L.SDK_OPT_DONATE, int(donate))
        try:
            L.check(self.lib.sdk_solve_batch_budget(self.ctx, _ptr(boards), _ptr(masks), _ptr(out), _ptr(status),
                                                    _ptr(work), len(boards),
                                                    L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                    "sdk_solve_batch_budget")
        finally:
            self.set_option(L.SDK_OPT_DONATE, old)
        return out, status, work

    def classify_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], out uint8[n,81]): does each board have no completion
        (SDK_UNSOLVABLE), exactly one (SDK_SOLVED, out = that completion) or several
        (SDK_MULTIPLE)?  out is the input for every status but SDK_SOLVED.  budget as in
        solve_batch (a board that runs out is SDK_BUDGET_HIT)."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        L.check(self.lib.sdk_classify_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), n,
                                            L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_classify_batch")
        return status, out

    def grade_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], level uint8[n], open uint8[n], out uint8[n,81]): which
        technique does each board need (sdk_grade_batch)?  status and out are classify_batch's.
        level is 1 (naked singles), 2 (+ hidden singles), 3 (+ locked candidates) or 4 (a search)
        for a board with exactly one completion and clean givens, 0 for every other; open is the
        number of cells the three techniques leave open on a level-4 board, else 0.  budget as in
        classify_batch: it bounds the search only (a board that runs out has level 0)."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        level = np.empty(n, dtype=np.uint8)
        open_ = np.empty(n, dtype=np.uint8)
        L.check(self.lib.sdk_grade_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), _ptr(level), _ptr(open_), n,
                                         L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_grade_batch")
        return status, level, open_, out

    def rate_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], level uint8[n], open uint8[n], backdoors uint8[n], key
        uint8[n], out uint8[n,81]): grade_batch, and for every level-4 board its single-cell backdoors
        (sdk_rate_batch) -- the empty cells whose correct digit, once given, lets the three techniques
        finish the board.  backdoors is their number (0: the board needs two guesses), key the lowest
        such cell (SDK_RATE_NONE = 0xFF if none); both are 0xFF for every board of another level.
        status, level, open and out are exactly grade_batch's.  Like grade_batch this call is not
        sharded by MultiDeviceEngine or ShardedBatch: it runs on this engine's device."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        level, open_, backdoors, key = (np.empty(n, dtype=np.uint8) for _ in range(4))
        L.check(self.lib.sdk_rate_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), _ptr(level), _ptr(open_),
                                        _ptr(backdoors), _ptr(key), n,
                                        L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_rate_batch")
        return status, level, open_, backdoors, key, out

    def subsets_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], level uint8[n], open uint8[n], open4 uint8[n], out
        uint8[n,81]): grade_batch, and for every level-4 board the number of cells still open once
        naked and hidden pairs, triples and quads join the three techniques (sdk_subsets_batch).
        open4 == 0: the subsets finish the board, it needs no guess; open4 is SDK_SUBSETS_NONE = 0xFF
        for every board of another level.  status, level, open and out are exactly grade_batch's.
        Like grade_batch and rate_batch this call is not sharded by MultiDeviceEngine or ShardedBatch:
        it runs on this engine's device."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        level, open_, open4 = (np.empty(n, dtype=np.uint8) for _ in range(3))
        L.check(self.lib.sdk_subsets_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), _ptr(level), _ptr(open_),
                                           _ptr(open4), n, L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_subsets_batch")
        return status, level, open_, open4, out

    def fish_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], level uint8[n], open uint8[n], open4 uint8[n], open5 uint8[n],
        out uint8[n,81]): subsets_batch, and for every level-4 board the number of cells still open once
        X-wings, swordfish and jellyfish (row and column fish of sizes 2..4) join the subsets
        (sdk_fish_batch).  open4 > 0 and open5 == 0: the board needs a fish, and a fish is enough; open5 is
        SDK_FISH_NONE = 0xFF for every board of another level.  status, level, open and out are exactly
        grade_batch's, open4 is subsets_batch's.  Not sharded by MultiDeviceEngine or ShardedBatch: it runs
        on this engine's device."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        level, open_, open4, open5 = (np.empty(n, dtype=np.uint8) for _ in range(4))
        L.check(self.lib.sdk_fish_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), _ptr(level), _ptr(open_),
                                        _ptr(open4), _ptr(open5), n,
                                        L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_fish_batch")
        return status, level, open_, open4, open5, out

    def wings_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], level uint8[n], open uint8[n], open4 uint8[n], open5 uint8[n],
        open6 uint8[n], out uint8[n,81]): fish_batch, and for every level-4 board the number of cells still
        open once XY-wings, XYZ-wings and simple colouring join the fish (sdk_wings_batch).  open5 > 0 and
        open6 == 0: the board needs a wing or a colouring, and that is enough; open6 is SDK_WINGS_NONE = 0xFF
        for every board of another level.  status, level, open and out are exactly grade_batch's, open4 and
        open5 are fish_batch's.  Not sharded by MultiDeviceEngine or ShardedBatch: it runs on this engine's
        device."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        level, open_, open4, open5, open6 = (np.empty(n, dtype=np.uint8) for _ in range(5))
        L.check(self.lib.sdk_wings_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), _ptr(level), _ptr(open_),
                                         _ptr(open4), _ptr(open5), _ptr(open6), n,
                                         L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_wings_batch")
        return status, level, open_, open4, open5, open6, out

    def chains_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], level uint8[n], open uint8[n], open4 uint8[n], open5 uint8[n],
        open6 uint8[n], open7 uint8[n], out uint8[n,81]): wings_batch, and for every level-4 board the number
        of cells still open once X-chains and XY-chains join the wings and simple colouring
        (sdk_chains_batch).  open6 > 0 and open7 == 0: the board needs a chain, and a chain is enough; open7
        is SDK_CHAINS_NONE = 0xFF for every board of another level.  status, level, open and out are exactly
        grade_batch's, open4, open5 and open6 are wings_batch's.  Not sharded by MultiDeviceEngine or
        ShardedBatch: it runs on this engine's device."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        level, open_, open4, open5, open6, open7 = (np.empty(n, dtype=np.uint8) for _ in range(6))
        L.check(self.lib.sdk_chains_batch(self.ctx, _ptr(boards), _ptr(out), _ptr(status), _ptr(level), _ptr(open_),
                                          _ptr(open4), _ptr(open5), _ptr(open6), _ptr(open7), n,
                                          L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_chains_batch")
        return status, level, open_, open4, open5, open6, open7, out

    def canonical_batch(self, boards, budget=None):
        """uint8[n,81] -> (status int8[n], canon uint8[n,81], solution uint8[n,81], gather uint8[n,81],
        relabel uint8[n,10], ties uint16[n]): the canonical form of each board under the Sudoku
        symmetries (sdk_canonical_batch).  status is classify_batch's.  For a board with exactly one
        completion and clean givens, canon is the smallest image of the board among the symmetries that
        take its completion to the smallest image of any, solution is that image of the completion,
        (gather, relabel) is the symmetry in synth.apply_symmetries' form and ties the number of
        automorphisms of the completion.  Two such boards are the same puzzle iff their canon rows are
        equal: np.unique(canon[status == 1], axis=0) dedupes a corpus.  Every other board comes back
        unchanged with the identity symmetry, ties 0 and classify_batch's out as solution.  Like
        grade_batch this call is not sharded by MultiDeviceEngine or ShardedBatch."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if budget is not None and not 0 <= int(budget) < (1 << 63):
            raise ValueError("budget must be 0 (unlimited) or a positive node count")
        canon, solution, gather = (np.empty_like(boards) for _ in range(3))
        status = np.empty(n, dtype=np.int8)
        relabel = np.empty((n, 10), dtype=np.uint8)
        ties = np.empty(n, dtype=np.uint16)
        L.check(self.lib.sdk_canonical_batch(self.ctx, _ptr(boards), _ptr(canon), _ptr(solution), _ptr(status),
                                             _ptr(gather), _ptr(relabel), _ptr(ties), n,
                                             L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_canonical_batch")
        return status, canon, solution, gather, relabel, ties

    @staticmethod
    def check_order(order, n):
        """order -> uint8[n,81], every row a permutation of 0..80 (else ValueError)."""
        order = np.asarray(order)
        if order.size != n * 81:
            raise ValueError(f"order must be [{n}, 81]")
        wide = order.reshape(n, 81).astype(np.int64, copy=False)
        if n and not (np.sort(wide, axis=1) == np.arange(81)).all():
            raise ValueError("every order row must be a permutation of 0..80")
        return np.ascontiguousarray(wide, dtype=np.uint8)

    def minimize_batch(self, boards, order=None, seed=0):
        """uint8[n,81] -> (puzzles uint8[n,81], status int8[n]): greedy clue removal on the GPU
        (sdk_minimize_batch).  status[i] is classify_batch's verdict of board i; a board that is
        not SDK_SOLVED comes back unchanged, the others lose, in the cell order of order[i]
        (uint8[n,81], a permutation of 0..80 per row), every clue without which they still have
        exactly one completion.  order=None draws one permutation per board from
        np.random.default_rng(seed).  A bad order raises ValueError before any launch."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if order is None:
            order = np.random.default_rng(seed).permuted(np.tile(np.arange(81, dtype=np.uint8), (n, 1)), axis=1)
        order = self.check_order(order, n)
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        L.check(self.lib.sdk_minimize_batch(self.ctx, _ptr(boards), _ptr(order), _ptr(out), _ptr(status), n),
                "sdk_minimize_batch")
        return out, status

    @staticmethod
    def _check_level(level):
        level = int(level)
        if not L.SDK_GRADE_NAKED <= level <= L.SDK_GRADE_LOCKED:
            raise ValueError("level must be 1 (naked singles), 2 (+ hidden singles) or 3 (+ locked candidates)")
        return level

    def minimize_level_batch(self, boards, level, order=None, seed=0):
        """uint8[n,81] -> (puzzles uint8[n,81], status int8[n]): clue removal that stops at a technique
        level, on the GPU (sdk_minimize_level_batch).  status[i] is 1 when board i has clean givens and
        the techniques of `level` (grade_batch's levels 1..3) close it; every other board comes back
        unchanged with status 0.  An eligible board loses, in the cell order of order[i] (as in
        minimize_batch, and drawn from `seed` the same way when None), every clue without which those
        techniques still close it: grade_batch gives the result a level <= `level`, and no clue of it
        can go at that level.  A bad level or order raises ValueError before any launch.  Like
        grade_batch this call is not sharded by MultiDeviceEngine or ShardedBatch."""
        level = self._check_level(level)
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if order is None:
            order = np.random.default_rng(seed).permuted(np.tile(np.arange(81, dtype=np.uint8), (n, 1)), axis=1)
        order = self.check_order(order, n)
        out = np.empty_like(boards)
        status = np.empty(n, dtype=np.int8)
        L.check(self.lib.sdk_minimize_level_batch(self.ctx, _ptr(boards), _ptr(order), level, _ptr(out), _ptr(status),
                                                  n),
                "sdk_minimize_level_batch")
        return out, status

    def generate_level(self, n, level, seed=synth.DEFAULT_SEED + 3, lo=0):
        """Rows [lo, lo+n) of the stream of puzzles minimal for a technique level, made on the GPU
        (sdk_generate_level: generate_grids, then minimize_level_batch in the grids' own removal
        orders): (puzzles uint8[n,81], solutions uint8[n,81], status int8[n]).  Row k depends only on
        (seed, k, level); status is 1 for every row (a grid dropped by SDK_OPT_GEN_CAP is 0, zeros in
        both)."""
        level = self._check_level(level)
        n, seed, lo = self._stream_rows(n, seed, lo)
        puzzles = np.empty((n, 81), dtype=np.uint8)
        grids = np.empty((n, 81), dtype=np.uint8)
        status = np.empty(n, dtype=np.int8)
        L.check(self.lib.sdk_generate_level(self.ctx, seed, lo, n, level, _ptr(puzzles), _ptr(grids), _ptr(status)),
                "sdk_generate_level")
        return puzzles, grids, status

    @staticmethod
    def _stream_rows(n, seed, lo):
        n, seed, lo = int(n), int(seed), int(lo)
        if n < 0 or not 0 <= seed < (1 << 64) or not 0 <= lo < (1 << 64):
            raise ValueError("n must be >= 0, seed and lo unsigned 64-bit integers")
        return n, seed, lo

    def generate_grids(self, n, seed=synth.DEFAULT_SEED + 3, lo=0, want_order=False, want_placements=False):
        """Rows [lo, lo+n) of the stream of random complete grids, made on the GPU (sdk_generate_grids):
        (grids uint8[n,81], order, placements).  Row k depends only on (seed, k): the grids are
        synth.minimal_grids's, and with want_order / want_placements (else None) the cell orders
        uint8[n,81] and fill placement counts uint32[n] are synth.grid_orders's, byte for byte.  A
        grid whose fill places more than SDK_OPT_GEN_CAP digits comes back as zeros with the count
        0xFFFFFFFF."""
        n, seed, lo = self._stream_rows(n, seed, lo)
        grids = np.empty((n, 81), dtype=np.uint8)
        order = np.empty((n, 81), dtype=np.uint8) if want_order else None
        placements = np.empty(n, dtype=np.uint32) if want_placements else None
        L.check(self.lib.sdk_generate_grids(self.ctx, seed, lo, n, _ptr(grids), _ptr(order), _ptr(placements)),
                "sdk_generate_grids")
        return grids, order, placements

    def generate_batch(self, n, seed=synth.DEFAULT_SEED + 3, lo=0):
        """Rows [lo, lo+n) of the stream of minimal unique puzzles, made on the GPU
        (sdk_generate_puzzles: generate_grids, then minimize_batch in the grids' own removal orders):
        (puzzles uint8[n,81], solutions uint8[n,81], status int8[n]).  puzzles and solutions are
        exactly synth.make_minimal(n, seed, lo); status is SDK_SOLVED for every row (a grid dropped
        by SDK_OPT_GEN_CAP is SDK_MULTIPLE, zeros in both)."""
        n, seed, lo = self._stream_rows(n, seed, lo)
        puzzles = np.empty((n, 81), dtype=np.uint8)
        grids = np.empty((n, 81), dtype=np.uint8)
        status = np.empty(n, dtype=np.int8)
        L.check(self.lib.sdk_generate_puzzles(self.ctx, seed, lo, n, _ptr(puzzles), _ptr(grids), _ptr(status)),
                "sdk_generate_puzzles")
        return puzzles, grids, status

    @staticmethod
    def _graded_args(n, levels, seed, lo, clues, max_scan, chunk, band=None, band2=None):
        """The arguments of sdk_generate_graded from generate_graded's (ValueError for a bad one); band =
        (name, range) adds the (lo, hi) of sdk_generate_rated's backdoors or sdk_generate_subsets' open4,
        band2 a second pair behind it (sdk_generate_fish's open5, sdk_generate_wings' open6,
        sdk_generate_chains' open7)."""
        n, seed, lo = SudokuEngine._stream_rows(n, seed, lo)
        if n >= 1 << 31:
            raise ValueError("n must be below 2^31")
        levels = [int(v) for v in levels]
        if not levels or any(not 1 <= v <= 4 for v in levels):
            raise ValueError("levels must be a non-empty selection of 1, 2, 3, 4")
        mask = 0
        for v in levels:
            mask |= 1 << v
        clues_lo, clues_hi = (0, 81) if clues is None else (int(clues[0]), int(clues[1]))
        if not 0 <= clues_lo <= clues_hi <= 81:
            raise ValueError("clues must be (lo, hi) with 0 <= lo <= hi <= 81")
        max_scan, chunk = int(max_scan), int(chunk)
        if max_scan < 1 or lo + max_scan >= 1 << 64:
            raise ValueError("max_scan must be >= 1 and lo + max_scan an unsigned 64-bit integer")
        if not 0 <= chunk <= L.SDK_GRADED_CHUNK_MAX:
            raise ValueError("chunk must be 0 (automatic) or 1..2^24")
        if band is None:
            return seed, lo, n, mask, clues_lo, clues_hi, max_scan, chunk
        bands = []
        for name, rng in (band,) if band2 is None else (band, band2):
            f_lo, f_hi = (0, 64) if rng is None else (int(rng[0]), int(rng[1]))
            if not 0 <= f_lo <= f_hi <= 64:
                raise ValueError(f"{name} must be (lo, hi) with 0 <= lo <= hi <= 64")
            bands += [f_lo, f_hi]
        return (seed, lo, n, mask, clues_lo, clues_hi, *bands, max_scan, chunk)

    def _generate_selected(self, family, args, extra):
        """sdk_generate_<family> on host arrays of min(n, max_scan) rows, `extra` uint8 columns after
        level and open: (puzzles, solutions, level, open, *extra, index, scanned), `found` rows each."""
        n, max_scan = args[2], args[-2]     # _graded_args: (seed, lo, n, mask, ..., max_scan, chunk) with or without bands
        assert len(args) in (8, 10, 12)
        rows = min(n, max_scan)
        puzzles = np.empty((rows, 81), dtype=np.uint8)
        grids = np.empty((rows, 81), dtype=np.uint8)
        cols = [np.empty(rows, dtype=np.uint8) for _ in range(2 + extra)]
        index = np.empty(rows, dtype=np.uint64)
        found, scanned = ctypes.c_uint64(), ctypes.c_uint64()
        name = "sdk_generate_" + family
        L.check(getattr(self.lib, name)(self.ctx, *args, _ptr(puzzles), _ptr(grids), *map(_ptr, cols), _ptr(index),
                                        ctypes.byref(found), ctypes.byref(scanned)), name)
        f = found.value
        return (puzzles[:f], grids[:f], *(c[:f] for c in cols), index[:f], scanned.value)

    def _generate_selected_dev(self, family, args, d_puzzles, d_grids, d_cols, d_index):
        """sdk_generate_<family>_dev; d_cols: the optional device columns between d_grids and d_index."""
        found, scanned = ctypes.c_uint64(), ctypes.c_uint64()
        name = "sdk_generate_" + family + "_dev"
        L.check(getattr(self.lib, name)(self.ctx, *args, d_puzzles.ptr, d_grids.ptr,
                                        *(b.ptr if b else None for b in d_cols), d_index.ptr if d_index else None,
                                        ctypes.byref(found), ctypes.byref(scanned)), name)
        return found.value, scanned.value

    def generate_graded(self, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0, clues=None,
                        max_scan=1 << 26, chunk=0):
        """The first n puzzles of generate_batch's stream, from row lo on, whose grade_batch level is one
        of `levels` and whose clue count lies in clues = (lo, hi) (None: any), made, graded and selected
        on the GPU (sdk_generate_graded): (puzzles uint8[found,81], solutions uint8[found,81], level
        uint8[found], open uint8[found], index uint64[found], scanned).  At most max_scan rows are
        looked at, so found <= n; index holds the stream rows of the puzzles, ascending; scanned is the
        number of rows up to and including the n-th match (max_scan if there were fewer).  chunk is the
        number of rows per round (0 = automatic): it changes speed and memory only, never the result.
        A bad argument raises ValueError before any launch."""
        return self._generate_selected("graded", self._graded_args(n, levels, seed, lo, clues, max_scan, chunk), 0)

    def generate_rated(self, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0, clues=None, backdoors=None,
                       max_scan=1 << 26, chunk=0):
        """generate_graded with a rating filter (sdk_generate_rated): a level-4 puzzle is kept only when
        its rate_batch backdoor count lies in backdoors = (lo, hi) (None: 0..64); puzzles of levels 1..3
        are not filtered by it.  Returns generate_graded's tuple with the ratings after open:
        (puzzles, solutions, level, open, backdoors uint8[found], key uint8[found], index, scanned);
        backdoors and key are 0xFF for the puzzles of levels 1..3."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("backdoors", backdoors))
        return self._generate_selected("rated", args, 2)

    def generate_subsets(self, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0, clues=None, open4=None,
                         max_scan=1 << 26, chunk=0):
        """generate_graded with a subsets filter (sdk_generate_subsets): a level-4 puzzle is kept only
        when its subsets_batch count lies in open4 = (lo, hi) (None: 0..64); puzzles of levels 1..3 are
        not filtered by it.  levels=(4,), open4=(0, 0): the hard puzzles that need no guess.  Returns
        generate_graded's tuple with the counts after open: (puzzles, solutions, level, open, open4
        uint8[found], index, scanned); open4 is 0xFF for the puzzles of levels 1..3.  Not sharded by
        MultiDeviceEngine, like generate_graded and generate_rated."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open4", open4))
        return self._generate_selected("subsets", args, 1)

    def generate_fish(self, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0, clues=None, open4=None,
                      open5=None, max_scan=1 << 26, chunk=0):
        """generate_graded with a subsets and a fish filter (sdk_generate_fish): a level-4 puzzle is kept only
        when its fish_batch counts lie in open4 = (lo, hi) and open5 = (lo, hi) (None: 0..64); puzzles of
        levels 1..3 are not filtered by them.  levels=(4,), open4=(1, 64), open5=(0, 0): the puzzles that
        need a fish, and for which a fish is enough.  Returns generate_graded's tuple with the counts after
        open: (puzzles, solutions, level, open, open4 uint8[found], open5 uint8[found], index, scanned);
        both are 0xFF for the puzzles of levels 1..3.  Not sharded by MultiDeviceEngine, like
        generate_graded."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open4", open4), ("open5", open5))
        return self._generate_selected("fish", args, 2)

    def generate_wings(self, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0, clues=None, open5=None,
                       open6=None, max_scan=1 << 26, chunk=0):
        """generate_graded with a fish and a wings filter (sdk_generate_wings): a level-4 puzzle is kept only
        when its wings_batch counts lie in open5 = (lo, hi) and open6 = (lo, hi) (None: 0..64); puzzles of
        levels 1..3 are not filtered by them.  levels=(4,), open5=(1, 64), open6=(0, 0): the puzzles that
        need a wing or a colouring, and for which that is enough.  Returns generate_graded's tuple with the
        counts after open: (puzzles, solutions, level, open, open5 uint8[found], open6 uint8[found], index,
        scanned); both are 0xFF for the puzzles of levels 1..3.  Not sharded by MultiDeviceEngine, like
        generate_graded."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open5", open5), ("open6", open6))
        return self._generate_selected("wings", args, 2)

    def generate_chains(self, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0, clues=None, open6=None,
                        open7=None, max_scan=1 << 26, chunk=0):
        """generate_graded with a wings and a chains filter (sdk_generate_chains): a level-4 puzzle is kept
        only when its chains_batch counts lie in open6 = (lo, hi) and open7 = (lo, hi) (None: 0..64); puzzles
        of levels 1..3 are not filtered by them.  levels=(4,), open6=(1, 64), open7=(0, 0): the puzzles that
        need a chain, and for which a chain is enough.  Returns generate_graded's tuple with the counts after
        open: (puzzles, solutions, level, open, open6 uint8[found], open7 uint8[found], index, scanned); both
        are 0xFF for the puzzles of levels 1..3.  Not sharded by MultiDeviceEngine, like generate_graded."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open6", open6), ("open7", open7))
        return self._generate_selected("chains", args, 2)

    def expand(self, boards, masks=None, target=64):
        """Lex-ordered frontier below `boards` (sdk_expand_boards): uint8[k,81], children in the
        reference's DFS order, parents' order kept; at least one level, >= target boards unless
        nothing branches.  Contradicted subtrees vanish, solved boards stay."""
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = boards.shape[0]
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint16).reshape(n)
        cap = 9 * max(n, int(target), 1)
        # a per-thread staging buffer, grown as needed: a fresh 9 x target board array per call
        # is megabytes of new pages for every slice of a continued search (search.LexSearch)
        tl = self._tls
        out = getattr(tl, "expand_buf", None)
        if out is None or out.shape[0] < cap:
            out = tl.expand_buf = np.empty((cap, 81), dtype=np.uint8)
        k = ctypes.c_uint64()
        L.check(self.lib.sdk_expand_boards(self.ctx, _ptr(boards), _ptr(masks), n, int(target), _ptr(out), cap,
                                           ctypes.byref(k)), "sdk_expand_boards")
        return out[:k.value].copy()

    def count_solutions(self, board, limit=0):
        board = np.ascontiguousarray(board, dtype=np.uint8).reshape(81)
        cnt = ctypes.c_uint64()
        st = ctypes.c_int8()
        L.check(self.lib.sdk_count_solutions(self.ctx, _ptr(board), int(limit), ctypes.byref(cnt), ctypes.byref(st)),
                "sdk_count_solutions")
        return cnt.value, st.value

    def count_solutions_slice(self, board, rank, world, limit=0):
        """This rank's share of a frontier-split count: (local_count, frontier_size, status)."""
        board = np.ascontiguousarray(board, dtype=np.uint8).reshape(81)
        cnt = ctypes.c_uint64()
        fr = ctypes.c_uint64()
        st = ctypes.c_int8()
        L.check(self.lib.sdk_count_solutions_slice(self.ctx, _ptr(board), int(limit), int(rank), int(world),
                                                   ctypes.byref(cnt), ctypes.byref(fr), ctypes.byref(st)),
                "sdk_count_solutions_slice")
        return cnt.value, fr.value, st.value

    # frontier records (rebalanced counts move them between ranks)
    def frontier_boards(self):
        """(device address, size) of the current frontier's uint8[size][81] records."""
        p = ctypes.c_void_p()
        size = ctypes.c_uint64()
        L.check(self.lib.sdk_frontier_boards_dev(self.ctx, ctypes.byref(p), ctypes.byref(size)),
                "sdk_frontier_boards_dev")
        return p.value, size.value

    def frontier_records(self, lo, hi):
        """(device address, bytes) of records [lo, hi) of the current frontier: what a rank sends
        to another (comm p2p) when it hands on part of its live subtrees."""
        p, size = self.frontier_boards()
        if not 0 <= lo <= hi <= size:
            raise ValueError(f"records [{lo}, {hi}) outside the frontier of {size}")
        return p + 81 * int(lo), 81 * (int(hi) - int(lo))

    def record_buffer(self, n):
        """A device buffer for n board records (a receive buffer of moved records)."""
        return self.alloc(81 * max(1, int(n)))

    def frontier_load(self, d_boards, n, offset=0):
        """The n records at device buffer `d_boards` (+ offset boards) become the current
        frontier (in the mode of the frontier built last)."""
        ptr = (d_boards.ptr.value if hasattr(d_boards, "ptr") else int(d_boards)) + 81 * int(offset)
        L.check(self.lib.sdk_frontier_load_dev(self.ctx, ctypes.c_void_p(ptr), int(n)), "sdk_frontier_load_dev")

    def frontier_refine_range(self, lo, hi, target):
        """Keep frontier boards [lo, hi) and expand them until they number `target`: (size, leaves)."""
        size = ctypes.c_uint64()
        leaves = ctypes.c_uint64()
        L.check(self.lib.sdk_frontier_refine_range(self.ctx, int(lo), int(hi), int(target), ctypes.byref(size),
                                                   ctypes.byref(leaves)), "sdk_frontier_refine_range")
        return size.value, leaves.value

    def frontier_refine_head(self, lo, mid, hi, target):
        """Frontier boards [lo, mid) refined towards `target`, then [mid, hi) unchanged: (size, leaves)."""
        size = ctypes.c_uint64()
        leaves = ctypes.c_uint64()
        L.check(self.lib.sdk_frontier_refine_head(self.ctx, int(lo), int(mid), int(hi), int(target),
                                                  ctypes.byref(size), ctypes.byref(leaves)),
                "sdk_frontier_refine_head")
        return size.value, leaves.value

    # ------------------------------------------- one-board multi-GPU searches
    def frontier_build(self, board, mask=None, mode=L.SDK_FRONTIER_COUNT, target=0):
        """Build the deterministic frontier of `board` on this GPU: (size, leaves)."""
        board = np.ascontiguousarray(board, dtype=np.uint8).reshape(81)
        m = None if mask is None else np.array([int(mask)], dtype=np.uint16)
        size = ctypes.c_uint64()
        leaves = ctypes.c_uint64()
        L.check(self.lib.sdk_frontier_build(self.ctx, _ptr(board), _ptr(m), int(mode), int(target),
                                            ctypes.byref(size), ctypes.byref(leaves)), "sdk_frontier_build")
        return size.value, leaves.value

    def frontier_refine(self, first, step, target):
        """Keep frontier boards first, first+step, ... and expand them on this GPU until they
        number `target` (the rank-local second stage of a split): (size, leaves met)."""
        size = ctypes.c_uint64()
        leaves = ctypes.c_uint64()
        L.check(self.lib.sdk_frontier_refine(self.ctx, int(first), int(step), int(target), ctypes.byref(size),
                                             ctypes.byref(leaves)), "sdk_frontier_refine")
        return size.value, leaves.value

    def frontier_count(self, first, step, end, limit, d_result):
        """Completions below frontier boards first, first+step, ... < end -> d_result {count, budget hits}."""
        L.check(self.lib.sdk_frontier_count_dev(self.ctx, int(first), int(step), int(end), int(limit), d_result.ptr),
                "sdk_frontier_count_dev")

    def frontier_first(self, lo, hi, d_found, d_best):
        """Lex-ordered scan step: lowest hit index in [lo, hi) -> d_found, its board + status -> d_best."""
        L.check(self.lib.sdk_frontier_first_dev(self.ctx, int(lo), int(hi), d_found.ptr, d_best.ptr),
                "sdk_frontier_first_dev")

    def result_buffer(self, count, dtype):
        """A small device buffer for per-rank results (a handle for the comm layer)."""
        buf = self.alloc(count * np.dtype(dtype).itemsize)
        buf.upload(np.zeros(count, dtype=dtype))
        return buf

    def read(self, buf, count, dtype):
        out = np.empty(count, dtype=dtype)
        return buf.download(out)

    # ----------------------------------------------------------------- RCCL
    @staticmethod
    def comm_unique_id():
        lib = L.load()
        buf = (ctypes.c_uint8 * L.SDK_COMM_ID_BYTES)()
        L.check(lib.sdk_comm_unique_id(buf), "sdk_comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid, rank, world):
        buf = (ctypes.c_uint8 * L.SDK_COMM_ID_BYTES).from_buffer_copy(uid)
        L.check(self.lib.sdk_comm_init(self.ctx, buf, int(rank), int(world)), "sdk_comm_init")

    def comm_destroy(self):
        L.check(self.lib.sdk_comm_destroy(self.ctx), "sdk_comm_destroy")

    def comm_allreduce(self, d_buf, count, dtype, op):
        L.check(self.lib.sdk_comm_allreduce_dev(self.ctx, d_buf.ptr, int(count), int(dtype), int(op)),
                "sdk_comm_allreduce_dev")

    def comm_broadcast(self, d_buf, nbytes, root):
        L.check(self.lib.sdk_comm_broadcast_dev(self.ctx, d_buf.ptr, int(nbytes), int(root)), "sdk_comm_broadcast_dev")

    def comm_p2p(self, ops):
        """One grouped ncclSend/ncclRecv: ops = [(L.SDK_COMM_SEND | L.SDK_COMM_RECV, peer,
        device address or DeviceBuffer, nbytes), ...]."""
        k = len(ops)
        if k == 0:
            return
        kinds = (ctypes.c_int * k)(*[int(o[0]) for o in ops])
        peers = (ctypes.c_int * k)(*[int(o[1]) for o in ops])
        bufs = (ctypes.c_void_p * k)(*[(o[2].ptr.value if hasattr(o[2], "ptr") else int(o[2])) for o in ops])
        sizes = (ctypes.c_size_t * k)(*[int(o[3]) for o in ops])
        L.check(self.lib.sdk_comm_p2p_dev(self.ctx, k, kinds, peers, bufs, sizes), "sdk_comm_p2p_dev")

    def comm_allgather(self, d_send, d_recv, nbytes):
        L.check(self.lib.sdk_comm_allgather_dev(self.ctx, d_send.ptr, d_recv.ptr, int(nbytes)),
                "sdk_comm_allgather_dev")

    # --------------------------------------------------------- device batch
    def check_batch_dev(self, d_boards, d_verdict, n):
        L.check(self.lib.sdk_check_batch_dev(self.ctx, d_boards.ptr, d_verdict.ptr, int(n)), "sdk_check_batch_dev")

    def solve_batch_dev(self, d_in, d_out, d_status, n, d_mask=None, d_work=None):
        L.check(self.lib.sdk_solve_batch_dev(self.ctx, d_in.ptr, d_mask.ptr if d_mask else None, d_out.ptr,
                                             d_status.ptr, d_work.ptr if d_work else None, int(n)),
                "sdk_solve_batch_dev")

    def classify_batch_dev(self, d_in, d_out, d_status, n, budget=None):
        L.check(self.lib.sdk_classify_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, int(n),
                                                L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_classify_batch_dev")

    def grade_batch_dev(self, d_in, d_out, d_status, d_level, n, d_open=None, budget=None):
        """d_in and d_out 16-byte aligned (d_out may be d_in); d_open optional."""
        L.check(self.lib.sdk_grade_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, d_level.ptr,
                                             d_open.ptr if d_open else None, int(n),
                                             L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_grade_batch_dev")

    def rate_batch_dev(self, d_in, d_out, d_status, d_level, d_backdoors, n, d_open=None, d_key=None, budget=None):
        """rate_batch on device buffers: as grade_batch_dev (d_in and d_out 16-byte aligned, d_out may
        be d_in), d_backdoors required, d_open and d_key optional."""
        L.check(self.lib.sdk_rate_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, d_level.ptr,
                                            d_open.ptr if d_open else None, d_backdoors.ptr,
                                            d_key.ptr if d_key else None, int(n),
                                            L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_rate_batch_dev")

    def subsets_batch_dev(self, d_in, d_out, d_status, d_level, d_open4, n, d_open=None, budget=None):
        """subsets_batch on device buffers: as grade_batch_dev (d_in and d_out 16-byte aligned, d_out
        may be d_in), d_open4 required, d_open optional."""
        L.check(self.lib.sdk_subsets_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, d_level.ptr,
                                               d_open.ptr if d_open else None, d_open4.ptr, int(n),
                                               L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_subsets_batch_dev")

    def fish_batch_dev(self, d_in, d_out, d_status, d_level, d_open5, n, d_open=None, d_open4=None, budget=None):
        """fish_batch on device buffers: as grade_batch_dev (d_in and d_out 16-byte aligned, d_out may be
        d_in), d_open5 required, d_open and d_open4 optional."""
        L.check(self.lib.sdk_fish_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, d_level.ptr,
                                            d_open.ptr if d_open else None, d_open4.ptr if d_open4 else None,
                                            d_open5.ptr, int(n),
                                            L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_fish_batch_dev")

    def wings_batch_dev(self, d_in, d_out, d_status, d_level, d_open6, n, d_open=None, d_open4=None, d_open5=None,
                        budget=None):
        """wings_batch on device buffers: as grade_batch_dev (d_in and d_out 16-byte aligned, d_out may be
        d_in), d_open6 required, d_open, d_open4 and d_open5 optional."""
        L.check(self.lib.sdk_wings_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, d_level.ptr,
                                             d_open.ptr if d_open else None, d_open4.ptr if d_open4 else None,
                                             d_open5.ptr if d_open5 else None, d_open6.ptr, int(n),
                                             L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_wings_batch_dev")

    def chains_batch_dev(self, d_in, d_out, d_status, d_level, d_open7, n, d_open=None, d_open4=None, d_open5=None,
                         d_open6=None, budget=None):
        """chains_batch on device buffers: as grade_batch_dev (d_in and d_out 16-byte aligned, d_out may be
        d_in), d_open7 required, d_open, d_open4, d_open5 and d_open6 optional."""
        L.check(self.lib.sdk_chains_batch_dev(self.ctx, d_in.ptr, d_out.ptr, d_status.ptr, d_level.ptr,
                                              d_open.ptr if d_open else None, d_open4.ptr if d_open4 else None,
                                              d_open5.ptr if d_open5 else None, d_open6.ptr if d_open6 else None,
                                              d_open7.ptr if d_open7 else None, int(n),
                                              L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_chains_batch_dev")

    def canonical_batch_dev(self, d_in, d_canon, d_status, n, d_solution=None, d_gather=None, d_relabel=None,
                            d_ties=None, budget=None):
        """canonical_batch on device buffers: d_in and d_canon 16-byte aligned (d_canon may be d_in);
        d_solution, d_gather, d_relabel (10 bytes per board) and d_ties (uint16 per board) optional."""
        opt = lambda d: d.ptr if d else None
        L.check(self.lib.sdk_canonical_batch_dev(self.ctx, d_in.ptr, d_canon.ptr, opt(d_solution), d_status.ptr,
                                                 opt(d_gather), opt(d_relabel), opt(d_ties), int(n),
                                                 L.SDK_BUDGET_CONTEXT if budget is None else int(budget)),
                "sdk_canonical_batch_dev")

    def minimize_batch_dev(self, d_in, d_order, d_out, d_status, n):
        """The order rows are not validated on this path (see include/sudoku_hip.h)."""
        L.check(self.lib.sdk_minimize_batch_dev(self.ctx, d_in.ptr, d_order.ptr, d_out.ptr, d_status.ptr, int(n)),
                "sdk_minimize_batch_dev")

    def minimize_level_batch_dev(self, d_in, d_order, level, d_out, d_status, n):
        """The level and the order rows are not validated on this path (see include/sudoku_hip.h);
        d_out may be d_in."""
        L.check(self.lib.sdk_minimize_level_batch_dev(self.ctx, d_in.ptr, d_order.ptr, int(level), d_out.ptr,
                                                      d_status.ptr, int(n)),
                "sdk_minimize_level_batch_dev")

    def generate_level_dev(self, d_puzzles, d_grids, d_status, n, level, seed=synth.DEFAULT_SEED + 3, lo=0):
        L.check(self.lib.sdk_generate_level_dev(self.ctx, int(seed), int(lo), int(n), int(level), d_puzzles.ptr,
                                                d_grids.ptr, d_status.ptr),
                "sdk_generate_level_dev")

    def generate_grids_dev(self, d_grids, n, seed=synth.DEFAULT_SEED + 3, lo=0, d_order=None, d_placements=None):
        L.check(self.lib.sdk_generate_grids_dev(self.ctx, int(seed), int(lo), int(n), d_grids.ptr,
                                                d_order.ptr if d_order else None,
                                                d_placements.ptr if d_placements else None),
                "sdk_generate_grids_dev")

    def generate_batch_dev(self, d_puzzles, d_grids, d_status, n, seed=synth.DEFAULT_SEED + 3, lo=0):
        L.check(self.lib.sdk_generate_puzzles_dev(self.ctx, int(seed), int(lo), int(n), d_puzzles.ptr, d_grids.ptr,
                                                  d_status.ptr),
                "sdk_generate_puzzles_dev")

    def generate_graded_dev(self, d_puzzles, d_grids, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0,
                            clues=None, max_scan=1 << 26, chunk=0, d_level=None, d_open=None, d_index=None):
        """generate_graded into device buffers of n rows (d_puzzles, d_grids 16-byte aligned; the others
        optional): -> (found, scanned).  Rows from `found` on are left as they were; the rows are valid
        after synchronize()."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk)
        return self._generate_selected_dev("graded", args, d_puzzles, d_grids, (d_level, d_open), d_index)

    def generate_rated_dev(self, d_puzzles, d_grids, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0,
                           clues=None, backdoors=None, max_scan=1 << 26, chunk=0, d_level=None, d_open=None,
                           d_backdoors=None, d_key=None, d_index=None):
        """generate_rated into device buffers of n rows, as generate_graded_dev: -> (found, scanned)."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("backdoors", backdoors))
        return self._generate_selected_dev("rated", args, d_puzzles, d_grids, (d_level, d_open, d_backdoors, d_key),
                                           d_index)

    def generate_subsets_dev(self, d_puzzles, d_grids, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0,
                             clues=None, open4=None, max_scan=1 << 26, chunk=0, d_level=None, d_open=None,
                             d_open4=None, d_index=None):
        """generate_subsets into device buffers of n rows, as generate_graded_dev: -> (found, scanned)."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open4", open4))
        return self._generate_selected_dev("subsets", args, d_puzzles, d_grids, (d_level, d_open, d_open4), d_index)

    def generate_fish_dev(self, d_puzzles, d_grids, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0,
                          clues=None, open4=None, open5=None, max_scan=1 << 26, chunk=0, d_level=None, d_open=None,
                          d_open4=None, d_open5=None, d_index=None):
        """generate_fish into device buffers of n rows, as generate_graded_dev: -> (found, scanned)."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open4", open4), ("open5", open5))
        return self._generate_selected_dev("fish", args, d_puzzles, d_grids, (d_level, d_open, d_open4, d_open5),
                                           d_index)

    def generate_wings_dev(self, d_puzzles, d_grids, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0,
                           clues=None, open5=None, open6=None, max_scan=1 << 26, chunk=0, d_level=None, d_open=None,
                           d_open5=None, d_open6=None, d_index=None):
        """generate_wings into device buffers of n rows, as generate_graded_dev: -> (found, scanned)."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open5", open5), ("open6", open6))
        return self._generate_selected_dev("wings", args, d_puzzles, d_grids, (d_level, d_open, d_open5, d_open6),
                                           d_index)

    def generate_chains_dev(self, d_puzzles, d_grids, n, levels=(1, 2, 3, 4), seed=synth.DEFAULT_SEED + 3, lo=0,
                            clues=None, open6=None, open7=None, max_scan=1 << 26, chunk=0, d_level=None, d_open=None,
                            d_open6=None, d_open7=None, d_index=None):
        """generate_chains into device buffers of n rows, as generate_graded_dev: -> (found, scanned)."""
        args = self._graded_args(n, levels, seed, lo, clues, max_scan, chunk, ("open6", open6), ("open7", open7))
        return self._generate_selected_dev("chains", args, d_puzzles, d_grids, (d_level, d_open, d_open6, d_open7),
                                           d_index)

    def select_rows_dev(self, rows):
        """One round of the graded selection on caller-supplied device rows (sdk_select_rows_dev): `rows`
        is an L.SelectRows of device addresses and scalars -> (total, last).  puzzles and grids hold
        whole tiles of 64 rows; the outputs are valid on return."""
        total, last = ctypes.c_uint64(), ctypes.c_uint64()
        L.check(self.lib.sdk_select_rows_dev(self.ctx, ctypes.byref(rows), ctypes.byref(total), ctypes.byref(last)),
                "sdk_select_rows_dev")
        return total.value, last.value
