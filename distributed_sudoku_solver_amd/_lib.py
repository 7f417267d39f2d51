"""ctypes binding of libsudoku_hip.so (C-ABI declared in include/sudoku_hip.h).

The shared library is built in-tree (distributed_sudoku_solver_amd/libsudoku_hip.so,
see csrc/Makefile or __graft_entry__.build()).  There is no fallback: if the
library is missing or fails to load, every entry point raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDK_LIB_PATH", os.path.join(HERE, "libsudoku_hip.so"))
HEADER = os.path.join(os.path.dirname(HERE), "include", "sudoku_hip.h")

SDK_ABI_VERSION = 2
SDK_OK = 0
SDK_EINVAL = -1
SDK_EHIP = -2
SDK_ENOMEM = -3
SDK_ECOMM = -4

SDK_SOLVED = 1
SDK_UNSOLVABLE = 0
SDK_BUDGET_HIT = -2
SDK_MULTIPLE = 2      # sdk_classify_batch / sdk_minimize_batch only: at least two completions
SDK_BUDGET_CONTEXT = (1 << 64) - 1    # sdk_solve_batch_budget: use the context's SDK_OPT_NODE_BUDGET

# sdk_grade_batch levels: the technique set a board needs (0: not uniquely solvable / givens not clean)
SDK_GRADE_NONE = 0
SDK_GRADE_NAKED = 1
SDK_GRADE_HIDDEN = 2
SDK_GRADE_LOCKED = 3
SDK_GRADE_SEARCH = 4
# sdk_generate_graded: every level (bits 1..4 of level_mask), the largest explicit chunk
SDK_GRADE_MASK_ALL = 0x1E
SDK_GRADED_CHUNK_MAX = 1 << 24
# sdk_rate_batch: backdoors / key of a board that is not of level SDK_GRADE_SEARCH, key of one without a backdoor
SDK_RATE_NONE = 0xFF
# sdk_subsets_batch: open4 of a board that is not of level SDK_GRADE_SEARCH
SDK_SUBSETS_NONE = 0xFF
# sdk_fish_batch: open5 of a board that is not of level SDK_GRADE_SEARCH
SDK_FISH_NONE = 0xFF
# sdk_wings_batch: open6 of a board that is not of level SDK_GRADE_SEARCH
SDK_WINGS_NONE = 0xFF
# sdk_chains_batch: open7 of a board that is not of level SDK_GRADE_SEARCH
SDK_CHAINS_NONE = 0xFF

SDK_CHECK_OK = 1
SDK_CHECK_RAW_NAMEERROR = 2

SDK_OPT_ORDER = 1
SDK_OPT_NODE_BUDGET = 2
SDK_OPT_WAVES_PER_CU = 3
SDK_OPT_CHECK_BLOCKS_PER_CU = 4
SDK_OPT_WORK_COUNTER = 5
SDK_OPT_DEVICE_CUS = 6
SDK_OPT_SOLVER = 7
SDK_OPT_WAVES_PER_CU2 = 8
SDK_OPT_CHECK_VARIANT = 9
SDK_OPT_SOLVE_CHUNK = 10
SDK_OPT_TIMING = 11
SDK_OPT_TIMER_EVENTS = 12
SDK_OPT_LOCKED = 13
SDK_OPT_XCD_HEADS = 14
SDK_OPT_DONATE = 15
SDK_OPT_DONATED = 16
SDK_OPT_SPLIT_BOARDS = 17
SDK_OPT_DONATE_MODE = 18
SDK_OPT_LEX_BOARDS = 19
SDK_OPT_DONATE_MAX = 20
SDK_OPT_DN_FAULT = 21
SDK_OPT_DONATE_HELPERS = 22
SDK_OPT_DONATE_RESUME = 23
SDK_OPT_RESUMED = 24
SDK_OPT_PROP32 = 25
SDK_OPT_PROP32_LC = 26
SDK_OPT_PROP32_MIN = 27
SDK_OPT_PROP32_UNDECIDED = 28
SDK_OPT_PROP32_HANDOVER = 29
SDK_OPT_PROP32_TAIL = 30
SDK_OPT_GEN_CAP = 31
SDK_DONATE_CONTEXT = -1    # sdk_solve_batch_ex: use the context's SDK_OPT_DONATE
SDK_CHECK_REG1 = 0
SDK_CHECK_REG2 = 1
SDK_CHECK_GLDS2 = 2
SDK_CHECK_GLDS3 = 3
SDK_CHECK_GLDS4 = 4
SDK_CHECK_WAVE1 = 5
SDK_CHECK_WAVE2 = 6

SDK_SOLVER_WAVE = 0
SDK_SOLVER_HALFWAVE = 1
SDK_SOLVER_QUAD = 2
SDK_SOLVER_LANE = 3

SDK_WORK_NODES = 0
SDK_WORK_ROUNDS = 1
SDK_WORK_DEPTH = 2

SDK_ORDER_MRV_UNIQUE = 0
SDK_ORDER_LEX = 1

SDK_FRONTIER_COUNT = 0
SDK_FRONTIER_FIRST = 1

SDK_COMM_ID_BYTES = 128
SDK_COMM_U64 = 0
SDK_COMM_I64 = 1
SDK_COMM_U8 = 2
SDK_COMM_SUM = 0
SDK_COMM_MIN = 1
SDK_COMM_MAX = 2
SDK_COMM_SEND = 0
SDK_COMM_RECV = 1

# every symbol the header declares: name -> (restype, argtypes)
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


class SelectRows(ctypes.Structure):
    """sdk_select_rows (include/sudoku_hip.h): the arguments of sdk_select_rows_dev, field for field."""
    _fields_ = ([(k, _vp) for k in ("puzzles", "grids", "status", "level", "open", "backdoors", "key", "open4")]
                + [(k, ctypes.c_uint64) for k in ("m", "first", "base", "n")]
                + [(k, ctypes.c_uint32) for k in ("level_mask", "clues_lo", "clues_hi", "backdoors_lo",
                                                  "backdoors_hi", "open4_lo", "open4_hi")]
                + [(k, _vp) for k in ("out_puzzles", "out_grids", "out_level", "out_open", "out_index",
                                      "out_backdoors", "out_key", "out_open4")])


SIGNATURES = {
    "sdk_abi_version": (ctypes.c_int, []),
    "sdk_last_error": (ctypes.c_char_p, []),
    "sdk_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "sdk_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "sdk_destroy": (ctypes.c_int, [_vp]),
    "sdk_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64]),
    "sdk_get_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    "sdk_check_batch": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
    "sdk_check_batch_i64": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
    "sdk_solve_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "sdk_solve_batch_budget": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_solve_batch_ex": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64, ctypes.c_int64]),
    "sdk_classify_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_classify_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_grade_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_grade_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_rate_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_rate_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_subsets_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_subsets_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_fish_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_fish_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_wings_batch": (ctypes.c_int, [_vp] * 9 + [_sz, ctypes.c_uint64]),
    "sdk_wings_batch_dev": (ctypes.c_int, [_vp] * 9 + [_sz, ctypes.c_uint64]),
    "sdk_chains_batch": (ctypes.c_int, [_vp] * 10 + [_sz, ctypes.c_uint64]),
    "sdk_chains_batch_dev": (ctypes.c_int, [_vp] * 10 + [_sz, ctypes.c_uint64]),
    # (ctx, in, canon, solution, status, gather, relabel, ties, n, node_budget)
    "sdk_canonical_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_canonical_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_uint64]),
    "sdk_minimize_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "sdk_minimize_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "sdk_minimize_level_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _sz]),
    "sdk_minimize_level_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _sz]),
    "sdk_generate_level": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_int, _vp, _vp, _vp]),
    "sdk_generate_level_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_int, _vp, _vp,
                                              _vp]),
    "sdk_generate_grids": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, _vp, _vp, _vp]),
    "sdk_generate_grids_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, _vp, _vp, _vp]),
    "sdk_generate_puzzles": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, _vp, _vp, _vp]),
    "sdk_generate_puzzles_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, _vp, _vp, _vp]),
    "sdk_generate_graded": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                           _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_graded_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                               _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_rated": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_rated_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_subsets": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp,
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_subsets_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz, ctypes.c_uint32,
                                                ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_fish": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz] + [ctypes.c_uint32] * 7 +
                          [ctypes.c_uint64, ctypes.c_uint64] + [_vp] * 7 +
                          [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_fish_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz] + [ctypes.c_uint32] * 7 +
                              [ctypes.c_uint64, ctypes.c_uint64] + [_vp] * 7 +
                              [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_wings": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz] + [ctypes.c_uint32] * 7 +
                           [ctypes.c_uint64, ctypes.c_uint64] + [_vp] * 7 +
                           [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_wings_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz] + [ctypes.c_uint32] * 7 +
                               [ctypes.c_uint64, ctypes.c_uint64] + [_vp] * 7 +
                               [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_chains": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz] + [ctypes.c_uint32] * 7 +
                            [ctypes.c_uint64, ctypes.c_uint64] + [_vp] * 7 +
                            [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_generate_chains_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _sz] + [ctypes.c_uint32] * 7 +
                                [ctypes.c_uint64, ctypes.c_uint64] + [_vp] * 7 +
                                [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_select_rows_dev": (ctypes.c_int, [_vp, ctypes.POINTER(SelectRows), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_frontier_boards_dev": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_frontier_load_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64]),
    "sdk_frontier_refine_range": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_frontier_refine_head": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_comm_send_dev": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int]),
    "sdk_comm_recv_dev": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int]),
    "sdk_comm_p2p_dev": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "sdk_expand_boards": (ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_uint64, _vp, _sz,
                                         ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_count_solutions": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_int8)]),
    "sdk_count_solutions_slice": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                 ctypes.POINTER(ctypes.c_int8)]),
    "sdk_frontier_build": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_uint64,
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "sdk_frontier_refine": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp]),
    "sdk_frontier_count_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                              ctypes.c_uint64, _vp]),
    "sdk_frontier_first_dev": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp]),
    "sdk_comm_unique_id": (ctypes.c_int, [_vp]),
    "sdk_comm_init": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    "sdk_comm_init_all": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "sdk_comm_destroy": (ctypes.c_int, [_vp]),
    "sdk_comm_allreduce_dev": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int]),
    "sdk_comm_broadcast_dev": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int]),
    "sdk_comm_allgather_dev": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
    "sdk_dev_alloc": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(_vp)]),
    "sdk_dev_free": (ctypes.c_int, [_vp, _vp]),
    "sdk_memcpy_h2d": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
    "sdk_memcpy_d2h": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
    "sdk_synchronize": (ctypes.c_int, [_vp]),
    "sdk_check_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _sz]),
    "sdk_solve_batch_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "sdk_timer_reset": (ctypes.c_int, [_vp]),
    "sdk_timer_read": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
}

# diagnostics the library exports beside the header (sudoku_hip.hip, "diagnostics (not in the header)")
DEBUG_SIGNATURES = {
    "sdk_debug_p32_list": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
}

_lib = None


class SudokuHipError(RuntimeError):
    pass


def load():
    """Load libsudoku_hip.so (once). Raises if it is missing: no CPU fallback exists."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SudokuHipError(
            f"{LIB_PATH} not found: build it with `make -C distributed_sudoku_solver_amd/csrc` "
            "or `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(LIB_PATH)
    # a library named by SDK_LIB_PATH (dev A/B builds of older commits) may predate newer
    # entry points; the in-tree library must export every one
    override = "SDK_LIB_PATH" in os.environ
    for name, (res, args) in SIGNATURES.items():
        if override and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in DEBUG_SIGNATURES.items():
        if override and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != SDK_OK:
        msg = load().sdk_last_error()
        msg = msg.decode() if msg else ""
        raise SudokuHipError(f"{what} failed ({rc}): {msg}")
    return rc
