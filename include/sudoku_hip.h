/*
 * sudoku_hip.h -- C-ABI of libsudoku_hip.so, the MI355X (gfx950) Sudoku engine.
 *
 * The reference (jsturm-11/distributed_sudoku_solver) has no FFI: its hot path
 * is two Python call contracts, which this ABI replaces (see INTEGRATION.md for
 * the ctypes binding the reference side would add):
 *
 *   DHTNode.solve_sudoku(puzzle, uuid, arr=range(1,10)) -> bool
 *       DHT_Node.py:474-538 (twin main.py:301-354), with find_next_empty
 *       utils.py:14-25, is_valid utils.py:27-56 and the TASK digit range that
 *       split_array_in_middle (utils.py:1-9) produces.
 *       -> sdk_solve_batch / sdk_solve_batch_dev
 *   Sudoku(grid).check() -> bool            sudoku.py:43-94
 *       -> sdk_check_batch / sdk_check_batch_dev
 *   (no reference counterpart: is this board that board under the Sudoku symmetries?)
 *       -> sdk_canonical_batch
 *   (no reference counterpart)
 *       -> sdk_count_solutions
 *   (no reference counterpart: a batch's verdicts, the technique a board needs,
 *   and inside the search level the number of single-cell backdoors)
 *       -> sdk_classify_batch, sdk_grade_batch, sdk_rate_batch, sdk_subsets_batch, sdk_fish_batch,
 *          sdk_wings_batch, sdk_chains_batch
 *       -> sdk_generate_puzzles, sdk_generate_graded, sdk_generate_rated,
 *          sdk_generate_subsets, sdk_generate_fish, sdk_generate_wings, sdk_generate_chains,
 *          sdk_minimize_level_batch, sdk_generate_level
 *   DFS subtree split across ring nodes (NEEDWORK/TASK, DHT_Node.py:491-510,
 *   225-250; utils.py:1-9) -- within one node of GPUs:
 *       -> sdk_frontier_* + sdk_comm_* (RCCL over xGMI)
 *
 * Conventions
 *   - Boards are uint8_t[81], row-major, 0 = empty, 1..9 = given digit,
 *     10..255 = an out-of-domain given that (as in the reference, where only
 *     `== guess` comparisons happen) never conflicts with a digit.
 *   - Every function returns SDK_OK (0) or a negative SDK_E* code; the message
 *     of the last failure on the calling thread is sdk_last_error().  No C++
 *     exception and no abort() crosses this boundary.
 *   - An sdk_ctx binds one HIP device and one HIP stream.  Calls on one context
 *     are serialised by an internal mutex; distinct contexts may be used from
 *     different threads concurrently.
 *   - Host-pointer calls are synchronous.  *_dev calls take device pointers,
 *     enqueue on the context stream and return immediately (sdk_synchronize).
 *     Device boards must be 16-byte aligned.
 */
#ifndef SUDOKU_HIP_H
#define SUDOKU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDK_ABI_VERSION 2   /* 2: sdk_solve_batch_ex, frontier records, p2p send/recv; version 2 */
                            /* also gained sdk_classify_batch[_dev] and sdk_minimize_batch[_dev]  */
                            /* and sdk_generate_grids[_dev] / sdk_generate_puzzles[_dev]          */
                            /* and sdk_grade_batch[_dev] and sdk_generate_graded[_dev]            */
                            /* and sdk_rate_batch[_dev] and sdk_generate_rated[_dev]              */
                            /* and sdk_subsets_batch[_dev] and sdk_generate_subsets[_dev]         */
                            /* and sdk_minimize_level_batch[_dev], sdk_generate_level[_dev]       */
                            /* and sdk_select_rows_dev                                            */
                            /* and sdk_canonical_batch[_dev]                                      */
                            /* and sdk_fish_batch[_dev] and sdk_generate_fish[_dev]               */
                            /* and sdk_wings_batch[_dev] and sdk_generate_wings[_dev]             */
                            /* and sdk_chains_batch[_dev] and sdk_generate_chains[_dev]           */
                            /* (new symbols only: nothing a version-2 caller uses changed)        */

/* return codes */
#define SDK_OK        0
#define SDK_EINVAL   -1   /* bad argument */
#define SDK_EHIP     -2   /* HIP runtime failure (message in sdk_last_error) */
#define SDK_ENOMEM   -3   /* device or host allocation failed */
#define SDK_ECOMM    -4   /* RCCL failure (message in sdk_last_error) */

/* per-board solve status (int8_t) */
#define SDK_SOLVED        1   /* out = lexicographically first completion          */
#define SDK_UNSOLVABLE    0   /* out = input (the reference restores the grid)     */
#define SDK_BUDGET_HIT   -2   /* node budget exhausted; out = input                */
#define SDK_MULTIPLE 2   /* classify only: at least two completions; out = input */

/* check verdict bits (uint8_t) */
#define SDK_CHECK_OK        1u  /* intended Sudoku.check(): all 27 units pass     */
#define SDK_CHECK_RAW_NAMEERROR 2u /* reference check() would raise NameError      */
                                   /* (sudoku.py:68): rows ok, cols ok, box00 sum 45 */

/* options for sdk_set_option */
#define SDK_OPT_ORDER        1  /* SDK_ORDER_* (default LEX)                           */
#define SDK_OPT_NODE_BUDGET  2  /* max search nodes per board, 0 = unlimited          */
#define SDK_OPT_WAVES_PER_CU 3  /* solver residency, 1..32 (default 32)               */
#define SDK_OPT_CHECK_BLOCKS_PER_CU 4 /* checker grid = CUs x this, 1..16 (default 3)  */
#define SDK_OPT_WORK_COUNTER 5  /* what solve `work` counts: SDK_WORK_* (default nodes) */
#define SDK_OPT_DEVICE_CUS   6  /* read-only: compute units of the context's GPU        */
#define SDK_OPT_SOLVER       7  /* solve kernel: SDK_SOLVER_* (default QUAD)             */
#define SDK_OPT_WAVES_PER_CU2 8 /* grid of the HALFWAVE / QUAD solver per CU, 1..32 (default 28) */
#define SDK_OPT_CHECK_VARIANT 9 /* checker tile pipeline: SDK_CHECK_* (default REG1) */
#define SDK_OPT_SOLVE_CHUNK  10  /* boards per solver dequeue, 0 = automatic (default)  */
#define SDK_OPT_TIMING       11  /* 1 = bracket every kernel with HIP events for        */
                                 /* sdk_timer_read (default 0: no events are created)    */
#define SDK_OPT_TIMER_EVENTS 12  /* read-only: HIP event pairs the context holds         */
#define SDK_OPT_LOCKED       13  /* QUAD solver: locked-candidates pass (pointing /      */
                                 /* claiming) at propagation fixpoints before branching: */
                                 /* 0 never, 1 at the root node only (default), 2 at     */
                                 /* every node; same answers, fewer search nodes         */
#define SDK_OPT_XCD_HEADS    14  /* QUAD solver: 1 = one dequeue head per XCD segment of */
                                 /* the batch (default), 0 = one shared head             */
#define SDK_OPT_DONATE       15  /* QUAD solver (LEX or MRV_UNIQUE order): phased solve  */
                                 /* with subtree donation.  1 (default) or a split       */
                                 /* budget >= 2: every board first gets at most that     */
                                 /* many search nodes (1: 128); the boards that need     */
                                 /* more are solved again by the donation kernel, where  */
                                 /* idle waves take a heavy board's shallowest untried   */
                                 /* branches.  Same boards and statuses; `work` adds up  */
                                 /* both phases and the board's parts.  0 = off: one     */
                                 /* launch, every board searched by one slot             */
#define SDK_OPT_DONATED      16  /* read-only: branches handed to idle waves by the last */
                                 /* solve's donation phase (waits for it)                */
#define SDK_OPT_SPLIT_BOARDS 17  /* read-only: boards the last solve passed to its       */
                                 /* donation phase                                       */
#define SDK_OPT_DONATE_MODE  18  /* the donation phase's order: 1 (default) exhaustive:  */
                                 /* MRV, at most two completions per board (a unique one */
                                 /* is the lex-first), boards with several are solved    */
                                 /* again in LEX with donation; 0: LEX directly          */
#define SDK_OPT_LEX_BOARDS   19  /* read-only: boards of the last solve's donation phase */
                                 /* that needed the LEX re-solve                         */
#define SDK_OPT_DONATE_MAX   20  /* largest batch solved in phases with donation         */
                                 /* (default 2^19; 0 = any size): a larger batch is one  */
                                 /* launch, where its heavy boards are a small share of  */
                                 /* the time (1M minimal puzzles: the phases cost 6 %)   */
#define SDK_OPT_DN_FAULT     21  /* test only: 1 = idle waves of the donation kernel skip */
                                 /* writing their registration entry, so a donor's       */
                                 /* bounded wait for it runs out: the solve then fails   */
                                 /* with SDK_EHIP (every wait on another wave inside a   */
                                 /* launch is bounded and reports this way)              */
#define SDK_OPT_DONATE_HELPERS 22 /* waves of a donation launch per board it re-solves   */
                                 /* (plus 64; default 2, at most the resident grid)      */
#define SDK_OPT_DONATE_RESUME 23 /* 1 (default): a board the split phase stops resumes  */
                                 /* in the donation launch from its open subtrees (the   */
                                 /* split phase leaves its DFS stack); 0: it restarts    */
#define SDK_OPT_RESUMED      24  /* read-only: boards of the last phased solve resumed   */
                                 /* from their saved stacks (its last pass; waits)       */
#define SDK_OPT_PROP32       25  /* QUAD solver: 1 (default) = a batch is first run      */
                                 /* through bit-sliced root propagation (32 boards per   */
                                 /* half-wave: singles + locked candidates); boards it   */
                                 /* does not decide are searched by solve4 and scattered */
                                 /* back -- same answers and statuses.  Plain solves     */
                                 /* only (no masks, work counters or strided inputs)     */
#define SDK_OPT_PROP32_LC    26  /* ... a locked-candidates pass every N steps (low byte),  */
                                 /* the first after step F (N | F << 8; F = 0: after step */
                                 /* N); default 5 | 3 << 8: after steps 3, 8, 13, ...     */
#define SDK_OPT_PROP32_MIN   27  /* ... for batches of at least N boards (default 4096)   */
#define SDK_OPT_PROP32_UNDECIDED 28 /* read-only: boards the last solve's propagation pass */
                                 /* left to the search (waits)                           */
#define SDK_OPT_PROP32_HANDOVER 29 /* ... 1 (default): with no node budget the search     */
                                 /* starts from a board's propagated grid (same          */
                                 /* completions); 0: from its input                      */
#define SDK_OPT_PROP32_TAIL  30  /* ... live | step << 8: from `step` on, a 64-board     */
                                 /* group with at most `live` boards still open hands     */
                                 /* them to the search (0 = never)                       */
#define SDK_OPT_GEN_CAP      31  /* sdk_generate_*: a grid is kept iff its fill placed at   */
                                 /* most this many digits, 81..2^31-1 (default 2^20; the   */
                                 /* heaviest fill of 5 M grids placed 935)                  */

#define SDK_CHECK_REG1       0  /* 1 tile ahead, staged in VGPRs (check_kernel)        */
#define SDK_CHECK_REG2       1  /* 2 tiles ahead, VGPR ring (check_kernel_rr2)         */
#define SDK_CHECK_GLDS2      2  /* LDS-DMA ring of 2 tiles (check_kernel_glds<2>)      */
#define SDK_CHECK_GLDS3      3  /* LDS-DMA ring of 3 tiles (check_kernel_glds<3>)      */
#define SDK_CHECK_GLDS4      4  /* LDS-DMA ring of 4 tiles (check_kernel_glds<4>)      */
#define SDK_CHECK_WAVE1      5  /* per-wave 64-board tiles, no barrier, 1 ahead       */
#define SDK_CHECK_WAVE2      6  /* ... 2 tiles ahead per wave (check_kernel_wave<2>)   */

#define SDK_SOLVER_WAVE      0  /* one board per wavefront (solve_kernel)              */
#define SDK_SOLVER_HALFWAVE  1  /* two boards per wavefront, 27 lanes x 3 cells each   */
#define SDK_SOLVER_QUAD      2  /* four boards per wavefront: HALFWAVE's layout with two */
                                /* boards packed in the 16-bit halves of every word      */
#define SDK_SOLVER_LANE      3  /* one board per lane: the reference's naive DFS itself  */
                                /* (LDS-resident stack); `work` = the reference's        */
                                /* validations, SDK_OPT_NODE_BUDGET counts validations;  */
                                /* SDK_ORDER_LEX only; counts use WAVE                   */

#define SDK_WORK_NODES       0  /* search nodes (propagation fixpoints)                */
#define SDK_WORK_ROUNDS      1  /* propagation rounds (profiling)                      */
#define SDK_WORK_DEPTH       2  /* deepest DFS level reached (profiling, tests)         */

#define SDK_ORDER_MRV_UNIQUE 0  /* MRV search for <=2 solutions; lex re-search if >=2 */
#define SDK_ORDER_LEX        1  /* lowest-index branching after propagation            */

typedef struct sdk_ctx sdk_ctx;

int         sdk_abi_version(void);
const char *sdk_last_error(void);
int         sdk_device_count(int *count);

int sdk_create(int device, sdk_ctx **out);
int sdk_destroy(sdk_ctx *ctx);
int sdk_set_option(sdk_ctx *ctx, int key, int64_t value);
int sdk_get_option(sdk_ctx *ctx, int key, int64_t *value);

/* ---- host-pointer batch API (synchronous) ------------------------------- */

/* Replaces Sudoku.check() (sudoku.py:43-94) for n boards: verdict[i] gets
 * SDK_CHECK_* bits, evaluated with the reference's literal per-unit rule
 * `sum == 45 and len(set) == 9`. */
int sdk_check_batch(sdk_ctx *ctx, const uint8_t *boards, uint8_t *verdict, size_t n);

/* The same for int64 cells (the reference's check() takes any Python int):
 * |value| < 2^59 (else SDK_EINVAL), so a unit's sum is exact. */
int sdk_check_batch_i64(sdk_ctx *ctx, const int64_t *boards, uint8_t *verdict, size_t n);

/* Replaces DHTNode.solve_sudoku (DHT_Node.py:474-538) for n boards.
 *   first_cell_mask  nullable; bit d (1..9) = digit d may be tried at the
 *                    lowest-index empty input cell (the TASK `range`); NULL =
 *                    range(1,10) for every board.
 *   out              lexicographically first completion (= the reference's
 *                    row-major ascending-digit DFS result) when status == 1,
 *                    else a copy of the input.
 *   status           SDK_SOLVED / SDK_UNSOLVABLE / SDK_BUDGET_HIT.
 *   work             nullable; search nodes spent per board (engine counter, not
 *                    the reference's naive-DFS `validations`). */
int sdk_solve_batch(sdk_ctx *ctx, const uint8_t *in, const uint16_t *first_cell_mask,
                    uint8_t *out, int8_t *status, uint64_t *work, size_t n);

/* sdk_solve_batch with the node budget of THIS call (search nodes per board, 0 =
 * unlimited, SDK_BUDGET_CONTEXT = the context's SDK_OPT_NODE_BUDGET): callers that
 * share a context (several ring nodes on one GPU) bound their own launches without
 * touching the shared option.  A board that runs out is SDK_BUDGET_HIT -- never
 * SDK_UNSOLVABLE: its subtree is unexplored, not empty (the reference would still be
 * searching, DHT_Node.py:474-538).  Its launch ends anyway, so one hard board cannot
 * hold back the rest of its batch. */
#define SDK_BUDGET_CONTEXT UINT64_MAX
int sdk_solve_batch_budget(sdk_ctx *ctx, const uint8_t *in, const uint16_t *first_cell_mask,
                           uint8_t *out, int8_t *status, uint64_t *work, size_t n, uint64_t node_budget);

/* sdk_solve_batch_budget with this call's SDK_OPT_DONATE as well (SDK_DONATE_CONTEXT = the
 * context's; 0 = one launch, one slot per board; 1 or a split budget >= 2 = the phased
 * solve with subtree donation).  Threads sharing a context (ring nodes on one GPU, a node's
 * batch and search threads) pick the launch shape per call without touching the shared
 * option. */
#define SDK_DONATE_CONTEXT -1
int sdk_solve_batch_ex(sdk_ctx *ctx, const uint8_t *in, const uint16_t *first_cell_mask,
                       uint8_t *out, int8_t *status, uint64_t *work, size_t n, uint64_t node_budget,
                       int64_t donate);

/* Uniqueness verdicts for n boards: does board i have no completion, exactly one, or several?
 *   status  SDK_UNSOLVABLE (none), SDK_SOLVED (exactly one; out = that completion),
 *           SDK_MULTIPLE (at least two) or SDK_BUDGET_HIT.
 *   out     the input for every status but SDK_SOLVED.
 * The constraint is the solver's and sdk_count_solutions' own (givens never conflict with
 * givens, 10..255 are inert).  node_budget as in sdk_solve_batch_budget (SDK_BUDGET_CONTEXT =
 * the context's SDK_OPT_NODE_BUDGET).  Always the QUAD kernel, in one launch after the
 * propagation pass (SDK_OPT_PROP32*, as for a plain solve), whatever SDK_OPT_SOLVER,
 * SDK_OPT_ORDER and SDK_OPT_DONATE say; it changes no option.  Any n up to 2^31-1 (batches
 * above 2^24 boards run in slices of that many). */
int sdk_classify_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, size_t n,
                       uint64_t node_budget);

/* Difficulty grades for n boards: which solving technique does board i need?
 *
 * A board's candidate state is 81 sets: a given d in 1..9 is {d}, an empty cell {1..9}; a cell is
 * closed when exactly one candidate is left.  Three rules:
 *   N  naked singles      an open cell loses every digit that is the candidate of a closed cell
 *                         in one of its three units;
 *   H  hidden singles     an open cell keeps only the candidates that some unit of its holds in
 *                         no other cell, if it has any (two such candidates are both kept);
 *   L  locked candidates  pointing and claiming over the 54 box-line triads: a digit that a box
 *                         holds only in one line goes from the rest of the line, one that a line
 *                         holds only in one box goes from the rest of the box.
 * R1 = {N}, R2 = {N, H}, R3 = {N, H, L}; F_k(board) is the state in which no rule of R_k changes
 * anything.  The rules only remove candidates, never a digit of a completion, and a rule that can
 * fire stays able to fire (or becomes moot) after further removals, so F_k does not depend on the
 * order of application: the grade is a pure function of the board.
 *
 *   status  sdk_classify_batch's verdict: SDK_UNSOLVABLE, SDK_SOLVED, SDK_MULTIPLE or
 *           SDK_BUDGET_HIT; node_budget as there (SDK_BUDGET_CONTEXT = the context's).  The
 *           propagation steps are free: a budget only bounds the search of the boards they leave.
 *   out     as classify: the completion for SDK_SOLVED, else the input.
 *   level   uint8[n].  For a board with status SDK_SOLVED and clean givens (all in 0..9, none
 *           repeated in a unit): the smallest k in 1..3 for which every cell of F_k is closed
 *           (SDK_GRADE_NAKED / _HIDDEN / _LOCKED), or SDK_GRADE_SEARCH if there is none.
 *           SDK_GRADE_NONE for every other board -- a uniquely solvable board with an inert
 *           (10..255) or duplicated given included.
 *   open    uint8[n], nullable.  For a board of level SDK_GRADE_SEARCH the number of open cells of
 *           F_3 (what the techniques left to the search); 0 for every other board.
 * The search's node count is deliberately not part of the grade: it depends on the boards a
 * board shares a wave with.  The grading pass always runs, for any n, whatever SDK_OPT_PROP32*,
 * SDK_OPT_SOLVER, SDK_OPT_ORDER and SDK_OPT_DONATE say; the call changes no option.  Any n up to
 * 2^31-1 (slices of 2^24 boards); one span under SDK_OPT_TIMING. */
#define SDK_GRADE_NONE   0
#define SDK_GRADE_NAKED  1
#define SDK_GRADE_HIDDEN 2
#define SDK_GRADE_LOCKED 3
#define SDK_GRADE_SEARCH 4
int sdk_grade_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, uint8_t *level,
                    uint8_t *open, size_t n, uint64_t node_budget);

/* Ratings inside level SDK_GRADE_SEARCH: how many single-cell backdoors does a board have?
 *
 * Take a board of level SDK_GRADE_SEARCH: exactly one completion S, clean givens, F_3 not closed.
 * For an empty input cell c, child(c) is the board with S[c] written into c, and c is a backdoor
 * when every cell of F_3(child(c)) is closed: the one guess that lets the techniques finish.
 *   backdoors  uint8[n], required: the number of backdoor cells, 0..64 (a uniquely solvable board
 *              has at least 17 clues, so at most 64 empty cells).  0: no single right guess is
 *              enough, the board needs two.
 *   key        uint8[n], nullable: the lowest-index backdoor cell (0..80), SDK_RATE_NONE if none.
 * Both are SDK_RATE_NONE for every board of any other level (no probe is run for them), a board
 * whose search hit the node budget (level SDK_GRADE_NONE) included.
 * By the monotonicity argument above (the rules only remove, and a rule that can fire stays able
 * to): F_3 of a child does not depend on the schedule; a child built from the input, from F_3's
 * closed cells, or from any grid between the two has the same F_3; a cell already closed in F_3 is
 * never a backdoor (its child has the parent's F_3, which is open), so counting over the empty
 * cells and over the open cells of F_3 is the same; and a child holds S, so it is never refuted
 * and its givens are clean.  The rating is a pure function of the board.
 *   status, out, level, open  exactly sdk_grade_batch's, byte for byte, under every option and
 *              budget (open nullable).
 * The call is a grade call with one more stage per slice (rate32_kernel.h: all the probes of one
 * board are one group of the propagation pass, synthesised in registers -- no child is ever
 * written to memory).  It changes no option and leaves SDK_OPT_PROP32_UNDECIDED as a grade call
 * does; its result does not depend on SDK_OPT_PROP32_LC.  Any n up to 2^31-1 (slices of 2^24
 * boards); one span under SDK_OPT_TIMING. */
#define SDK_RATE_NONE 0xFFu
int sdk_rate_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, uint8_t *level,
                   uint8_t *open, uint8_t *backdoors, uint8_t *key, size_t n, uint64_t node_budget);

/* Subsets inside level SDK_GRADE_SEARCH: what do naked and hidden pairs, triples and quads leave open?
 *
 * Two more rules on the candidate sets and 27 units of N, H and L (sdk_grade_batch):
 *   naked S_k   k cells of a unit whose candidate sets have a union of at most k digits: every other
 *               cell of the unit loses those digits;
 *   hidden S_k  k digits that only k or fewer cells of a unit hold: those cells lose every other digit.
 * k = 1 of each is N and H.  R4 = R3 + {naked and hidden S_2, S_3, S_4}, and F_4 is its fixpoint.  Both
 * premises survive further removals and neither rule removes a digit of a completion, so the argument
 * above carries over: F_4 is one state whatever the order of application, a pure function of the
 * board.  A naked subset of k among a unit's m open cells removes what the hidden subset of the other
 * m - k digits removes; with m <= 9, sizes up to 4 on both sides cover every size.
 *   open4   uint8[n], required.  For a board of level SDK_GRADE_SEARCH the number of open cells of
 *           F_4, 0..64; 0: the subsets finish the board, no guess is needed.  SDK_SUBSETS_NONE for
 *           every board of any other level, a board whose search hit the node budget (level
 *           SDK_GRADE_NONE) included.
 *   status, out, level, open  exactly sdk_grade_batch's, byte for byte, under every option and
 *           budget (open nullable).
 * The call is a grade call with one more stage per slice (subsets_kernel.h: one level-4 board per
 * half-wave, one unit per lane, from the board's input row).  It changes no option and leaves
 * SDK_OPT_PROP32_UNDECIDED as a grade call does.  Any n up to 2^31-1 (slices of 2^24 boards); one span
 * under SDK_OPT_TIMING. */
#define SDK_SUBSETS_NONE 0xFFu
int sdk_subsets_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, uint8_t *level,
                      uint8_t *open, uint8_t *open4, size_t n, uint64_t node_budget);

/* Basic fish inside level SDK_GRADE_SEARCH: what do X-wings, swordfish and jellyfish leave open?
 *
 * On the candidate sets of sdk_grade_batch.  For a digit d, M_d is the 9 x 9 bit matrix whose row r holds
 * the columns c at which cell (r, c) still has candidate d; closed cells are included.
 *   row fish of size k     k rows of M_d whose union has at most k columns: every other row loses those
 *                          columns, that is, the cells lose candidate d;
 *   column fish of size k  the same on the transpose of M_d.
 * k = 1 is a hidden single of a line followed by N; k = 2, 3, 4 are X-wing, swordfish, jellyfish.  Finned,
 * sashimi and franken fish are not part of it.  R5 = R4 + {row and column fish of sizes 2..4, every
 * digit}, and F_5 is its fixpoint.  A fish removes no digit of a completion (Hall's condition on the
 * digit's places) and its premise survives further removals, so the argument above carries over: F_5 is
 * one state whatever the order of application, a pure function of the board.  A row fish of size k among
 * the m rows where d is not yet placed removes what the column fish of size m - k removes; with m <= 9,
 * sizes up to 4 on both orientations cover every size.
 *   open5   uint8[n], required.  For a board of level SDK_GRADE_SEARCH the number of open cells of
 *           F_5, 0..64; 0 with open4 > 0: the board needs a fish, and a fish is enough.  SDK_FISH_NONE for
 *           every board of any other level, a board whose search hit the node budget (level
 *           SDK_GRADE_NONE) included.
 *   open4   uint8[n], nullable: sdk_subsets_batch's column, byte for byte.
 *   status, out, level, open  exactly sdk_grade_batch's, byte for byte, under every option and
 *           budget (open nullable).
 * The call is a grade call with one more stage per slice, in the place of the subsets stage
 * (fish_kernel.h: one level-4 board per half-wave; the subsets stage's rounds to F_4, where open4 is
 * taken, then rounds in which nine lanes take a digit each).  It changes no option and leaves
 * SDK_OPT_PROP32_UNDECIDED as a grade call does.  Any n up to 2^31-1 (slices of 2^24 boards); one span
 * under SDK_OPT_TIMING. */
#define SDK_FISH_NONE 0xFFu
int sdk_fish_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, uint8_t *level,
                   uint8_t *open, uint8_t *open4, uint8_t *open5, size_t n, uint64_t node_budget);

/* Wings and simple colouring inside level SDK_GRADE_SEARCH: what do XY-wings, XYZ-wings and simple
 * colouring leave open?
 *
 * R6 = R5 + {W, C} on the grader's candidate sets.  F_6 is its fixpoint.  open6 is the number of open cells
 * of F_6 for a board of level SDK_GRADE_SEARCH.  For every other board open6 is SDK_WINGS_NONE = 0xFF,
 * budget hits included.
 *
 * W (wings).
 *   The pivot p is an open cell with 2 or 3 candidates P.
 *   The pincers q != r are bivalue cells, each sharing a unit with p, with candidate sets Q != R and
 *   Q & R a single digit z.
 *   XY-wing:  P == (Q | R) & ~z.  Every cell other than p, q, r that shares a unit with q and with r loses z.
 *   XYZ-wing: P == Q | R.  Every cell other than p, q, r that shares a unit with p, with q and with r
 *   loses z.
 * C (simple colouring, one digit at a time).
 *   The places of d are the cells that hold candidate d, closed cells included, as in M_d of the fish.
 *   A link is a unit with exactly two places.
 *   The links make a graph on the places.  Each connected component with at least one link is two-coloured.
 *   Wrap: if two places of one colour share a unit, every place of that colour loses d.
 *   Trap: a place outside the component that shares a unit with a place of each colour loses d.
 * Both rules remove no digit of a completion.  A premise that further removals break is taken over by
 * singles, so F_6 is one state whatever the order of application (tests/wings_model.py pins three orders on
 * data); the stage's order is a W + C pass from F_5, then F_5 again, until a pass changes nothing.
 *   open6   uint8[n], required.  0..64 for a board of level SDK_GRADE_SEARCH; 0 with open5 > 0: the board
 *           needs a wing or a colouring, and that is enough.
 *   open4, open5  uint8[n], nullable: sdk_fish_batch's columns, byte for byte.
 *   status, out, level, open  exactly sdk_grade_batch's, byte for byte, under every option and budget
 *           (open nullable).
 * The call is a grade call with one more stage per slice, in the place of the fish stage (wings_kernel.h:
 * the fish stage's layout and rounds to F_5, where open5 is taken, then wide rounds).  It changes no option
 * and leaves SDK_OPT_PROP32_UNDECIDED as a grade call does.  Any n up to 2^31-1; one span under
 * SDK_OPT_TIMING. */
#define SDK_WINGS_NONE 0xFFu
int sdk_wings_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, uint8_t *level,
                    uint8_t *open, uint8_t *open4, uint8_t *open5, uint8_t *open6, size_t n,
                    uint64_t node_budget);

/* Chains inside level SDK_GRADE_SEARCH: what do X-chains and XY-chains leave open?
 *
 * R7 = R6 + {X, Y} on the grader's candidate sets.  F_7 is its fixpoint.  open7 is the number of open cells
 * of F_7 for a board of level SDK_GRADE_SEARCH.  For every other board open7 is SDK_CHAINS_NONE = 0xFF,
 * budget hits included.
 *
 * X (X-chains, one digit d at a time).
 *   The places of d are the cells that hold candidate d, closed cells included, as in M_d of the fish and the
 *   colouring's places.  A link is a unit with exactly two places.
 *   For every open place s: ON starts as the other ends of the links through s.  Until ON stops growing, OFF
 *   is the places that share a unit with a cell of ON, and every link with exactly one end in OFF puts its
 *   other end into ON; s itself is never put into ON.
 *   For every t in ON either s or t holds d: every open cell that shares a unit with s and with t loses d.
 *   Skyscrapers, two-string kites, turbot fish and the colour trap are its short cases.
 * Y (XY-chains).
 *   For every bivalue cell s and each of its two digits z: a state (c, v) means "c is v"; the start state is
 *   (s, the other digit of s); from (c, v) the chain goes to every bivalue cell c2 != s that shares a unit
 *   with c and holds v, in the state (c2, the other digit of c2).
 *   For every reached state (c, z) with c != s either s or c holds z: every open cell that shares a unit with
 *   s and with c loses z.  XY-wings are the length-three case; remote pairs are included.
 * Both rules remove no digit of a completion.  A premise that further removals break becomes a single, so F_7
 * is one state whatever the order of application (tests/chains_model.py pins three orders on data); the
 * stage's order is an X + Y pass from F_6, both from one snapshot, then F_6 again, until a pass changes
 * nothing.  No chain removal touches a board before its open4, open5 and open6 are stored.
 *   open7   uint8[n], required.  0..64 for a board of level SDK_GRADE_SEARCH; 0 with open6 > 0: the board
 *           needs a chain, and a chain is enough.
 *   open4, open5, open6  uint8[n], nullable: sdk_wings_batch's columns, byte for byte.
 *   status, out, level, open  exactly sdk_grade_batch's, byte for byte, under every option and budget
 *           (open nullable).
 * The call is a grade call with one more stage per slice, in the place of the wings stage (chains_kernel.h:
 * the wings stage's layout and rounds to F_6, where open6 is taken, then chain rounds).  It changes no option
 * and leaves SDK_OPT_PROP32_UNDECIDED as a grade call does.  Any n up to 2^31-1; one span under
 * SDK_OPT_TIMING. */
#define SDK_CHAINS_NONE 0xFFu
int sdk_chains_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *out, int8_t *status, uint8_t *level,
                     uint8_t *open, uint8_t *open4, uint8_t *open5, uint8_t *open6, uint8_t *open7, size_t n,
                     uint64_t node_budget);

/* Canonical forms for n boards: are two boards the same puzzle under the Sudoku symmetries?
 *
 * A symmetry is a pair (g, rho).  g is a permutation of the cells 0..80 (new cell -> old cell) made of a
 * row permutation and a column permutation that keep bands and stacks, and optionally the transposition:
 * 2 * 6^8 = 3,359,232 cell maps.  rho is a permutation of 1..9 with rho[0] = 0.
 * image(B)[c] = rho[B[g[c]]].
 *
 * A board is eligible when sdk_classify_batch gives it SDK_SOLVED and its givens are clean, as
 * sdk_grade_batch defines clean -- equivalently its completion S is a valid grid (a completion keeps a
 * duplicated or inert given).  For an eligible board P with completion S:
 *   M     the canonical solution: the lexicographically smallest image(S) over all symmetries, 81 bytes
 *         row-major.  Its first row is 1..9.
 *   C     the canonical puzzle: the lexicographically smallest image(P), 0 = empty sorting first, over the
 *         symmetries with image(S) == M.  Two eligible boards are equivalent iff their C are equal: the
 *         symmetries that take S' = T(S) to M are those that take S to M composed with the inverse of T,
 *         so both boards minimise over the same set of images.
 *   ties  the number of cell maps g for which some rho gives image(S) == M: the order of the
 *         automorphism group of S, 1 for almost every grid, at most 648.
 *   the returned symmetry: among those that attain C, the one of lowest candidate index
 *         k = (t * 9 + r0) * 1296 + q.  t = 1: G is the transpose of S, else G = S; r0 is the row of G
 *         that becomes row 0; q = ((s * 6 + i0) * 6 + i1) * 6 + i2 arranges the columns over the six
 *         permutations P3 = 012, 021, 102, 120, 201, 210: image column j is column
 *         3 * P3[s][j / 3] + P3[i_(j / 3)][j % 3] of G.  With image rows rr and columns cc of G,
 *         g[9 i + j] = 9 * rr[i] + cc[j] for t = 0 and 9 * cc[j] + rr[i] for t = 1.
 * The result is a pure function of the board, and the canonical form of C is C under the identity.
 *
 * The reduction behind the candidates: given (t, r0, q), rho is forced by "row 0 of the image is 1..9", and
 * the rest of the minimal image by sorting -- the rows of a band differ in column 0, so row 0's band-mates
 * follow in ascending order of their relabelled first cell, each other band is sorted the same way, and
 * the band that holds the smaller first cell comes first.  M is the minimum over 2 * 9 * 1296 = 23,328
 * candidates, and every symmetry with image M is exactly one of them.
 *
 *   canon     uint8[n][81], required: C; the input for an ineligible board.
 *   status    required: exactly sdk_classify_batch's, under every option and budget (node_budget as there).
 *   solution  uint8[n][81], nullable: M for an eligible board, classify's `out` for every other.
 *   gather    uint8[n][81], nullable: g;  relabel  uint8[n][10], nullable: rho;  ties  uint16[n], nullable.
 *             An ineligible board (no or several completions, budget hit, unclean givens) has the identity
 *             gather 0..80, the identity relabel 0..9 and ties 0.
 * The classify path, then one launch of canon_kernel.h per slice (one board per wave).  It changes no
 * option and leaves SDK_OPT_PROP32_UNDECIDED as a classify call does.  Any n up to 2^31-1 (slices of 2^24
 * boards); one span under SDK_OPT_TIMING. */
int sdk_canonical_batch(sdk_ctx *ctx, const uint8_t *in, uint8_t *canon, uint8_t *solution, int8_t *status,
                        uint8_t *gather, uint8_t *relabel, uint16_t *ties, size_t n, uint64_t node_budget);

/* Greedy clue removal for n boards.  order is uint8[n][81]; row i is a permutation of 0..80, the
 * cell order in which board i's clues are tried (anything else: SDK_EINVAL).  Per board:
 *   status[i] = sdk_classify_batch's verdict of the input (no budget);
 *   if it is not SDK_SOLVED, out[i] = the input; otherwise for q = 0..80 the cell order[i][q],
 *   if non-zero, is cleared, and put back unless the board still has exactly one completion.
 * out[i] is the result: a pure function of (board, order row), and a minimal puzzle (no clue
 * can go) with the input's completion.  A "clue" is any non-zero cell; an inert given goes,
 * because removing it changes no completion.  81 rounds of one streaming kernel and a classify
 * launch each, enqueued without the host.  Any n up to 2^31-1 (slices of 2^24 boards). */
int sdk_minimize_batch(sdk_ctx *ctx, const uint8_t *in, const uint8_t *order, uint8_t *out,
                       int8_t *status, size_t n);

/* Random complete grids, made on the GPU (generate_kernel.h, one grid per lane).  Row i is stream
 * index k = first + i of `seed`: the grid a randomised row-major backtracking fill gives under the
 * splitmix64 stream of (seed, k) -- a pure function of (seed, k), the grid of the host generator
 * (csrc/gen_minimal.c gen_grid_one; synth.minimal_grids), byte for byte.
 *   grids       uint8[n][81].
 *   order       nullable, uint8[n][81]: the permutation of 0..80 the same stream draws after the
 *               fill -- the cell order in which the host generator removes clues.
 *   placements  nullable, uint32[n]: digits the fill wrote into cells (81 = it never took one back).
 * A grid whose fill places more than SDK_OPT_GEN_CAP digits is not kept: its row is 81 zeros and its
 * count 0xFFFFFFFF.  Its order row is the stream's all the same (the order continues the stream
 * where the fill leaves it, so the fill is still followed to its end); the fill itself, and with it
 * every loop of the kernel, stops at max(SDK_OPT_GEN_CAP, 2^20) placements, after which the order is
 * drawn from the stream as it stands.  first + n must not overflow; any n up to 2^31-1 (slices of
 * 2^24 rows).  Under SDK_OPT_TIMING a call records one span, whatever its slices. */
int sdk_generate_grids(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n, uint8_t *grids,
                       uint8_t *order, uint32_t *placements);

/* Minimal unique puzzles, made on the GPU: the grids of sdk_generate_grids, then sdk_minimize_batch
 * over them in their own removal orders (kept in a context buffer), all enqueued without the host.
 * Row i is the host generator's puzzle first + i (gen_minimal_one; synth.make_minimal) with its
 * grid, byte for byte.
 *   puzzles  uint8[n][81];  grids  uint8[n][81], the puzzles' completions;
 *   status   the minimiser's: SDK_SOLVED for every grid that was kept.  A grid that was not (see
 *            SDK_OPT_GEN_CAP) is 81 zeros: SDK_MULTIPLE, and its puzzle row is 81 zeros too.
 * All three are required.  Under SDK_OPT_TIMING a call records one span (the generate launches and
 * the minimise rounds of all its slices). */
int sdk_generate_puzzles(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n, uint8_t *puzzles,
                         uint8_t *grids, int8_t *status);

/* Clue removal that stops at a technique level.  R_level is sdk_grade_batch's technique set of that
 * level (naked singles; + hidden singles; + locked candidates) and "R_level closes a board" means its
 * fixpoint F_level has every cell closed -- such a board has exactly one completion, so no search is
 * involved.  level must be SDK_GRADE_NAKED..SDK_GRADE_LOCKED, else SDK_EINVAL.  order as for
 * sdk_minimize_batch (rows that are not permutations of 0..80: SDK_EINVAL).  Per board:
 *   board i is eligible when its givens are clean (each 1..9, none twice in a unit) and R_level
 *   closes it: status[i] = 1.  Every other board -- inert or duplicated givens, no or several
 *   completions, one that needs more than R_level -- has status[i] = 0 and out[i] = the input, byte
 *   for byte;
 *   for an eligible board and q = 0..80 the cell order[i][q], if non-zero, is cleared, and put back
 *   unless R_level still closes the board without it.
 * out[i] is the result: a pure function of (board, order row, level); sdk_grade_batch gives it a
 * level <= `level`, and none of its clues can go under R_level (removing a given only enlarges every
 * candidate set, so a removal that failed in its round fails at every later state: one pass over
 * the order is enough).  One launch per slice: a group of 64 boards runs its eligibility test and
 * its 81 rounds inside reduce32_kernel.h.  out may be in.  Any n up to 2^31-1 (slices of 2^24
 * boards); one span under SDK_OPT_TIMING; no option is changed. */
int sdk_minimize_level_batch(sdk_ctx *ctx, const uint8_t *in, const uint8_t *order, int level,
                             uint8_t *out, int8_t *status, size_t n);

/* Level-minimal puzzles, made on the GPU: the grids of sdk_generate_grids, then
 * sdk_minimize_level_batch over them in their own removal orders (kept in a context buffer), all
 * enqueued without the host.  Row i is a pure function of (seed, first + i, level).
 *   puzzles  uint8[n][81];  grids  uint8[n][81], the puzzles' completions;
 *   status   the minimiser's: 1 for every grid that was kept.  A grid that was not (see
 *            SDK_OPT_GEN_CAP) is 81 zeros: status 0, and its puzzle row is 81 zeros too.
 * All three are required; level as above.  One span under SDK_OPT_TIMING. */
int sdk_generate_level(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n, int level,
                       uint8_t *puzzles, uint8_t *grids, int8_t *status);

/* Puzzles of a requested grade: the first n puzzles of the stream, from index `first` on, that match
 * a predicate -- generated, graded and selected on the GPU; only the matches leave the device.
 *
 * Candidate k is row k of sdk_generate_puzzles(seed, ...).  Its level and open count are the ones
 * sdk_grade_batch gives that puzzle with no node budget (the context's SDK_OPT_NODE_BUDGET has no
 * effect, as in the minimiser); its clue count is the number of its non-zero cells.  Candidate k is a
 * hit when its generator status is SDK_SOLVED, bit `level` of level_mask is set and
 * clues_lo <= clues <= clues_hi.  A grid dropped by SDK_OPT_GEN_CAP is a row of zeros of level
 * SDK_GRADE_NONE: never a hit.
 *
 * The window is [first, first + max_scan).  *found = min(n, hits in the window).  For j < *found, with
 * k_j the j-th smallest hit: puzzles[j] and grids[j] are its puzzle and its completion, level[j] and
 * open[j] its grade, index[j] = k_j.  Rows j >= *found are not written, in either form (the host form
 * copies *found rows back).  *scanned = k_(n-1) - first + 1 when *found == n, else max_scan: a number
 * of the result, not of the work done.  The result is a pure function of (seed, first, n, level_mask,
 * clues_lo, clues_hi, max_scan, SDK_OPT_GEN_CAP).
 *
 *   level_mask  a non-empty set of bits SDK_GRADE_NAKED..SDK_GRADE_SEARCH (1..4), else SDK_EINVAL;
 *   clues_lo <= clues_hi <= 81;  max_scan >= 1, and first + max_scan must not overflow;
 *   n           as in the other generate calls (at most 2^31-1); n == 0 launches nothing and gives
 *               *found = *scanned = 0;
 *   chunk       stream indices per round, 0 = automatic, or 1..2^24.  The window is scanned in rounds
 *               (generate, grade, then three selection launches: select_kernel.h) until n hits are
 *               found or it ends; the last round may look past `scanned`.  chunk changes speed and
 *               work memory (about 250 bytes per index of a round), never a byte of the result.
 *               Automatic: the first round is 4 n indices; a later one is what the hit rate so far
 *               asks for the missing hits, plus a quarter (twice the round before while there was no
 *               hit yet); every automatic round is within 4096..2^20 indices and the window.
 *   puzzles, grids  uint8[n][81], required;  level, open  uint8[n], index  uint64[n], scanned: nullable;
 *   found       required.
 * The call holds the context for all its rounds and reads one 8-byte count back per round, its only
 * host round trip.  It changes no option; under SDK_OPT_TIMING it records one span. */
int sdk_generate_graded(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                        uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                        uint64_t max_scan, uint64_t chunk,
                        uint8_t *puzzles, uint8_t *grids, uint8_t *level, uint8_t *open,
                        uint64_t *index, uint64_t *found, uint64_t *scanned);

/* Puzzles of a requested grade and rating: sdk_generate_graded with one more condition.  Candidate k
 * is a hit when it is a hit of sdk_generate_graded(level_mask, clues_lo, clues_hi) and, if its level
 * is SDK_GRADE_SEARCH, backdoors_lo <= backdoors <= backdoors_hi (sdk_rate_batch's count with no
 * node budget).  Candidates of levels 1..3 are not filtered by the range.
 *   backdoors_lo <= backdoors_hi <= 64, else SDK_EINVAL;
 *   backdoors, key  uint8[n], nullable: the hits' ratings (SDK_RATE_NONE for levels 1..3).
 * Everything else is sdk_generate_graded's: the window, found, scanned, chunk (speed only), the
 * purity of the result (now also a function of the range), one 8-byte readback per round, one span.
 * A round grades with the rate stage; when level_mask lacks SDK_GRADE_SEARCH the stage is skipped.
 * With the range (0, 64) the shared outputs are sdk_generate_graded's, byte for byte. */
int sdk_generate_rated(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                       uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                       uint32_t backdoors_lo, uint32_t backdoors_hi,
                       uint64_t max_scan, uint64_t chunk,
                       uint8_t *puzzles, uint8_t *grids, uint8_t *level, uint8_t *open,
                       uint8_t *backdoors, uint8_t *key,
                       uint64_t *index, uint64_t *found, uint64_t *scanned);

/* Puzzles of a requested grade and subsets count: sdk_generate_graded with one more condition.
 * Candidate k is a hit when it is a hit of sdk_generate_graded(level_mask, clues_lo, clues_hi) and, if
 * its level is SDK_GRADE_SEARCH, open4_lo <= open4 <= open4_hi (sdk_subsets_batch's count with no node
 * budget).  Candidates of levels 1..3 are not filtered by the range.  (0, 0) with level_mask =
 * 1 << SDK_GRADE_SEARCH: the puzzles beyond locked candidates that need no guess.
 *   open4_lo <= open4_hi <= 64, else SDK_EINVAL;
 *   open4  uint8[n], nullable: the hits' counts (SDK_SUBSETS_NONE for levels 1..3).
 * Everything else is sdk_generate_graded's: the window, found, scanned, chunk (speed only), the
 * purity of the result (now also a function of the range), one 8-byte readback per round, one span.
 * A round grades with the subsets stage; when level_mask lacks SDK_GRADE_SEARCH the stage is skipped.
 * With the range (0, 64) the shared outputs are sdk_generate_graded's, byte for byte. */
int sdk_generate_subsets(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                         uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                         uint32_t open4_lo, uint32_t open4_hi,
                         uint64_t max_scan, uint64_t chunk,
                         uint8_t *puzzles, uint8_t *grids, uint8_t *level, uint8_t *open,
                         uint8_t *open4,
                         uint64_t *index, uint64_t *found, uint64_t *scanned);

/* Puzzles of a requested grade, subsets count and fish count: sdk_generate_graded with two more
 * conditions.  Candidate k is a hit when it is a hit of sdk_generate_graded(level_mask, clues_lo,
 * clues_hi) and, if its level is SDK_GRADE_SEARCH, open4_lo <= open4 <= open4_hi and open5_lo <= open5 <=
 * open5_hi (sdk_fish_batch's counts with no node budget).  Candidates of levels 1..3 are not filtered by
 * the ranges.  open4 = (1, 64), open5 = (0, 0) with level_mask = 1 << SDK_GRADE_SEARCH: the puzzles that
 * need a fish, and for which a fish is enough.
 *   open4_lo <= open4_hi <= 64 and open5_lo <= open5_hi <= 64, else SDK_EINVAL;
 *   open4, open5  uint8[n], nullable: the hits' counts (0xFF for levels 1..3).
 * Everything else is sdk_generate_graded's: the window, found, scanned, chunk (speed only), the
 * purity of the result (now also a function of the ranges), one 8-byte readback per round, one span.
 * A round grades with the fish stage; when level_mask lacks SDK_GRADE_SEARCH the stage is skipped.
 * With both ranges (0, 64) the shared outputs are sdk_generate_graded's, byte for byte. */
int sdk_generate_fish(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                      uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                      uint32_t open4_lo, uint32_t open4_hi, uint32_t open5_lo, uint32_t open5_hi,
                      uint64_t max_scan, uint64_t chunk,
                      uint8_t *puzzles, uint8_t *grids, uint8_t *level, uint8_t *open,
                      uint8_t *open4, uint8_t *open5,
                      uint64_t *index, uint64_t *found, uint64_t *scanned);

/* Puzzles of a requested grade, fish count and wings count: sdk_generate_graded with two more conditions.
 * Candidate k is a hit when it is a hit of sdk_generate_graded(level_mask, clues_lo, clues_hi) and, if its
 * level is SDK_GRADE_SEARCH, open5_lo <= open5 <= open5_hi and open6_lo <= open6 <= open6_hi
 * (sdk_wings_batch's counts with no node budget).  Candidates of levels 1..3 are not filtered by the ranges.
 * open5 = (1, 64), open6 = (0, 0) with level_mask = 1 << SDK_GRADE_SEARCH: the puzzles that need a wing or a
 * colouring, and for which that is enough.
 *   open5_lo <= open5_hi <= 64 and open6_lo <= open6_hi <= 64, else SDK_EINVAL;
 *   open5, open6  uint8[n], nullable: the hits' counts (0xFF for levels 1..3).
 * Everything else is sdk_generate_graded's.  A round grades with the wings stage; when level_mask lacks
 * SDK_GRADE_SEARCH the stage is skipped.  With open6 = (0, 64) the rows are sdk_generate_fish's with
 * open4 = (0, 64); with both ranges (0, 64) the shared outputs are sdk_generate_graded's, byte for byte. */
int sdk_generate_wings(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                       uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                       uint32_t open5_lo, uint32_t open5_hi, uint32_t open6_lo, uint32_t open6_hi,
                       uint64_t max_scan, uint64_t chunk,
                       uint8_t *puzzles, uint8_t *grids, uint8_t *level, uint8_t *open,
                       uint8_t *open5, uint8_t *open6,
                       uint64_t *index, uint64_t *found, uint64_t *scanned);

/* Puzzles of a requested grade, wings count and chains count: sdk_generate_graded with two more conditions.
 * Candidate k is a hit when it is a hit of sdk_generate_graded(level_mask, clues_lo, clues_hi) and, if its
 * level is SDK_GRADE_SEARCH, open6_lo <= open6 <= open6_hi and open7_lo <= open7 <= open7_hi
 * (sdk_chains_batch's counts with no node budget).  Candidates of levels 1..3 are not filtered by the ranges.
 * open6 = (1, 64), open7 = (0, 0) with level_mask = 1 << SDK_GRADE_SEARCH: the puzzles that need a chain, and
 * for which a chain is enough.
 *   open6_lo <= open6_hi <= 64 and open7_lo <= open7_hi <= 64, else SDK_EINVAL;
 *   open6, open7  uint8[n], nullable: the hits' counts (0xFF for levels 1..3).
 * Everything else is sdk_generate_graded's.  A round grades with the chains stage; when level_mask lacks
 * SDK_GRADE_SEARCH the stage is skipped.  With open7 = (0, 64) the rows are sdk_generate_wings' with
 * open5 = (0, 64); with both ranges (0, 64) the shared outputs are sdk_generate_graded's, byte for byte. */
int sdk_generate_chains(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                        uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                        uint32_t open6_lo, uint32_t open6_hi, uint32_t open7_lo, uint32_t open7_hi,
                        uint64_t max_scan, uint64_t chunk,
                        uint8_t *puzzles, uint8_t *grids, uint8_t *level, uint8_t *open,
                        uint8_t *open6, uint8_t *open7,
                        uint64_t *index, uint64_t *found, uint64_t *scanned);

/* The worklist step of a resumable lex-first search of a board whose solve hit the
 * budget (distributed_sudoku_solver_amd/search.py; the in-node form of handing a
 * subtree on, DHT_Node.py:491-510): expand n boards -- board i with first-cell mask
 * first_cell_masks[i] (nullable = range(1,10) everywhere) -- breadth-first in the
 * reference's DFS order (lowest open cell after propagation, digits ascending, solved
 * boards kept, contradicted ones dropped), at least one level deep and on until the
 * frontier holds >= target boards or nothing branches.  The frontier goes to `out`
 * (*out_n boards, uint8[*out_n][81]); children keep their parents' order, so board k's
 * completions all precede board k+1's in lex order, and the union of their completions
 * is exactly the seeds'.  cap = capacity of `out` in boards; cap >= 9 * max(n, target)
 * always suffices (SDK_EINVAL if the frontier does not fit). */
int sdk_expand_boards(sdk_ctx *ctx, const uint8_t *boards, const uint16_t *first_cell_masks, size_t n,
                      uint64_t target, uint8_t *out, size_t cap, uint64_t *out_n);

/* Counts completions of one board (same constraint as the solver), stopping
 * at `limit` (0 = no limit).  status as above. */
int sdk_count_solutions(sdk_ctx *ctx, const uint8_t *board, uint64_t limit,
                        uint64_t *count, int8_t *status);

/* Multi-GPU form (one context per GPU, one call per rank): every rank expands
 * the same deterministic breadth-first frontier of `board` and counts the
 * subtrees of its contiguous slice; rank 0 also counts the completions met
 * during expansion.  The sum of `count` over ranks is the total (callers
 * all-reduce it).  frontier_size (nullable) = boards in the split frontier. */
int sdk_count_solutions_slice(sdk_ctx *ctx, const uint8_t *board, uint64_t limit, int rank, int world,
                              uint64_t *count, uint64_t *frontier_size, int8_t *status);

/* ---- multi-GPU searches of ONE board ---------------------
 *
 * Every rank builds the same deterministic breadth-first frontier of the board
 * on its own GPU (no exchange), works on its share of it, and combines results
 * with RCCL collectives on device memory, enqueued on the context stream.
 *
 *   SDK_FRONTIER_COUNT  MRV branching; completions met while expanding are
 *                       counted in *leaves (identical on every rank) and dropped.
 *   SDK_FRONTIER_FIRST  lowest-open-cell branching, digits ascending, solved
 *                       boards kept: frontier index order = the reference's DFS
 *                       order (DHT_Node.py:522), so the first frontier board with
 *                       a completion holds the reference's answer.  The digit
 *                       mask (nullable) restricts the lowest empty cell of
 *                       `board`, like a TASK `range`.
 * target = frontier size to reach (0 = 8 boards per resident solver wave). */
#define SDK_FRONTIER_COUNT 0
#define SDK_FRONTIER_FIRST 1
int sdk_frontier_build(sdk_ctx *ctx, const uint8_t *board, const uint16_t *first_cell_mask, int mode,
                       uint64_t target, uint64_t *size, uint64_t *leaves);

/* Count mode: completions below frontier boards first, first+step, ... < end,
 * written to d_result (device, 2 x uint64): {count, boards that hit the node
 * budget}.  The per-board search stops the batch once count >= limit (0 = none). */
/* Second, rank-local stage of a frontier split (count mode): keep boards first,
 * first+step, ... of the frontier built last and expand them further on this device
 * until they number `target` (or nothing branches); *size / *leaves = the refined
 * frontier and the completions met while refining (this rank's alone).  A rank can so
 * take its share of a small replicated frontier and grow it locally, instead of every
 * rank expanding a world-sized frontier. */
int sdk_frontier_refine(sdk_ctx *ctx, uint64_t first, uint64_t step, uint64_t target, uint64_t *size,
                        uint64_t *leaves);
int sdk_frontier_count_dev(sdk_ctx *ctx, uint64_t first, uint64_t step, uint64_t end, uint64_t limit,
                           void *d_result);

/* First mode: solve frontier boards [lo, hi) (each to its lex-first completion)
 * and write the lowest index whose status is not SDK_UNSOLVABLE to d_found
 * (device int64; INT64_MAX if none) and that board's output + status to d_best
 * (device, 82 bytes: board[81], int8 status).  d_found is also the launch's found
 * word: a board that ends solved or at the node budget lowers it, and boards above
 * it stop at their next check ("shards whose index is above the
 * minimum may stop"), so the launch ends once every board below the lowest hit is
 * decided.  The result is the one a launch that solves every board would give. */
int sdk_frontier_first_dev(sdk_ctx *ctx, uint64_t lo, uint64_t hi, void *d_found, void *d_best);

/* Frontier records, for moving live subtrees between ranks (SURVEY §8(e) rebalance; the
 * device form of the reference handing a partial board on mid-search, DHT_Node.py:502-509):
 *   sdk_frontier_boards_dev   *d_boards = device address of the current frontier's
 *                             uint8[*size][81] records (valid until the next frontier call
 *                             on this context); send a range of it with sdk_comm_send_dev.
 *   sdk_frontier_load_dev     the n records at d_boards (device, e.g. received with
 *                             sdk_comm_recv_dev) become the current frontier, in the mode
 *                             of the frontier built last (copied; 0 leaves).
 *   sdk_frontier_refine_range keep frontier boards [lo, hi) and expand them on this device
 *                             until they number `target` (or nothing branches): a rank splits
 *                             its last heavy subtree into second-level records.  The mode is
 *                             the frontier's: count mode counts the completions met while
 *                             refining in *leaves; first mode keeps them in place (lex order,
 *                             *leaves = 0), so the refined range is still sorted by completion. */
int sdk_frontier_boards_dev(sdk_ctx *ctx, void **d_boards, uint64_t *size);
int sdk_frontier_load_dev(sdk_ctx *ctx, const void *d_boards, uint64_t n);
int sdk_frontier_refine_range(sdk_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t target, uint64_t *size,
                              uint64_t *leaves);
/* Keep boards [lo, mid) refined as sdk_frontier_refine_range does, followed by boards
 * [mid, hi) unchanged (the new frontier: refined([lo, mid)) ++ [mid, hi)).  A first-solution
 * search splits the one board that hit its node budget (mid = lo + 1) and keeps the rest of
 * its live range as it is; in first mode the frontier stays sorted by completion. */
int sdk_frontier_refine_head(sdk_ctx *ctx, uint64_t lo, uint64_t mid, uint64_t hi, uint64_t target,
                             uint64_t *size, uint64_t *leaves);

/* RCCL communicator bound to a context (one rank per GPU).  Rank 0 makes the
 * id, the caller distributes it (e.g. over torch.distributed/gloo), every rank
 * calls sdk_comm_init (collective, blocks until all ranks joined). */
#define SDK_COMM_ID_BYTES 128
#define SDK_COMM_U64 0
#define SDK_COMM_I64 1
#define SDK_COMM_U8  2
#define SDK_COMM_SUM 0
#define SDK_COMM_MIN 1
#define SDK_COMM_MAX 2
int sdk_comm_unique_id(uint8_t *id /* SDK_COMM_ID_BYTES */);
int sdk_comm_init(sdk_ctx *ctx, const uint8_t *id, int rank, int world);
/* Single-process form: creates one context per device of
 * `devices` (distinct GPUs) and ONE RCCL clique over them (ncclCommInitAll);
 * ctxs[k] is rank k.  Collectives on the contexts must then be issued from one
 * host thread per context (each call enqueues on its own stream).  On failure
 * no context is left behind (ctxs[k] = NULL).  Release with sdk_destroy. */
int sdk_comm_init_all(const int *devices, int ndev, sdk_ctx **ctxs);
int sdk_comm_destroy(sdk_ctx *ctx);
/* In place, on device memory, enqueued on the context stream. */
int sdk_comm_allreduce_dev(sdk_ctx *ctx, void *d_buf, size_t count, int dtype, int op);
int sdk_comm_broadcast_dev(sdk_ctx *ctx, void *d_buf, size_t bytes, int root);
/* d_recv[r*bytes .. (r+1)*bytes) = rank r's d_send (ncclAllGather): the live-range
 * exchange of the rebalanced frontier count (shard.sharded_count_rebalanced). */
int sdk_comm_allgather_dev(sdk_ctx *ctx, const void *d_send, void *d_recv, size_t bytes);
/* Point-to-point on device memory (ncclSend / ncclRecv inside one ncclGroupStart/End):
 * the frontier-record moves of the rebalanced count.  sdk_comm_p2p_dev issues `nops`
 * operations as one group: ops[k] = SDK_COMM_SEND (bufs[k] -> rank peers[k]) or
 * SDK_COMM_RECV (rank peers[k] -> bufs[k]), bytes[k] each (a matching pair of calls on
 * the two ranks must agree on the size). */
#define SDK_COMM_SEND 0
#define SDK_COMM_RECV 1
int sdk_comm_send_dev(sdk_ctx *ctx, const void *d_buf, size_t bytes, int peer);
int sdk_comm_recv_dev(sdk_ctx *ctx, void *d_buf, size_t bytes, int peer);
int sdk_comm_p2p_dev(sdk_ctx *ctx, int nops, const int *ops, const int *peers, void *const *bufs,
                     const size_t *bytes);

/* ---- device-pointer API (asynchronous on the context stream) ------------ */
int sdk_dev_alloc(sdk_ctx *ctx, size_t bytes, void **dptr);
int sdk_dev_free(sdk_ctx *ctx, void *dptr);
int sdk_memcpy_h2d(sdk_ctx *ctx, void *dst, const void *src, size_t bytes);
int sdk_memcpy_d2h(sdk_ctx *ctx, void *dst, const void *src, size_t bytes);
int sdk_synchronize(sdk_ctx *ctx);

int sdk_check_batch_dev(sdk_ctx *ctx, const void *d_boards, void *d_verdict, size_t n);
int sdk_solve_batch_dev(sdk_ctx *ctx, const void *d_in, const void *d_first_cell_mask,
                        void *d_out, void *d_status, void *d_work, size_t n);
/* d_in and d_out 16-byte aligned, or the propagation pass is skipped */
int sdk_classify_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, size_t n,
                           uint64_t node_budget);
/* d_in and d_out 16-byte aligned (else SDK_EINVAL; d_out may be d_in).  The order rows are not
 * validated here: an entry >= 81 is "no cell" (that round leaves the board unchanged), and a
 * repeated cell is tried again (a no-op: it is empty, or it could not go). */
int sdk_minimize_batch_dev(sdk_ctx *ctx, const void *d_in, const void *d_order, void *d_out,
                           void *d_status, size_t n);
/* d_in and d_out 16-byte aligned, else SDK_EINVAL (this form never skips the pass); d_out may be
 * d_in (exactly: any other overlap is undefined).  d_level uint8[n], d_open uint8[n] or NULL. */
int sdk_grade_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, void *d_level,
                        void *d_open, size_t n, uint64_t node_budget);
/* as sdk_grade_batch_dev (alignment, d_out may be d_in: the parents then come from the copy put
 * aside); d_backdoors uint8[n] required, d_open and d_key uint8[n] or NULL. */
int sdk_rate_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, void *d_level,
                       void *d_open, void *d_backdoors, void *d_key, size_t n, uint64_t node_budget);
/* as sdk_grade_batch_dev (alignment, d_out may be d_in); d_open4 uint8[n] required, d_open uint8[n]
 * or NULL. */
int sdk_subsets_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, void *d_level,
                          void *d_open, void *d_open4, size_t n, uint64_t node_budget);
/* as sdk_grade_batch_dev (alignment, d_out may be d_in); d_open5 uint8[n] required, d_open and d_open4
 * uint8[n] or NULL. */
int sdk_fish_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, void *d_level,
                       void *d_open, void *d_open4, void *d_open5, size_t n, uint64_t node_budget);
/* as sdk_grade_batch_dev (alignment, d_out may be d_in); d_open6 uint8[n] required, d_open, d_open4 and
 * d_open5 uint8[n] or NULL. */
int sdk_wings_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, void *d_level,
                        void *d_open, void *d_open4, void *d_open5, void *d_open6, size_t n,
                        uint64_t node_budget);
/* as sdk_grade_batch_dev (alignment, d_out may be d_in); d_open7 uint8[n] required, d_open, d_open4,
 * d_open5 and d_open6 uint8[n] or NULL. */
int sdk_chains_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_out, void *d_status, void *d_level,
                         void *d_open, void *d_open4, void *d_open5, void *d_open6, void *d_open7, size_t n,
                         uint64_t node_budget);
/* d_in and d_canon 16-byte aligned, else SDK_EINVAL; d_canon may be d_in (exactly).  d_solution, d_gather,
 * d_relabel and d_ties (uint16[n]) or NULL; a d_solution that is not 16-byte aligned only skips the
 * propagation pass, as in sdk_classify_batch_dev. */
int sdk_canonical_batch_dev(sdk_ctx *ctx, const void *d_in, void *d_canon, void *d_solution, void *d_status,
                            void *d_gather, void *d_relabel, void *d_ties, size_t n, uint64_t node_budget);
/* d_grids (and d_order, d_puzzles) 16-byte aligned, else SDK_EINVAL; d_order and d_placements
 * (uint32[n]) nullable.  Spans as the host-pointer forms: one per call. */
int sdk_generate_grids_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n, void *d_grids,
                           void *d_order, void *d_placements);
int sdk_generate_puzzles_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n, void *d_puzzles,
                             void *d_grids, void *d_status);
/* d_in and d_out 16-byte aligned (else SDK_EINVAL; d_out may be d_in).  The order rows are not
 * validated here: an entry >= 81 is "no cell" (that round leaves the board unchanged), and a
 * repeated cell is tried again (a no-op: it is empty, or it could not go). */
int sdk_minimize_level_batch_dev(sdk_ctx *ctx, const void *d_in, const void *d_order, int level,
                                 void *d_out, void *d_status, size_t n);
/* d_puzzles and d_grids 16-byte aligned, else SDK_EINVAL */
int sdk_generate_level_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n, int level,
                           void *d_puzzles, void *d_grids, void *d_status);
/* d_puzzles and d_grids 16-byte aligned (and d_index 8-byte), else SDK_EINVAL; d_level, d_open,
 * d_index and scanned nullable; found and scanned are host pointers.  The call returns when the scan
 * is decided (it waits for every round's count): *found and *scanned are final then, and the device
 * rows are valid after sdk_synchronize.  Rows from *found on are not written. */
int sdk_generate_graded_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                            uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                            uint64_t max_scan, uint64_t chunk,
                            void *d_puzzles, void *d_grids, void *d_level, void *d_open,
                            void *d_index, uint64_t *found, uint64_t *scanned);
/* as sdk_generate_graded_dev; d_backdoors and d_key uint8[n] or NULL */
int sdk_generate_rated_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                           uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                           uint32_t backdoors_lo, uint32_t backdoors_hi,
                           uint64_t max_scan, uint64_t chunk,
                           void *d_puzzles, void *d_grids, void *d_level, void *d_open,
                           void *d_backdoors, void *d_key,
                           void *d_index, uint64_t *found, uint64_t *scanned);
/* as sdk_generate_graded_dev; d_open4 uint8[n] or NULL */
int sdk_generate_subsets_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                             uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                             uint32_t open4_lo, uint32_t open4_hi,
                             uint64_t max_scan, uint64_t chunk,
                             void *d_puzzles, void *d_grids, void *d_level, void *d_open,
                             void *d_open4,
                             void *d_index, uint64_t *found, uint64_t *scanned);
/* as sdk_generate_graded_dev; d_open4 and d_open5 uint8[n] or NULL */
int sdk_generate_fish_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                          uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                          uint32_t open4_lo, uint32_t open4_hi, uint32_t open5_lo, uint32_t open5_hi,
                          uint64_t max_scan, uint64_t chunk,
                          void *d_puzzles, void *d_grids, void *d_level, void *d_open,
                          void *d_open4, void *d_open5,
                          void *d_index, uint64_t *found, uint64_t *scanned);
/* as sdk_generate_graded_dev; d_open5 and d_open6 uint8[n] or NULL */
int sdk_generate_wings_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                           uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                           uint32_t open5_lo, uint32_t open5_hi, uint32_t open6_lo, uint32_t open6_hi,
                           uint64_t max_scan, uint64_t chunk,
                           void *d_puzzles, void *d_grids, void *d_level, void *d_open,
                           void *d_open5, void *d_open6,
                           void *d_index, uint64_t *found, uint64_t *scanned);
/* as sdk_generate_graded_dev; d_open6 and d_open7 uint8[n] or NULL */
int sdk_generate_chains_dev(sdk_ctx *ctx, uint64_t seed, uint64_t first, size_t n,
                            uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                            uint32_t open6_lo, uint32_t open6_hi, uint32_t open7_lo, uint32_t open7_hi,
                            uint64_t max_scan, uint64_t chunk,
                            void *d_puzzles, void *d_grids, void *d_level, void *d_open,
                            void *d_open6, void *d_open7,
                            void *d_index, uint64_t *found, uint64_t *scanned);

/* One round of the selection behind sdk_generate_graded / _rated / _subsets (select_kernel.h), on rows
 * the caller supplies instead of rows the generator and the grader made: the seam through which the
 * selection kernels are tested.  Row i (0 <= i < m) is a hit when status[i] == SDK_SOLVED, level[i] < 32
 * and bit level[i] of level_mask is set, clues_lo <= (non-zero bytes of puzzles[i]) <= clues_hi, and,
 * if level[i] == SDK_GRADE_SEARCH, backdoors_lo <= backdoors[i] <= backdoors_hi where `backdoors` is
 * given and open4_lo <= open4[i] <= open4_hi where `open4` is given.  The hits keep their order and
 * take the ranks base, base + 1, ...; a hit of rank r < n is written to row r of every output that is
 * given: its puzzle and grid row, level, open, first + i, and backdoors / key / open4 (SDK_RATE_NONE /
 * SDK_SUBSETS_NONE, 0xFF, where that source is NULL).  Nothing else of an output is written.
 *   puzzles, grids  uint8[tiles * 64][81] with tiles = ceil(m / 64): WHOLE tiles of 64 rows, 16-byte
 *                   aligned.  The rows from m to the end of the last tile are read and ignored; the
 *                   call cannot check that they are there.
 *   status  int8[m];  level, open  uint8[m];  backdoors, key, open4  uint8[m] or NULL;
 *   m       1..2^24;  first + m must not overflow;
 *   n       the quota, 1..2^31-1;  base < n: the hits of the earlier rounds;
 *   level_mask and the three ranges: as sdk_generate_graded, _rated and _subsets;
 *   out_puzzles, out_grids  uint8[n][81], 16-byte aligned, required;  out_level, out_open,
 *                   out_backdoors, out_key, out_open4  uint8[n] or NULL;  out_index  uint64[n] or NULL.
 * All of these are device pointers.  *total = base + every hit of the rows, whatever the quota;
 * *last = 1 + the row of the hit of rank n - 1, or 0 when that hit is not among these rows (host
 * pointers, both required).  Rounds chain: a stream cut into calls with base = the call before's
 * *total writes what one call over the whole stream writes.  The call sets the context's selection
 * word to {base, 0}, enqueues the three launches, reads the word back (8 bytes) and returns; it is one
 * span under SDK_OPT_TIMING.  A bad argument is SDK_EINVAL: nothing is launched or written. */
typedef struct sdk_select_rows {
    const void *puzzles, *grids, *status, *level, *open;
    const void *backdoors, *key, *open4;
    uint64_t m, first, base, n;
    uint32_t level_mask, clues_lo, clues_hi;
    uint32_t backdoors_lo, backdoors_hi, open4_lo, open4_hi;
    void *out_puzzles, *out_grids, *out_level, *out_open, *out_index;
    void *out_backdoors, *out_key, *out_open4;
} sdk_select_rows;
int sdk_select_rows_dev(sdk_ctx *ctx, const sdk_select_rows *rows, uint64_t *total, uint64_t *last);

/* Kernel time accounting (HIP events on the context stream, bracketing every
 * kernel launched by the *_dev / host calls since the last reset).  Only with
 * SDK_OPT_TIMING = 1; at most 65536 timed launches between resets (further
 * launches fail with SDK_EINVAL).  Valid after sdk_synchronize. */
int sdk_timer_reset(sdk_ctx *ctx);
int sdk_timer_read(sdk_ctx *ctx, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* SUDOKU_HIP_H */
