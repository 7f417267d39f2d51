// solve_args.h -- what the host and the solve kernels (solve_kernel.h, solve2_kernel.h, solve4_kernel.h,
// solve_lane_kernel.h) share: the launch arguments, the order and status constants, the dequeue-head
// layout and the per-workgroup stack sizes.  Plain C++: host files include it without the kernels.
#pragma once
#include <cstdint>

namespace sdk {

constexpr int kMaxDepth = 81;
constexpr uint32_t kChunk = 4;        // expand_kernel chunk; solve_kernel takes SolveArgs::chunk
// words of a workgroup's global stack: one board per wave, two (solve2_kernel), four (solve4_kernel)
constexpr int kStackWordsPerBlock = kMaxDepth * 64;
constexpr int kStack2WordsPerBlock = kMaxDepth * 64 * 2;
constexpr int kStack4WordsPerBlock = kMaxDepth * 2 * 64 * 2;
constexpr int kLaneThreads = 256;          // solve_lane_kernel: 4 independent waves per workgroup

// ORDER_CLASSIFY (sdk_classify_batch, QUAD solver only; not an SDK_ORDER_*): MRV search for at most
// two completions like ORDER_MRV, but the second one ends the board as kStMultiple with its input
// restored instead of starting the LEX re-search
enum { ORDER_MRV = 0, ORDER_LEX = 1, ORDER_CLASSIFY = 2 };

struct SolveArgs {
    const uint8_t* in;
    const uint16_t* mask;      // nullable: first-cell digit mask, bit d = digit d
    uint8_t* out;
    int8_t* status;
    uint64_t* work;            // nullable
    uint64_t n;
    uint32_t* next;            // work counter (zeroed before launch)
    uint32_t* stack;           // gridDim.x * kStackWordsPerBlock words
    uint64_t budget;           // nodes per board, 0 = unlimited
    int order;                 // SDK_ORDER_*, or ORDER_CLASSIFY
    uint64_t limit;            // count mode: per-board completion limit (0 = none)
    unsigned long long* count; // count mode: running total over the batch (atomic)
    unsigned long long* counts;// count mode: per-board counts (nullable)
    int count_mode;
    uint32_t chunk;            // boards per dequeue (one atomic on `next` per chunk)
    int work_rounds;           // what work[] counts: 0 search nodes, 1 propagation rounds, 2 max DFS depth
    uint64_t in_first;         // board i of the launch reads in[(in_first + i*in_step)*81];
    uint64_t in_step;          // outputs stay dense (out[i*81], status[i]); 0/1 = contiguous
    int locked;                // QUAD solver: locked-candidates pass at fixpoints (SDK_OPT_LOCKED)
    uint32_t* heads;           // QUAD solver: kHeads dequeue heads, one per XCD segment (nullable)
    void* donate;              // QUAD solver, LEX solves: subtree-donation area (donate_args.h, DnCtl first)
    const uint32_t* n_dev;     // donation kernel: board count read on the device (a phase's list
                               // length, written by an earlier launch); `n` is then its bound
    void* save = nullptr;      // QUAD split phase: stacks of boards that reach the split budget
                               // (donate_args.h SplitSave; nullable)
    uint32_t* save_idx = nullptr;   // ... and each saved board's entry (by board index)
    uint64_t budget_big = 0;        // QUAD split phase of a device-counted batch (n_dev): the budget
                                    // when more than kBudgetBigBoards boards are searched (0 = budget)
    long long* found = nullptr;     // QUAD first-solution scan (sdk_frontier_first): the lowest board
                                    // index (in_first + i * in_step) with status 1 or -2 so far; boards
                                    // above it are cancelled (solve4_kernel.h, s_found4)
};
// the phased solve's default split budget doubles above this many searched boards (sudoku_hip.hip, launch_solve)
constexpr uint64_t kBudgetBigBoards = 1ull << 19;
// status of a board a first-solution scan stopped because it lies above a lower board's hit
constexpr int kStCancelled = -3;
// status of a classified board with at least two completions (SDK_MULTIPLE)
constexpr int kStMultiple = 2;

// per-XCD dequeue: the first n - n/128 boards are cut into kHeads contiguous segments with a
// head each, workgroup g takes chunks of segment g % kHeads (the XCD the round-robin
// dispatch put it on) and, once that is drained, of the shared tail (one more head);
// heads kHeadStride words apart (own cache lines)
#ifndef SDK_HEADS
#define SDK_HEADS 8
#endif
constexpr int kHeads = SDK_HEADS;   // a multiple of 8: segment g % kHeads stays on one XCD
constexpr int kHeadStride = 64;
// the heads buffer: kHeads segment heads, the shared tail, then the launch's dequeue counter, so
// one memset clears a QUAD launch's dequeue state
constexpr int kHeadNext = (kHeads + 1) * kHeadStride;
constexpr int kHeadWords = (kHeads + 2) * kHeadStride;

}  // namespace sdk
