// sudoku_hip.hip -- libsudoku_hip.so: C-ABI (include/sudoku_hip.h) over the gfx950 kernels.
//
// Plain C++ (the Makefile compiles it with no device pass): the kernels are behind launch.h.
// Host side is deliberately thin: a context = (device, stream, grow-only device
// workspaces, HIP event pairs for kernel timing, options) behind a mutex.  No
// CPU compute path exists: every board is checked / solved by a HIP kernel.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/sudoku_hip.h"
#include "launch.h"   // every kernel: its unit's launch functions and *_args.h (this file is plain C++)

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIPCALL(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? SDK_ENOMEM : SDK_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

constexpr size_t kMaxTimedLaunches = 1u << 16;

// A device allocation owned by its holder: freed when the holder goes (sdk_destroy deletes the
// context after selecting its device), so no buffer added to sdk_ctx can leak.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {      // (std::swap of two buffers moves through this)
        if (this != &o) {
            if (p) (void)hipFree(p);
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
};

// argument checks the host-pointer and _dev forms of a call share
int check_budget_arg(uint64_t node_budget) {
    if (node_budget != SDK_BUDGET_CONTEXT && node_budget > (uint64_t)INT64_MAX)
        return fail(SDK_EINVAL, "node budget out of range");
    return SDK_OK;
}
int check_board_count(size_t n) {
    if (n > 0x7FFFFFFFull) return fail(SDK_EINVAL, "at most 2^31-1 boards per call");
    return SDK_OK;
}
// every row of a host-pointer call's removal orders is a permutation of 0..80
int check_order_rows(const uint8_t* order, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        bool seen[81] = {};
        for (int q = 0; q < 81; ++q) {
            const uint8_t v = order[i * 81 + q];
            if (v >= 81 || seen[v])
                return fail(SDK_EINVAL, "order row %zu is not a permutation of 0..80 (entry %d = %u)", i, q, (unsigned)v);
            seen[v] = true;
        }
    }
    return SDK_OK;
}
// an ABI node budget as a SolveCall's: SDK_BUDGET_CONTEXT is "the context's"
int64_t budget_arg(uint64_t node_budget) { return node_budget == SDK_BUDGET_CONTEXT ? -1 : (int64_t)node_budget; }

}  // namespace

// Pinned host staging of the host-pointer calls (Staging below): the
// caller's arrays are copied into it on the CPU and moved by true asynchronous DMA.  HIP's own path
// for pageable memory took 12-25 ms per call now and then for a 1.3 MB transfer whose kernel ran
// 0.2 ms (profiles/r05/slice_probe_timing_r05c.log: a node's search slices), all of it CPU time in
// the calling thread.  Grown as needed up to kStageMax; larger calls keep the pageable path.
struct HostBuf {
    void* p = nullptr;
    size_t bytes = 0;
};
constexpr size_t kStageMax = size_t(256) << 20;
constexpr size_t kStageInit = size_t(8) << 20;   // allocated with the context: pinning costs ~ms
                                                 // (the first slice of a node paid 34 ms growing it)

// The boards one phase of a phased solve passes to the next, as a dense batch: their list (length
// word first, then their indices), their inputs and first-cell masks, and the donation launch's answers.
struct DnTail {
    DevBuf list, in, mask, out, st, work;
};

struct sdk_ctx {
    int device = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    std::mutex mu;
    HostBuf stage;                 // pinned staging (see HostBuf)
    // options
    int64_t order = SDK_ORDER_LEX;     // lex-first DFS: no uniqueness proof needed (faster than MRV_UNIQUE, r02)
    int64_t budget = 0;
    int64_t waves_per_cu = 32;
    int64_t check_blocks_per_cu = 3;
    int64_t check_variant = SDK_CHECK_REG1;
    int64_t solve_chunk = 0;          // boards per dequeue, 0 = automatic
    int64_t work_rounds = 0;
    int64_t solver = SDK_SOLVER_QUAD;
    int64_t locked = 1;                // QUAD: locked candidates at fixpoints (fewer search nodes, same answers)
    int64_t waves_per_cu2 = 28;       // solve2/solve4 grid per CU = solve4's resident waves (7 per SIMD; a larger
                                  // grid only adds waves that start once the queue is drained: 1 % slower, r02)
    // workspaces
    DevBuf stack, counter, heads, in, mask, out, status, work, verdict;
    uint32_t heads_round = 0;      // launches since the heads pool was cleared (kHeadRounds regions)
    int64_t xcd_heads = 1;             // QUAD: per-XCD dequeue heads (SDK_OPT_XCD_HEADS)
    int64_t donate = 1;                // QUAD, LEX solves: subtree donation (SDK_OPT_DONATE)
    DevBuf dn;                     // two donation areas (solve4_kernel.h: DnCtl, records, items,
                                   // mailboxes), one per donation phase of a phased solve
    DnTail dn_tail[2];             // [0] the phased solve's tail boards (area 0), [1] its LEX re-solves (area 1)
    DevBuf dn_stat;                // [0] boards the last phased solve passed to the donation
                                   // kernel, [1] of those, boards re-solved in LEX order
    // The last solve's outcome, read by later ABI calls (sdk_get_option, sdk_debug_p32_list,
    // dn_check_error) -- everything else about a call travels in its SolveCall.  A classify is a
    // one-launch solve: dn_ran is false after it, and prop32_ran is that of its last slice.  A
    // prop32 fallback solve (n_dev set) leaves prop32_ran alone.
    bool dn_ran = false;           // the last solve was phased (dn_stat and `delivered` are its)
    bool prop32_ran = false;       // the last solve ran the prop32 pass (p32_list[0] = its undecided boards)
    bool dn_err_check = false;     // a phased solve ran since its control blocks' error words were read
    int64_t dn_fault = 0;              // SDK_OPT_DN_FAULT (test only)
    int64_t dn_helpers = 2;            // SDK_OPT_DONATE_HELPERS: donation-launch waves per listed board (+ 64)
    int64_t dn_resume = 1;             // SDK_OPT_DONATE_RESUME: split boards resume from their saved stacks
    DevBuf dn_save, dn_save_idx, dn_seeds;   // sdk::SplitSave, its entry per board, the seed list
    int64_t dn_exhaustive = 1;         // phase 2 in MRV count-to-2 order (SDK_OPT_DONATE_MODE)
    int64_t dn_max = 1 << 19;      // largest batch solved in phases (SDK_OPT_DONATE_MAX, 0 = any)
    uint32_t dn_epoch = 0;         // launches that used it (mailbox / registration entries carry it)
    int dn_blocks_per_cu = 0;      // resident solve4_kernel<true> workgroups per CU (queried once)
    int64_t prop32 = 1;                // QUAD: bit-sliced root propagation first (SDK_OPT_PROP32)
    int64_t prop32_lc = 5 | (3 << 8);  // ... a locked-candidates pass every this many steps (low byte),
                                   //     the first after step (value >> 8), 0 = the period: after
                                   //     steps 3, 8, 13, ... (prop32 "schedule")
    int64_t prop32_min = 4096;     // ... for batches of at least this many boards
    int64_t prop32_handover = 1;       // ... undecided boards searched from their propagated grids
    int64_t prop32_tail_live = 0;      // ... a group's last (at most this many) live boards handed over
    int64_t prop32_tail_step = 24;     //     from this step on (SDK_OPT_PROP32_TAIL = live | step << 8)
    DevBuf p32_ctl, p32_list, p32_in, p32_out, p32_st;
    int clock_probe = 0;           // sdk_debug_clock_arm: prop32 passes run the stamped twin
    DevBuf p32_stamps;             // ... its stamps, 4 words per workgroup of the last such pass
    uint32_t p32_stamp_wgs = 0;
    DevBuf mz_cand, mz_out, mz_st; // sdk_minimize_batch: a round's candidates, their classify outputs and verdicts
    DevBuf mz_order;               // ... the host-pointer call's order rows
    DevBuf gr_in;                  // sdk_grade_batch_dev with d_out == d_in: a slice's inputs
    DevBuf gr_level, gr_open;      // sdk_grade_batch: the host-pointer call's grades (gr_open also
                                   // where the caller wants no open counts)
    DevBuf rt_bd, rt_key;          // sdk_rate_batch: the host-pointer call's ratings
    int64_t gen_cap = 1 << 20;     // SDK_OPT_GEN_CAP: a generated grid is kept iff its fill placed at most this many digits
    DevBuf gen_order;              // sdk_generate_puzzles: a slice's removal orders
    DevBuf gen_plc;                // sdk_generate_grids (host pointers): the placement counts
    // sdk_generate_graded: a round's candidates (puzzles, grids, generator status), their grading
    // (completions and verdicts nobody reads, level, open count) and selection (per tile of 64 rows:
    // ballot, popcount, offset); the call's device word (sdk::SelWord); the host-pointer call's outputs
    DevBuf gg_puz, gg_grid, gg_st, gg_sol, gg_gst, gg_level, gg_open, gg_ballot, gg_count, gg_offset, gg_word;
    DevBuf gg_out_puz, gg_out_grid, gg_out_level, gg_out_open, gg_out_index;
    DevBuf gg_bd, gg_key, gg_out_bd, gg_out_key;   // sdk_generate_rated: a round's ratings, the host call's
    DevBuf s4_open4, gg_o4, gg_out_o4;   // sdk_subsets_batch (host pointers); sdk_generate_subsets: a round's, the host call's
    DevBuf f5_open5, gg_o5, gg_out_o5;   // sdk_fish_batch, sdk_generate_fish: the same for open5 (open4 goes through the above)
    DevBuf f5_open4;                     // the fish stage's open4 of a slice where the caller wants none
    DevBuf w6_open6, gg_o6, gg_out_o6;   // sdk_wings_batch, sdk_generate_wings: the same for open6
    DevBuf w6_open5;                     // the wings stage's open5 of a slice where the caller wants none (open4: f5_open4)
    DevBuf c7_open7, gg_o7, gg_out_o7;   // sdk_chains_batch, sdk_generate_chains: the same for open7
    DevBuf c7_open6;                     // the chains stage's open6 of a slice where the caller wants none
    DevBuf cn_sol;                 // sdk_canonical_batch_dev without a solution buffer: a slice's completions
    DevBuf cn_gather, cn_relabel, cn_ties;   // sdk_canonical_batch: the host-pointer call's symmetries and tie counts
    DevBuf fr_a, fr_b, prop, bcell, bmask, nchild, offs, fr_status, fr_mask, tsum, fr_ctl;
    DevBuf fr_tail;                // refine_head: the boards kept after the refined ones
    // the device-resident frontier of the last sdk_frontier_build (in fr_a)
    uint64_t fr_size = 0;
    uint64_t fr_leaves = 0;
    uint32_t fr_levels = 0;
    bool fr_valid = false;
    int fr_mode = SDK_FRONTIER_COUNT;   // kept by refinements and loaded records
    // RCCL communicator (sdk_comm_init), one rank per context
    ncclComm_t comm = nullptr;
    int comm_rank = 0;
    int comm_world = 1;
    // timing
    int64_t timing = 0;           // SDK_OPT_TIMING
    bool timer_hold = false;      // a TimedSpan is open: the launches inside it are not timed apart
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
};

namespace {

constexpr uint64_t kDnSplitDefault = 128;   // SDK_OPT_DONATE = 1: split budget (search nodes) of the plain phase
                                            // (256 to round 3; profiles/r03/sweep_split_r03.log)
constexpr uint32_t kHeadRounds = 64;        // dequeue-head regions per clear (launch_solve_once)

// a pinned staging area of at least `bytes` (nullptr: too large, use the pageable path)
void* stage_host(HostBuf& b, size_t bytes) {
    if (bytes > kStageMax) return nullptr;
    if (b.bytes >= bytes) return b.p;
    if (b.p) (void)hipHostFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    // doubling growth: a node's slices grow their batches a little at a time
    const size_t want = std::min(kStageMax, std::max(bytes, std::max(b.bytes * 2, kStageInit)));
    if (hipHostMalloc(&b.p, want, hipHostMallocDefault) != hipSuccess) {
        b.p = nullptr;
        return nullptr;
    }
    b.bytes = want;
    return b.p;
}

int ensure(DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return SDK_OK;
    if (b.p) HIPCALL(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    size_t want = std::max(bytes, (size_t)256);
    HIPCALL(hipMalloc(&b.p, want));
    b.bytes = want;
    return SDK_OK;
}

// Kernel timing is opt-in (SDK_OPT_TIMING): with it off no event is created or
// recorded, so a long-running node or drop-in solver holds no per-launch state.
int timer_begin(sdk_ctx* c, hipEvent_t* stop_out) {
    *stop_out = nullptr;
    if (!c->timing || c->timer_hold) return SDK_OK;
    if (c->events_used >= kMaxTimedLaunches) return fail(SDK_EINVAL, "%zu timed launches since sdk_timer_reset", kMaxTimedLaunches);
    if (c->events_used == c->events.size()) {
        hipEvent_t a, b;
        HIPCALL(hipEventCreate(&a));
        HIPCALL(hipEventCreate(&b));
        c->events.emplace_back(a, b);
    }
    auto& pr = c->events[c->events_used++];
    HIPCALL(hipEventRecord(pr.first, c->stream));
    *stop_out = pr.second;
    return SDK_OK;
}

int timer_end(sdk_ctx* c, hipEvent_t stop) {
    if (stop) HIPCALL(hipEventRecord(stop, c->stream));
    return SDK_OK;
}

// Several launches timed as ONE span (a phased solve, the prop32 fallback, a minimise call): begin()
// records the start and holds the timer, so the launches and spans inside record nothing; end(rc)
// records the stop when the work returned SDK_OK.  The hold goes back to what it was on every path
// out of the scope (under an outer span the whole object does nothing).
struct TimedSpan {
    sdk_ctx* c;
    const bool outer;
    hipEvent_t stop = nullptr;
    explicit TimedSpan(sdk_ctx* ctx) : c(ctx), outer(ctx->timer_hold) {}
    ~TimedSpan() { c->timer_hold = outer; }
    int begin() {
        const int rc = timer_begin(c, &stop);
        if (!rc) c->timer_hold = true;
        return rc;
    }
    int end(int rc) {
        c->timer_hold = outer;
        return rc ? rc : timer_end(c, stop);
    }
};

// a grid for `items` at `per_block` each: at least one block, at most `blocks_per_cu` per CU
unsigned grid_for(const sdk_ctx* c, uint64_t items, uint64_t per_block, uint64_t blocks_per_cu) {
    return (unsigned)std::max<uint64_t>(
        1, std::min<uint64_t>((items + per_block - 1) / per_block, (uint64_t)c->cus * blocks_per_cu));
}

// One slot of a host-pointer call's staging: `bytes` that go from the caller's `h_src` to the device
// (`d_dst`) before the launch, come back from `d_src` to the caller's `h_dst` after it, or both through
// the same slot.  A null host pointer leaves that copy out; the slot keeps its place.
struct Piece {
    size_t bytes;
    const void* h_src;
    void* d_dst;
    const void* d_src = nullptr;
    void* h_dst = nullptr;
    char* slot = nullptr;   // (Staging's: its place in the pinned area)
};

// The copies of a host-pointer call: send() before the launch, fetch() after it (it synchronizes).
// The (at most eleven: sdk_generate_chains) pieces lie in the pinned area (HostBuf) in the order given -- widest element
// type first, so every slot is aligned for its type; a call too large for the area copies straight
// from / to the caller's pageable memory.  An error return between send() and the end of fetch()
// may leave copies from / into the area queued, so the stream is drained first: the next call's
// memcpy into the area (or a grow that frees it) cannot race them.
class Staging {
    sdk_ctx* c;
    Piece p[11];
    int np = 0;
    bool armed = true;

  public:
    Staging(sdk_ctx* ctx, std::initializer_list<Piece> pieces) : c(ctx) {
        size_t total = 0;
        for (const Piece& q : pieces) {
            p[np++] = q;
            total += q.bytes;
        }
        char* st = static_cast<char*>(stage_host(c->stage, total));
        for (int i = 0; i < np && st; ++i) {
            p[i].slot = st;
            st += p[i].bytes;
        }
    }
    ~Staging() {
        if (armed) (void)hipStreamSynchronize(c->stream);
    }
    int send() {
        for (int i = 0; i < np; ++i)
            if (p[i].h_src && p[i].slot) std::memcpy(p[i].slot, p[i].h_src, p[i].bytes);
        for (int i = 0; i < np; ++i)
            if (p[i].h_src)
                HIPCALL(hipMemcpyAsync(p[i].d_dst, p[i].slot ? p[i].slot : p[i].h_src, p[i].bytes,
                                       hipMemcpyHostToDevice, c->stream));
        return SDK_OK;
    }
    int fetch() {
        for (int i = 0; i < np; ++i)
            if (p[i].h_dst)
                HIPCALL(hipMemcpyAsync(p[i].slot ? p[i].slot : p[i].h_dst, p[i].d_src, p[i].bytes,
                                       hipMemcpyDeviceToHost, c->stream));
        HIPCALL(hipStreamSynchronize(c->stream));
        armed = false;
        for (int i = 0; i < np; ++i)
            if (p[i].h_dst && p[i].slot) std::memcpy(p[i].h_dst, p[i].slot, p[i].bytes);
        return SDK_OK;
    }
};

// One solve's arguments (launch_solve).  A call site gives the buffers and the board count, in this
// order (each of its own type), and names whatever else it sets.
struct SolveCall {
    const uint8_t* in = nullptr;        // boards in_first, in_first + in_step, ... of `in`
    const uint16_t* mask = nullptr;     // first-cell masks (nullable)
    uint8_t* out = nullptr;
    int8_t* status = nullptr;
    uint64_t* work = nullptr;           // work counters (nullable)
    size_t n = 0;
    const uint32_t* n_dev = nullptr;    // the batch's length on the device (n bounds it; the prop32 fallback)
    uint64_t in_first = 0, in_step = 1;
    int count_mode = 0;                 // count completions (up to `limit`) into *count / counts[i]
    uint64_t limit = 0;
    unsigned long long* count = nullptr;
    unsigned long long* counts = nullptr;
    int order = -1;                     // SDK_ORDER_* or sdk::ORDER_CLASSIFY; -1 = the context's
    int64_t budget = -1;                // search nodes per board, 0 = unlimited; -1 = the context's
    int64_t donate = -1;                // SDK_OPT_DONATE for this call; -1 = the context's
    int solver = -1;                    // SDK_SOLVER_*; -1 = the context's
    long long* found = nullptr;         // a first-solution scan's found word (frontier_first; SolveArgs::found)
};

// What one launch of a phased solve adds to its SolveCall (launch_solve_once).
struct SolvePhase {
    enum Kind { kPlain, kSplit, kDonation };
    Kind kind = kPlain;
    void* area = nullptr;               // kDonation: the donation area
    uint64_t budget_big = 0;            // kSplit: the budget above sdk::kBudgetBigBoards searched boards
    bool save = false;                  // kSplit: the stacks of stopped boards are saved for resume
};

int launch_check(sdk_ctx* c, const uint8_t* d_in, uint8_t* d_out, size_t n) {
    if (n == 0) return SDK_OK;
    if (reinterpret_cast<uintptr_t>(d_in) & 15) return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    const uint64_t tiles = (n + sdk::kCheckThreads - 1) / sdk::kCheckThreads;
    const unsigned grid = grid_for(c, n, sdk::kCheckThreads, c->check_blocks_per_cu);
    hipEvent_t stop;
    int rc = timer_begin(c, &stop);
    if (rc) return rc;
    int variant = c->check_variant;
    if (variant == SDK_CHECK_REG2 && tiles < 2ull * grid) variant = SDK_CHECK_REG1;   // rr2 needs a full tile per slot
    HIPCALL(sdk::launch_check(variant, d_in, d_out, (uint64_t)n, grid, c->stream));
    if ((rc = timer_end(c, stop))) return rc;
    return SDK_OK;
}

// One solve kernel launch.  `s` is a call launch_solve has resolved (order, budget and solver are
// values, not -1); `ph` says which launch of a phased solve (QUAD, LEX or MRV_UNIQUE solves with
// SDK_OPT_DONATE) it is: the plain launch; the split phase (plain kernel, s.budget = the split budget);
// or the donation kernel solve4_kernel<true> on the full resident grid, in donation area ph.area
// (see launch_solve).  The phases' control words are zeroed by launch_solve's prep launch.
int launch_solve_once(sdk_ctx* c, const SolveCall& s, const SolvePhase& ph = {}) {
    const size_t n = s.n;
    const int count_mode = s.count_mode;
    const bool plain = ph.kind == SolvePhase::kPlain, donation = ph.kind == SolvePhase::kDonation;
    if (n == 0) return SDK_OK;
    int rc;
    if ((rc = check_board_count(n))) return rc;
    sdk::SolveArgs a{};   // what every solve kernel takes from the call; the rest is set below
    a.in = s.in;
    a.mask = s.mask;
    a.out = s.out;
    a.status = s.status;
    a.work = s.work;
    a.n = n;
    a.budget = (uint64_t)s.budget;
    a.in_first = s.in_first;
    a.in_step = s.in_step;
    hipEvent_t stop;
    if (s.solver == SDK_SOLVER_LANE && !count_mode) {
        // one board per lane: the reference's own DFS (solve_lane_kernel.h); `work` =
        // the reference's validations, the budget counts validations
        if (!s.out || !s.status) return fail(SDK_EINVAL, "solve needs out and status buffers");
        if (s.order == SDK_ORDER_MRV_UNIQUE)
            return fail(SDK_EINVAL, "the LANE solver runs the reference's order only (SDK_ORDER_LEX)");
        if ((rc = ensure(c->counter, 256))) return rc;
        HIPCALL(hipMemsetAsync(c->counter.p, 0, 8, c->stream));
        a.next = static_cast<uint32_t*>(c->counter.p);
        if ((rc = timer_begin(c, &stop))) return rc;
        HIPCALL(sdk::launch_solve_lane(a, grid_for(c, n, sdk::kLaneThreads, 6), c->stream));
        return timer_end(c, stop);
    }
    // two (solve2_kernel) or four (solve4_kernel) boards per wave for solves; count mode stays
    // one board per wave
    // count mode: QUAD counts four boards per wave (solve4's count mode) unless per-board counts
    // are asked for; the other solvers count with the one-board-per-wave kernel
    const int per_wave = count_mode ? ((s.solver == SDK_SOLVER_QUAD && !s.counts) ? 4 : 1)
                                    : (s.solver == SDK_SOLVER_QUAD ? 4 : (s.solver == SDK_SOLVER_HALFWAVE ? 2 : 1));
    const bool two = per_wave == 2, four = per_wave == 4;
    if ((two || four) && !s.status) return fail(SDK_EINVAL, "solve needs a status buffer");
    if ((two || four) && !count_mode && !s.out) return fail(SDK_EINVAL, "solve needs an out buffer");
    const uint64_t slots = (uint64_t)c->cus * (per_wave > 1 ? c->waves_per_cu2 : c->waves_per_cu) * per_wave;
    // 16 boards per dequeue (fewer when a slot would get < 2 dequeues); 8 for the QUAD solver,
    // whose dequeues go to per-XCD heads with one stage per wave and dealt first chunks: there
    // 8 is the fastest at every C4 shard size and on 30-clue boards (round 3,
    // profiles/r03/sweep_chunk_r03.log: 1.25M 17-clue 1.489 vs 1.557 ms at 16, 10M 10.01 vs
    // 10.05, 30-clue 1M 0.648 vs 0.676).  Count mode uses single boards (subtrees differ by
    // orders of magnitude).
    // Round 4, QUAD by batch size (profiles/r04/ab_chunk_by_size_r04u.log, M 17-clue puzzles/s at
    // chunk 4 / 6 / 8): 1.25M boards 882 / 867 / 862, 2.5M 939 / 958 / 924, 5M 992 / 1000 / 994, 10M
    // 1026 / 1036 / 1036 -- below 64 boards per slot the launch drain (the last chunks) outweighs
    // the extra dequeues, so 4; else 6
    const uint64_t quad_chunk = n < slots * 64 ? 4 : 6;
    const uint32_t chunk = count_mode ? 1u
        : c->solve_chunk ? (uint32_t)c->solve_chunk
        : (uint32_t)std::min<uint64_t>(per_wave == 4 ? quad_chunk : 16, std::max<uint64_t>(1, n / (slots * 2)));
    const uint64_t want = (n + chunk - 1) / chunk;
    const unsigned grid = grid_for(c, want, per_wave, per_wave > 1 ? c->waves_per_cu2 : c->waves_per_cu);
    const size_t stack_words = four ? sdk::kStack4WordsPerBlock : (two ? sdk::kStack2WordsPerBlock : sdk::kStackWordsPerBlock);
    if ((rc = ensure(c->stack, (size_t)grid * stack_words * sizeof(uint32_t))) || (rc = ensure(c->counter, 256)))
        return rc;
    // QUAD with per-XCD heads: the dequeue counter lives in the heads region after the heads.
    // Plain launches take a fresh region of a pool of kHeadRounds, cleared by one memset every
    // kHeadRounds launches (a per-launch memset is its own ~4 us dispatch in front of the
    // kernel); the split phase's region is cleared by its prep launch.  Otherwise the counter
    // is word 0 of c->counter (words 1.. belong to callers).
    const bool use_heads = four && c->xcd_heads && !donation;
    uint32_t* heads = nullptr;
    if (use_heads) {
        if ((rc = ensure(c->heads, (size_t)kHeadRounds * sdk::kHeadWords * sizeof(uint32_t)))) return rc;
        uint32_t region = 0;
        if (plain) {
            region = c->heads_round++ % kHeadRounds;
            if (region == 0)
                HIPCALL(hipMemsetAsync(c->heads.p, 0, (size_t)kHeadRounds * sdk::kHeadWords * sizeof(uint32_t), c->stream));
        }
        heads = static_cast<uint32_t*>(c->heads.p) + (size_t)region * sdk::kHeadWords;
    } else if (plain) {
        HIPCALL(hipMemsetAsync(c->counter.p, 0, 8, c->stream));
    }
    a.next = use_heads ? heads + sdk::kHeadNext : static_cast<uint32_t*>(c->counter.p);
    a.heads = heads;
    a.stack = static_cast<uint32_t*>(c->stack.p);
    a.order = s.order;
    a.limit = s.limit;
    a.count = s.count;
    a.counts = s.counts;
    a.count_mode = count_mode;
    a.chunk = chunk;
    a.work_rounds = c->work_rounds;
    a.locked = c->locked;
    a.n_dev = s.n_dev;   // the plain and split launches of a prop32 fallback: the list's length
    // a first-solution scan (frontier_first): the plain QUAD launch cancels boards above the lowest hit
    if (four && !count_mode && plain) a.found = s.found;
    if (four && ph.kind == SolvePhase::kSplit) a.budget_big = ph.budget_big;   // (a device-counted batch)
    if (ph.kind == SolvePhase::kSplit && ph.save && four && !count_mode) {
        // the split phase leaves the stacks of the boards it stops (sdk::split_save4)
        a.save = c->dn_save.p;
        a.save_idx = static_cast<uint32_t*>(c->dn_save_idx.p);
    }
    unsigned grid_used = grid;
    if (four && !count_mode && donation) {
        // subtree donation: idle waves wait for items while any wave of the grid works, so the
        // grid is the resident one (its occupancy, not waves_per_cu2), whatever the batch size:
        // waves without a board of their own are the helpers
        if (c->dn_blocks_per_cu <= 0) {
            c->dn_blocks_per_cu = sdk::solve4_dn_blocks_per_cu();
            if (c->dn_blocks_per_cu <= 0) return fail(SDK_EHIP, "occupancy query for the donation kernel failed");
        }
        a.donate = ph.area;
        // the boards: a list length on the device (s.n_dev; n bounds it), one per dequeue on the
        // area's own counter
        a.chunk = 1;
        a.next = &static_cast<sdk::DnCtl*>(ph.area)->next;
        // the resident grid, at most what the kernel keeps of it for n boards: n / 4 + 64 + helpers x
        // min(n, kDnHelpCap) (solve4_kernel; the list on the device may be shorter, then it keeps less)
        grid_used = (unsigned)std::max<uint64_t>(
            1, std::min<uint64_t>({(uint64_t)c->cus * (uint64_t)std::min<int64_t>(c->dn_blocks_per_cu, c->waves_per_cu2),
                                   (uint64_t)sdk::kDnMbox,
                                   ((uint64_t)n + 3) / 4 + 64ull +
                                       (uint64_t)c->dn_helpers * std::min<uint64_t>(n, sdk::kDnHelpCap)}));
        if (grid_used > grid) {
            if ((rc = ensure(c->stack, (size_t)grid_used * stack_words * sizeof(uint32_t)))) return rc;
            a.stack = static_cast<uint32_t*>(c->stack.p);
        }
    }
    if ((rc = timer_begin(c, &stop))) return rc;
    if (four) {
        HIPCALL(sdk::launch_solve4(a, grid_used, c->stream));
    } else if (two) {
        HIPCALL(sdk::launch_solve2(a, grid, c->stream));
    } else {
        HIPCALL(sdk::launch_solve1(a, grid, c->stream));
    }
    return timer_end(c, stop);
}

// Solve launch.  QUAD solves with SDK_OPT_DONATE (LEX, or MRV_UNIQUE: its split phase counts to
// two completions and re-searches in LEX within the slot, like the plain launch) run in phases:
// every board first in
// the plain kernel with at most `split` search nodes (the C4/C2 path is that launch alone);
// the few boards that need more -- the launch's tail -- are gathered and solved again by
// solve4_kernel<true> on the full resident grid, where idle waves take subtrees of the
// heavy boards (subtree donation, solve4_kernel.h), and scattered back.  That second launch
// is exhaustive: MRV branching, at most two completions per board, every donated subtree
// needed work; a unique completion is the lex-first one.  The boards it finds several
// completions for (or cannot decide within the budget) are solved a third time in LEX
// order with donation.  Results are the ones a single slot finds (same boards and
// statuses; `work` adds up the phases and parts).
//
// Every phase is enqueued at once, without the host: the lists of boards a phase passes
// on live on the device (length word first), and the gather, donation and scatter kernels
// read their lengths there (an empty list costs a few microseconds of launches).  The
// phase buffers are sized for every board of the call, up to kDnCapBoards boards per
// phased pass; larger calls run in passes of that many.
constexpr uint64_t kDnCapBoards = 1ull << 24;

// List the boards of `from` (its statuses [0, n), n bounded by *n_dev when given) that carry `code`
// into tail `k`'s list (its length zeroed by the prep launch; k also numbers its dn_stat word and its
// donation area), copying their inputs and masks to the tail's dense batch.
// resume: the split phase's list -- boards with saved stacks go to the seed list, and
// dn_seed_kernel lists them after the restarted ones (donation area 0)
int dn_collect(sdk_ctx* c, const SolveCall& from, int8_t code, int k, bool resume) {
    DnTail& t = c->dn_tail[k];
    int rc;
    if ((rc = ensure(t.in, from.n * 81)) || (from.mask && (rc = ensure(t.mask, from.n * 2)))) return rc;
    sdk::DnResume rs{};
    if (resume) {
        rs.save = static_cast<const sdk::SplitSave*>(c->dn_save.p);
        rs.save_idx = static_cast<const uint32_t*>(c->dn_save_idx.p);
        rs.ctl = static_cast<sdk::DnCtl*>(c->dn.p);
        rs.seeds = static_cast<uint32_t*>(c->dn_seeds.p);
    }
    uint32_t* lst = static_cast<uint32_t*>(t.list.p);
    uint32_t* total = static_cast<uint32_t*>(c->dn_stat.p) + k;
    uint8_t* bin = static_cast<uint8_t*>(t.in.p);
    uint16_t* bmask = static_cast<uint16_t*>(from.mask ? t.mask.p : nullptr);
    HIPCALL(sdk::launch_dn_collect(from.status, from.n, from.n_dev, code, lst, total, from.in, from.mask, from.in_first,
                                   from.in_step, bin, bmask, rs, grid_for(c, from.n, 256, 8), c->stream));
    if (resume)
        HIPCALL(sdk::launch_dn_seed(rs.seeds, rs.save, lst, total, from.in, from.mask, from.in_first, from.in_step, bin,
                                    bmask, rs.ctl, grid_for(c, sdk::kSeedBoards, 1, 4), c->stream));
    return SDK_OK;
}

// Solve the (at most to.n) boards dn_collect listed in tail `k` with the donation kernel (`order`,
// to's budget) in donation area k, and scatter the answers into to's out, status and work.
// dequeue: the boards the donation launch dequeues when that is not the list's length (with
// resumed boards, the restarted ones alone).
int dn_resolve(sdk_ctx* c, const SolveCall& to, int k, int order, const uint32_t* dequeue = nullptr) {
    DnTail& t = c->dn_tail[k];
    int rc;
    if ((rc = ensure(t.out, to.n * 81)) || (rc = ensure(t.st, to.n)) || (to.work && (rc = ensure(t.work, to.n * 8))))
        return rc;
    const uint32_t* lst = static_cast<const uint32_t*>(t.list.p);
    SolveCall sub{static_cast<uint8_t*>(t.in.p), to.mask ? static_cast<uint16_t*>(t.mask.p) : nullptr,
                  static_cast<uint8_t*>(t.out.p), static_cast<int8_t*>(t.st.p),
                  to.work ? static_cast<uint64_t*>(t.work.p) : nullptr, to.n};
    sub.n_dev = dequeue ? dequeue : lst;
    sub.order = order;
    sub.budget = to.budget;
    sub.solver = to.solver;
    const SolvePhase ph{SolvePhase::kDonation, static_cast<char*>(c->dn.p) + (size_t)k * sdk::kDnBytes};
    if ((rc = launch_solve_once(c, sub, ph))) return rc;
    if (order == SDK_ORDER_MRV_UNIQUE) {
        // boards with several completions (or undecided): LEX order, donation again
        sub.n_dev = lst;
        if ((rc = dn_collect(c, sub, (int8_t)sdk::kDnRetryLex, 1, false)) ||
            (rc = dn_resolve(c, sub, 1, SDK_ORDER_LEX)))
            return rc;
    }
    HIPCALL(sdk::launch_dn_scatter(lst, sub.out, sub.status, sub.work, c->work_rounds == SDK_WORK_DEPTH, to.out,
                                   to.status, to.work, grid_for(c, to.n, 1, 16), c->stream));
    return SDK_OK;
}

// zero a phased pass's control words in one launch (sdk::dn_prep_kernel)
// resume: the pass saves the split phase's stacks (their buffers are sized and zeroed too)
int dn_prep(sdk_ctx* c, uint64_t cap, bool first_pass, bool resume) {
    int rc;
    if (c->dn.bytes < 2 * sdk::kDnBytes || c->dn_epoch > 0xFFFFFF00u) {
        // entries of epoch 0 (and, after 2^32 launches, the stale ones cleared once)
        if ((rc = ensure(c->dn, 2 * sdk::kDnBytes))) return rc;
        HIPCALL(hipMemsetAsync(c->dn.p, 0, 2 * sdk::kDnBytes, c->stream));
        c->dn_epoch = 0;
    }
    if ((rc = ensure(c->dn_stat, 256)) || (rc = ensure(c->counter, 256)) ||
        (rc = ensure(c->heads, (size_t)kHeadRounds * sdk::kHeadWords * sizeof(uint32_t))) ||
        (rc = ensure(c->dn_tail[0].list, (cap + 1) * sizeof(uint32_t))) ||
        (rc = ensure(c->dn_tail[1].list, (cap + 1) * sizeof(uint32_t))))
        return rc;
    sdk::DnPrep p{};
    p.counter = static_cast<uint32_t*>(c->counter.p);
    p.heads = c->xcd_heads ? static_cast<uint32_t*>(c->heads.p) : nullptr;
    p.heads_words = sdk::kHeadWords;   // the heads and the dequeue counter after them
    p.stat = first_pass ? static_cast<uint32_t*>(c->dn_stat.p) : nullptr;   // statistics add up over passes
    for (int k = 0; k < 2; ++k) {
        p.ctl[k] = reinterpret_cast<uint32_t*>(static_cast<char*>(c->dn.p) + (size_t)k * sdk::kDnBytes);
        p.epoch[k] = ++c->dn_epoch;
        p.list[k] = static_cast<uint32_t*>(c->dn_tail[k].list.p);
    }
    p.fault = c->dn_fault ? 1u : 0u;
    p.helpers = (uint32_t)c->dn_helpers;
    if (resume) {
        if ((rc = ensure(c->dn_save, sizeof(sdk::SplitSave))) || (rc = ensure(c->dn_save_idx, (size_t)cap * 4)) ||
            (rc = ensure(c->dn_seeds, (2 + 2 * (size_t)sdk::kSeedBoards) * 4)))
            return rc;
        p.seeds = static_cast<uint32_t*>(c->dn_seeds.p);
        p.save = static_cast<uint32_t*>(c->dn_save.p);
    }
    HIPCALL(sdk::launch_dn_prep(p, c->stream));
    return SDK_OK;
}

int launch_prop32_solve(sdk_ctx* c, const SolveCall& s);

// The solve launch described above kDnCapBoards.  Everything about the call is in `call`: of the
// context this reads options and workspaces and writes only the outcome fields (dn_ran, prop32_ran,
// dn_err_check).  The call's -1 fields are resolved once, here; the resolved call `s` is what the
// prop32 pass, the phases and the fallback get.
int launch_solve(sdk_ctx* c, const SolveCall& call) {
    SolveCall s = call;
    if (s.order < 0) s.order = c->order;
    if (s.budget < 0) s.budget = (int64_t)c->budget;
    if (s.donate < 0) s.donate = c->donate;
    if (s.solver < 0) s.solver = c->solver;
    const size_t n = s.n;
    const uint32_t* n_dev = s.n_dev;
    const uint64_t node_budget = (uint64_t)s.budget;
    if (!n_dev) c->prop32_ran = false;
    // the bit-sliced root propagation pass first (prop32_kernel.h): plain solves of whole batches
    // (no first-cell masks, work counters, strided inputs or first-solution scans), 16-byte
    // aligned, at least prop32_min boards; a budget of 1 node is left to solve4 (a board solved at
    // its root takes one); prop32 always runs locked-candidates passes, so with SDK_OPT_LOCKED 0
    // it only runs where no budget can tell the difference
    if (!n_dev && c->prop32 && s.solver == SDK_SOLVER_QUAD && !s.count_mode && s.out && s.status && !s.work &&
        !s.mask && s.in_first == 0 && s.in_step <= 1 && !s.found &&
        (node_budget == 0 || (node_budget >= 2 && c->locked)) &&
        (int64_t)n >= c->prop32_min && n <= kDnCapBoards &&
        ((reinterpret_cast<uintptr_t>(s.in) | reinterpret_cast<uintptr_t>(s.out)) & 15u) == 0)
        return launch_prop32_solve(c, s);
    const int64_t dn = s.donate;
    // the default split budget doubles above 2^19 SEARCHED boards (sdk::kBudgetBigBoards; a prop32
    // fallback batch's count is on the device, so its split launch picks the budget there): with ~30
    // boards per slot a heavy board's extra nodes overlap the bulk, and fewer boards reach the
    // donation launch (1M hard boards, 880k searched, LEX: 6.88 ms at 128, 6.14 at 256, 6.39 at 384;
    // 1M minimal, 460k searched: 2.68 ms at 128, 2.93 at 256; profiles/r05/sweep_phased_hard_r05s.log,
    // ab_lc_r05t.log)
    const bool split_auto = dn == 1;
    const uint64_t split = split_auto ? (!n_dev && n > sdk::kBudgetBigBoards ? 2 * kDnSplitDefault : kDnSplitDefault)
                                      : (uint64_t)dn;
    // (only where the node budget leaves room for it: with a budget B <= 256 a board needing
    // more than B nodes must end as a budget hit, which the split phase at 256 would solve)
    const uint64_t split_big = split_auto && n_dev && (node_budget == 0 || node_budget > 2 * kDnSplitDefault)
                                   ? 2 * kDnSplitDefault : 0;
    const bool two_phase = n > 0 && !s.count_mode && dn && s.solver == SDK_SOLVER_QUAD &&
                           (s.order == SDK_ORDER_LEX || s.order == SDK_ORDER_MRV_UNIQUE) && s.out && s.status &&
                           (node_budget == 0 || node_budget > split) &&
                           // a prop32 fallback batch (n_dev) holds only boards propagation left open:
                           // phased at any size (1M hard boards: 6.8 ms phased vs 8.3 in one launch,
                           // profiles/r05/ab_dnmax_r05r.log)
                           (c->dn_max == 0 || (int64_t)n <= c->dn_max || n_dev);
    c->dn_ran = two_phase;
    if (two_phase) c->dn_err_check = true;
    // resumed items keep the split phase's branching, so only MRV stacks resume, into the
    // exhaustive (MRV) donation launch: LEX items there cost more nodes than a restart in MRV
    // order (heavy 1000: 80k vs 61k nodes, 1.56 vs 1.30 ms), and LEX acceptance in a LEX
    // donation launch would need the closed prefixes MRV stacks do not have
    const bool resume = two_phase && c->dn_resume && c->dn_exhaustive && s.order == SDK_ORDER_MRV_UNIQUE;
    if (!two_phase) return launch_solve_once(c, s);
    if (n_dev && n > kDnCapBoards) return fail(SDK_EINVAL, "a device-counted batch is solved in one pass");
    // SDK_OPT_TIMING: the phases of one solve are one timed span
    TimedSpan span(c);
    int rc = span.begin();
    if (rc) return rc;
    const SolvePhase split_phase{SolvePhase::kSplit, nullptr, split_big, resume};
    const uint64_t step = s.in_step ? s.in_step : 1;
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        SolveCall pass = s;          // this pass's boards: kDnCapBoards of the call's from b0
        pass.n = std::min<uint64_t>(n - b0, kDnCapBoards);
        pass.out = s.out + b0 * 81;
        pass.status = s.status + b0;
        pass.work = s.work ? s.work + b0 : nullptr;
        pass.mask = s.mask ? s.mask + b0 : nullptr;
        pass.in_first = s.in_first + b0 * step;
        pass.in_step = step;
        SolveCall split_call = pass;  // ... every one of them first with the split budget
        split_call.budget = (int64_t)split;
        (void)((rc = dn_prep(c, pass.n, b0 == 0, resume)) ||
               (rc = launch_solve_once(c, split_call, split_phase)) ||
               (rc = dn_collect(c, pass, (int8_t)-2, 0, resume)) ||
               (rc = dn_resolve(c, pass, 0, c->dn_exhaustive ? SDK_ORDER_MRV_UNIQUE : SDK_ORDER_LEX,
                                resume ? static_cast<uint32_t*>(c->dn_seeds.p) + 1 : nullptr)));
    }
    return span.end(rc);
}

// The host side the two propagation passes share (prop32_kernel; the grading pass, grade32_kernel):
// workspaces, a pass's control words and common arguments, and the fallback over the boards it lists.
constexpr size_t kCtlBytes = (size_t)sdk::kP32Heads * sdk::kP32HeadStride * 4;   // the dequeue counters

// the pass's workspaces, for passes over at most `cap` boards
int p32_reserve(sdk_ctx* c, size_t cap) {
    int rc;
    if ((rc = ensure(c->p32_ctl, kCtlBytes)) || (rc = ensure(c->p32_list, (cap + 1) * 4)) ||
        (rc = ensure(c->p32_in, cap * 81)) || (rc = ensure(c->p32_out, cap * 81)) || (rc = ensure(c->p32_st, cap)))
        return rc;
    return SDK_OK;
}

// One pass over n boards: its dequeue counters and the list's length cleared (enqueued), and the
// arguments both kernels take; budget: the resolved node budget of the search that follows.
int p32_pass_begin(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, size_t n, int64_t budget,
                   sdk::Prop32Args* a) {
    HIPCALL(hipMemsetAsync(c->p32_ctl.p, 0, kCtlBytes, c->stream));
    HIPCALL(hipMemsetAsync(c->p32_list.p, 0, 4, c->stream));
    *a = sdk::Prop32Args{};
    a->in = in;
    a->out = out;
    a->status = status;
    a->n = n;
    a->heads = static_cast<uint32_t*>(c->p32_ctl.p);
    a->list = static_cast<uint32_t*>(c->p32_list.p);
    a->list_in = static_cast<uint8_t*>(c->p32_in.p);
    // the search continues from the propagated grids when no node budget applies (a budget counts
    // nodes from the input, so the statuses of budget hits would differ)
    a->handover = (c->prop32_handover && budget == 0) ? 1 : 0;
    return SDK_OK;
}

// The boards pass `a` listed (the list's length is on the device) through launch_solve -- `rest`
// names order, budget, donate and solver; the buffers are filled in here -- and their answers
// scattered back into the pass's out and status.
int p32_fallback(sdk_ctx* c, const sdk::Prop32Args& a, SolveCall rest) {
    rest.in = a.list_in;
    rest.out = static_cast<uint8_t*>(c->p32_out.p);
    rest.status = static_cast<int8_t*>(c->p32_st.p);
    rest.n = a.n;
    rest.n_dev = a.list;
    int rc = launch_solve(c, rest);
    if (rc) return rc;
    // one thread per 4 bytes of the list's boards (its length is on the device: sized for all n)
    if (sdk::launch_p32_scatter(rest.n_dev, rest.out, rest.status, a.in, a.out, a.status,
                                grid_for(c, a.n * 81, 1024, 8), c->stream) != hipSuccess)
        return fail(SDK_EHIP, "prop32 scatter launch failed");
    return SDK_OK;
}

// The prop32 pass (prop32_kernel.h) over the batch, then the boards it leaves undecided -- listed
// with their inputs on the device -- solved by the usual path (solve4, phased with donation when
// that applies) with the list's length read on the device, and their answers scattered back.
// Every launch is enqueued at once; an empty list costs the fallback's launches a few microseconds.
// `s` is the resolved call launch_solve's gate let through: plain (no masks, work counters, stride or
// found word), so the fallback is the same call over the list's boards.
int launch_prop32_solve(sdk_ctx* c, const SolveCall& s) {
    const size_t n = s.n;
    int rc;
    sdk::Prop32Args a;
    if ((rc = p32_reserve(c, n)) || (rc = p32_pass_begin(c, s.in, s.out, s.status, n, s.budget, &a))) return rc;
    // SDK_OPT_TIMING: two spans, the pass itself and its fallback (search + scatter) as one
    hipEvent_t stop;
    if ((rc = timer_begin(c, &stop))) return rc;
    a.lc_every = (uint32_t)std::max<int64_t>(1, c->prop32_lc & 0xFF);
    a.lc_first = (c->prop32_lc >> 8) ? (uint32_t)(c->prop32_lc >> 8) : a.lc_every;
    a.max_steps = 96;
    a.tail_live = a.handover ? (uint32_t)c->prop32_tail_live : 0u;
    a.tail_step = (uint32_t)c->prop32_tail_step;
    const unsigned grid = grid_for(c, n, 64, 20);   // a group of 64 boards per dequeue
    uint64_t* stamps = nullptr;
    if (c->clock_probe) {      // the diagnostic twin (sdk_debug_clock_arm)
        if ((rc = ensure(c->p32_stamps, (size_t)grid * 32))) return rc;
        stamps = static_cast<uint64_t*>(c->p32_stamps.p);
        c->p32_stamp_wgs = grid;
    }
    HIPCALL(sdk::launch_prop32(a, grid, c->stream, stamps));
    TimedSpan span(c);
    if ((rc = timer_end(c, stop)) || (rc = span.begin())) return rc;
    c->prop32_ran = true;
    SolveCall rest;     // the same order, budget, donate and solver over the list's boards
    rest.order = s.order;
    rest.budget = s.budget;
    rest.donate = s.donate;
    rest.solver = s.solver;
    return span.end(p32_fallback(c, a, rest));
}

// Classify launch (sdk_classify_batch): the solve path with ORDER_CLASSIFY -- the prop32 pass under
// the conditions a plain solve gets it (its statuses 1 and 0 are already "exactly one" and "none"),
// then ONE plain QUAD launch over the boards it left (no phases, no donation: launch_solve's
// two_phase is false for this order), whatever SDK_OPT_SOLVER and SDK_OPT_ORDER say.  Batches above
// kDnCapBoards (the pass's cap) go in slices of that many, so every slice gets the pass.
// budget: search nodes per board, -1 = the context's.
int launch_classify(sdk_ctx* c, const uint8_t* d_in, uint8_t* d_out, int8_t* d_status, size_t n, int64_t budget) {
    SolveCall s;
    s.order = sdk::ORDER_CLASSIFY;
    s.solver = SDK_SOLVER_QUAD;
    s.budget = budget;
    s.donate = 0;
    int rc = SDK_OK;
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        s.in = d_in + b0 * 81;
        s.out = d_out + b0 * 81;
        s.status = d_status + b0;
        s.n = std::min<uint64_t>(n - b0, kDnCapBoards);
        rc = launch_solve(c, s);
    }
    return rc;
}

// Grade launch (sdk_grade_batch; grade32_kernel.h): the grading pass over every slice of
// kDnCapBoards -- always, whatever SDK_OPT_PROP32* and the batch size, since the level is read from
// it; no tail hand-off (a tail snapshot is not a fixpoint) -- then the boards it lists through the
// classify search (launch_solve, ORDER_CLASSIFY, the list's length on the device), the usual scatter
// of their answers and the verdict kernel that keeps level 4 only for "exactly one".  Control words and
// the list are the prop32 pass's (re-initialised by every call that uses them).  One span under
// SDK_OPT_TIMING.  d_open null: the counts go to scratch.  d_out == d_in: a slice's inputs are
// copied aside first (the pass and the scatter read a board's input after its group's output is
// written).  budget as launch_classify's.  Outcome fields as a classify that ran the pass:
// prop32_ran (SDK_OPT_PROP32_UNDECIDED counts the last slice's listed boards), dn_ran false.
// d_bd non-null (sdk_rate_batch; rate32_kernel.h): the rate stage, per slice and behind its verdict
// kernel -- a slice's list is valid only inside its own iteration -- the slice's ratings filled with
// SDK_RATE_NONE, the dequeue counter (the pass's first control word, idle by then) cleared, and one
// wave per level-4 board of the list, whose length stays on the device.  The parents are the pass's
// inputs (the copy put aside when in place), the completions the slice's rows of d_out.  d_key
// nullable.  Without it the call enqueues exactly what it did before the stage existed.
// d_open4 non-null (sdk_subsets_batch; subsets_kernel.h): the subsets stage, in the same place and over
// the same work items -- the slice's counts filled with SDK_SUBSETS_NONE, the same counter cleared, one
// half-wave per level-4 board of the list.  It reads the parents only.  Without the pointer nothing of
// it is enqueued.
// d_open5 non-null (sdk_fish_batch; fish_kernel.h): the fish stage, where the subsets stage sits and in
// place of it -- it computes both counts.  Both columns filled with 0xFF, the same counter cleared, the
// same grid (one half-wave per level-4 board of the list, four waves per SIMD).  d_open4 null: the slice's
// open4 goes to the context's f5_open4.  Without the pointer nothing of it is enqueued.
// d_open6 non-null (sdk_wings_batch; wings_kernel.h): the wings stage, where the fish stage sits and in place
// of it -- it computes all three counts.  The three columns filled with 0xFF, the same counter cleared, the
// fish stage's grid.  d_open4 or d_open5 null: the slice's counts go to the context's f5_open4 / w6_open5.
// Without the pointer nothing of it is enqueued.
// d_open7 non-null (sdk_chains_batch; chains_kernel.h): the chains stage, where the wings stage sits and in
// place of it -- it computes all four counts.  The four columns filled with 0xFF, the same counter cleared, the
// fish stage's grid.  d_open4, d_open5 or d_open6 null: the slice's counts go to the context's f5_open4 /
// w6_open5 / c7_open6.  Without the pointer nothing of it is enqueued.
// The columns of a grade call beside out and status, one byte per board: level always, the others nullable.
struct GradeCols {
    uint8_t *level, *open;
    uint8_t *backdoors, *key;   // the rate stage (sdk_rate_batch)
    uint8_t* open4;             // the subsets stage (sdk_subsets_batch)
    uint8_t* open5 = nullptr;   // the fish stage (sdk_fish_batch), which fills open4 too
    uint8_t* open6 = nullptr;   // the wings stage (sdk_wings_batch), which fills open4 and open5 too
    uint8_t* open7 = nullptr;   // the chains stage (sdk_chains_batch), which fills open4, open5 and open6 too
};

int launch_grade(sdk_ctx* c, const uint8_t* d_in, uint8_t* d_out, int8_t* d_status, const GradeCols& cols, size_t n,
                 int64_t budget) {
    if (n == 0) return SDK_OK;
    uint8_t *const d_level = cols.level, *const d_open = cols.open, *const d_bd = cols.backdoors,
                   *const d_key = cols.key, *const d_open4 = cols.open4, *const d_open5 = cols.open5,
                   *const d_open6 = cols.open6, *const d_open7 = cols.open7;
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    if (budget < 0) budget = (int64_t)c->budget;
    const uint64_t cap = std::min<uint64_t>(n, kDnCapBoards);
    const bool in_place = d_in == d_out;
    int rc;
    if ((rc = p32_reserve(c, cap)) || (in_place && (rc = ensure(c->gr_in, cap * 81))) ||
        (!d_open && (rc = ensure(c->gr_open, cap))) ||
        ((d_open5 || d_open6 || d_open7) && !d_open4 && (rc = ensure(c->f5_open4, cap))) ||
        ((d_open6 || d_open7) && !d_open5 && (rc = ensure(c->w6_open5, cap))) ||
        (d_open7 && !d_open6 && (rc = ensure(c->c7_open6, cap))))
        return rc;
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        const uint8_t* in = d_in + b0 * 81;
        if (in_place) {
            HIPCALL(hipMemcpyAsync(c->gr_in.p, in, m * 81, hipMemcpyDeviceToDevice, c->stream));
            in = static_cast<const uint8_t*>(c->gr_in.p);
        }
        sdk::Grade32Args a{};
        if ((rc = p32_pass_begin(c, in, d_out + b0 * 81, d_status + b0, m, budget, &a.p))) break;
        a.level = d_level + b0;
        a.open = d_open ? d_open + b0 : static_cast<uint8_t*>(c->gr_open.p);
        HIPCALL(sdk::launch_grade32(a, grid_for(c, m, 64, 20), c->stream));
        c->prop32_ran = true;
        SolveCall rest;
        rest.order = sdk::ORDER_CLASSIFY;
        rest.solver = SDK_SOLVER_QUAD;
        rest.budget = budget;
        rest.donate = 0;
        if ((rc = p32_fallback(c, a.p, rest))) break;
        if (sdk::launch_g32_verdict(a.p.list, static_cast<const int8_t*>(c->p32_st.p), a.level, a.open,
                                    grid_for(c, m, 256, 8), c->stream) != hipSuccess)
            rc = fail(SDK_EHIP, "grade verdict launch failed");
        if (!rc && d_bd) {
            sdk::Rate32Args r{};
            r.in = in;
            r.sol = a.p.out;
            r.level = a.level;
            r.list = a.p.list;
            r.n = m;
            r.next = a.p.heads;
            r.backdoors = d_bd + b0;
            r.key = d_key ? d_key + b0 : nullptr;
            r.lc_every = (uint32_t)std::max<int64_t>(1, c->prop32_lc & 0xFF);
            r.lc_first = (c->prop32_lc >> 8) ? (uint32_t)(c->prop32_lc >> 8) : r.lc_every;
            HIPCALL(hipMemsetAsync(r.backdoors, 0xFF, m, c->stream));
            if (r.key) HIPCALL(hipMemsetAsync(r.key, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(r.next, 0, 4, c->stream));
            // four waves per SIMD, as the grader; at most one wave per listed board
            if (sdk::launch_rate32(r, grid_for(c, m, 1, 16), c->stream) != hipSuccess)
                rc = fail(SDK_EHIP, "rate launch failed");
        }
        if (!rc && d_open7) {
            sdk::Chains32Args w{};
            w.in = in;
            w.level = a.level;
            w.list = a.p.list;
            w.n = m;
            w.next = a.p.heads;
            w.open4 = d_open4 ? d_open4 + b0 : static_cast<uint8_t*>(c->f5_open4.p);
            w.open5 = d_open5 ? d_open5 + b0 : static_cast<uint8_t*>(c->w6_open5.p);
            w.open6 = d_open6 ? d_open6 + b0 : static_cast<uint8_t*>(c->c7_open6.p);
            w.open7 = d_open7 + b0;
            HIPCALL(hipMemsetAsync(w.open4, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.open5, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.open6, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.open7, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.next, 0, 4, c->stream));
            // four waves per SIMD; at most one wave per two listed boards
            if (sdk::launch_chains32(w, grid_for(c, m, 2, 16), c->stream) != hipSuccess)
                rc = fail(SDK_EHIP, "chains launch failed");
        } else if (!rc && d_open6) {
            sdk::Wings32Args w{};
            w.in = in;
            w.level = a.level;
            w.list = a.p.list;
            w.n = m;
            w.next = a.p.heads;
            w.open4 = d_open4 ? d_open4 + b0 : static_cast<uint8_t*>(c->f5_open4.p);
            w.open5 = d_open5 ? d_open5 + b0 : static_cast<uint8_t*>(c->w6_open5.p);
            w.open6 = d_open6 + b0;
            HIPCALL(hipMemsetAsync(w.open4, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.open5, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.open6, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(w.next, 0, 4, c->stream));
            // four waves per SIMD; at most one wave per two listed boards
            if (sdk::launch_wings32(w, grid_for(c, m, 2, 16), c->stream) != hipSuccess)
                rc = fail(SDK_EHIP, "wings launch failed");
        } else if (!rc && d_open5) {
            sdk::Fish32Args f{};
            f.in = in;
            f.level = a.level;
            f.list = a.p.list;
            f.n = m;
            f.next = a.p.heads;
            f.open4 = d_open4 ? d_open4 + b0 : static_cast<uint8_t*>(c->f5_open4.p);
            f.open5 = d_open5 + b0;
            HIPCALL(hipMemsetAsync(f.open4, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(f.open5, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(f.next, 0, 4, c->stream));
            // four waves per SIMD; at most one wave per two listed boards
            if (sdk::launch_fish32(f, grid_for(c, m, 2, 16), c->stream) != hipSuccess)
                rc = fail(SDK_EHIP, "fish launch failed");
        } else if (!rc && d_open4) {
            sdk::Subsets32Args s{};
            s.in = in;
            s.level = a.level;
            s.list = a.p.list;
            s.n = m;
            s.next = a.p.heads;
            s.open4 = d_open4 + b0;
            HIPCALL(hipMemsetAsync(s.open4, 0xFF, m, c->stream));
            HIPCALL(hipMemsetAsync(s.next, 0, 4, c->stream));
            // four waves per SIMD; at most one wave per two listed boards
            if (sdk::launch_subsets32(s, grid_for(c, m, 2, 16), c->stream) != hipSuccess)
                rc = fail(SDK_EHIP, "subsets launch failed");
        }
    }
    return span.end(rc);
}

// Canonical forms (sdk_canonical_batch; canon_kernel.h): per slice of kDnCapBoards, the classify path
// (launch_classify: its statuses and completions, under every option and budget) and then one launch of
// the canonical-form kernel, one wave per board, at most 16 one-wave workgroups per CU (four waves per
// SIMD).  The completions go to d_solution, or to the context's cn_sol where the caller wants none; the
// kernel overwrites an eligible board's completion with its canonical solution in place.  d_canon may be
// d_in: classify has read a slice's boards before the kernel writes them, and a wave reads its board before
// it writes.  One span under SDK_OPT_TIMING; outcome fields as the classify of the last slice.
struct CanonCols {
    uint8_t *solution, *gather, *relabel;
    uint16_t* ties;
};

int launch_canonical(sdk_ctx* c, const uint8_t* d_in, uint8_t* d_canon, int8_t* d_status, const CanonCols& cols,
                     size_t n, int64_t budget) {
    if (n == 0) return SDK_OK;
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_canon)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    const uint64_t cap = std::min<uint64_t>(n, kDnCapBoards);
    int rc;
    if (!cols.solution && (rc = ensure(c->cn_sol, cap * 81))) return rc;
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        uint8_t* sol = cols.solution ? cols.solution + b0 * 81 : static_cast<uint8_t*>(c->cn_sol.p);
        if ((rc = launch_classify(c, d_in + b0 * 81, sol, d_status + b0, m, budget))) break;
        sdk::CanonArgs a{};
        a.in = d_in + b0 * 81;
        a.sol = sol;
        a.status = d_status + b0;
        a.n = m;
        a.canon = d_canon + b0 * 81;
        a.solution = cols.solution ? sol : nullptr;
        a.gather = cols.gather ? cols.gather + b0 * 81 : nullptr;
        a.relabel = cols.relabel ? cols.relabel + b0 * 10 : nullptr;
        a.ties = cols.ties ? cols.ties + b0 : nullptr;
        if (sdk::launch_canon(a, grid_for(c, m, 1, 16), c->stream) != hipSuccess)
            rc = fail(SDK_EHIP, "canonical-form launch failed");
    }
    return span.end(rc);
}

// Greedy clue removal (sdk_minimize_batch; minimize_kernel.h): the inputs' verdicts, then 81 rounds
// of (round kernel, classify of the candidates with no budget) and a last commit, all enqueued on
// the stream with no host synchronisation.  Under SDK_OPT_TIMING the whole call is one span.
// Batches above kDnCapBoards go in slices of that many (a slice's 81 rounds, then the next).
int launch_minimize(sdk_ctx* c, const uint8_t* d_in, const uint8_t* d_order, uint8_t* d_out, int8_t* d_status,
                    size_t n) {
    if (n == 0) return SDK_OK;
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    const uint64_t cap = std::min<uint64_t>(n, kDnCapBoards);
    int rc;
    if ((rc = ensure(c->mz_cand, cap * 81)) || (rc = ensure(c->mz_out, cap * 81)) || (rc = ensure(c->mz_st, cap)))
        return rc;
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    uint8_t* cand = static_cast<uint8_t*>(c->mz_cand.p);
    uint8_t* scratch = static_cast<uint8_t*>(c->mz_out.p);
    int8_t* cst = static_cast<int8_t*>(c->mz_st.p);
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        sdk::MinRoundArgs a{};
        a.cur = d_out + b0 * 81;
        a.order = d_order + b0 * 81;
        a.status = d_status + b0;
        a.cst = cst;
        a.n = m;
        const unsigned grid = grid_for(c, m * 81, sdk::kMinBlockBytes, 8);
        // the inputs' verdicts (the completions go to scratch: `out` starts as the inputs)
        rc = launch_classify(c, d_in + b0 * 81, scratch, d_status + b0, m, 0);
        for (uint32_t q = 0; q <= 81 && !rc; ++q) {
            a.src = q == 0 ? d_in + b0 * 81 : a.cur;
            a.cand = q < 81 ? cand : nullptr;
            a.q = q;
            if (sdk::launch_minimize_round(a, grid, c->stream) != hipSuccess)
                rc = fail(SDK_EHIP, "minimise round launch failed");
            if (!rc && q < 81) rc = launch_classify(c, cand, scratch, cst, m, 0);
        }
    }
    return span.end(rc);
}

// Random complete grids (sdk_generate_grids; generate_kernel.h): rows [0, n) are stream indices
// first .. first + n - 1 of `seed`; the removal orders and placement counts are optional.  One
// persistent launch per slice of kDnCapBoards rows (the dequeue counter is 32 bits wide).  Under
// SDK_OPT_TIMING the call is one span (nothing of its own under an outer span).
int launch_generate(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint8_t* d_grids, uint8_t* d_order,
                    uint32_t* d_plc) {
    if (n == 0) return SDK_OK;
    int rc;
    if ((rc = ensure(c->counter, 256))) return rc;
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    for (uint64_t b0 = 0; b0 < n; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        sdk::GenArgs a{};
        a.seed_mul = seed * 0x100000001B3ull;
        a.first = first + b0;
        a.n = (uint32_t)m;
        a.cap = (uint32_t)c->gen_cap;
        a.hard = std::max(a.cap, sdk::kGenFloor);
        a.grids = d_grids + b0 * 81;
        a.order = d_order ? d_order + b0 * 81 : nullptr;
        a.placements = d_plc ? d_plc + b0 : nullptr;
        a.next = static_cast<uint32_t*>(c->counter.p);
        HIPCALL(hipMemsetAsync(c->counter.p, 0, 8, c->stream));
        HIPCALL(sdk::launch_generate_grids(a, grid_for(c, m, sdk::kGenThreads, sdk::kGenWavesPerCu), c->stream));
    }
    return span.end(SDK_OK);
}

// Minimal puzzles (sdk_generate_puzzles): per slice of kDnCapBoards rows, the grids and their
// removal orders (into the context's gen_order), then the minimiser over them -- make_minimal's
// rows, all enqueued without the host.  One span under SDK_OPT_TIMING.
int launch_generate_puzzles(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint8_t* d_puzzles, uint8_t* d_grids,
                            int8_t* d_status) {
    if (n == 0) return SDK_OK;
    if ((reinterpret_cast<uintptr_t>(d_puzzles) | reinterpret_cast<uintptr_t>(d_grids)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    int rc;
    if ((rc = ensure(c->gen_order, std::min<uint64_t>(n, kDnCapBoards) * 81))) return rc;
    uint8_t* d_order = static_cast<uint8_t*>(c->gen_order.p);
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        if ((rc = launch_generate(c, seed, first + b0, m, d_grids + b0 * 81, d_order, nullptr))) break;
        rc = launch_minimize(c, d_grids + b0 * 81, d_order, d_puzzles + b0 * 81, d_status + b0, m);
    }
    return span.end(rc);
}

// Level-minimal clue removal (sdk_minimize_level_batch; reduce32_kernel.h): per slice of kDnCapBoards
// boards the pass's dequeue counters cleared and ONE launch -- a group's eligibility run and its 81
// rounds are inside the kernel.  A group reads its own 64 input rows only (at its begin, and those of
// its ineligible boards at its end, before it writes) and writes only its own rows, so d_out may be
// d_in with nothing put aside.  One span under SDK_OPT_TIMING.
int launch_reduce_level(sdk_ctx* c, const uint8_t* d_in, const uint8_t* d_order, int level, uint8_t* d_out,
                        int8_t* d_status, size_t n) {
    if (n == 0) return SDK_OK;
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    int rc;
    if ((rc = ensure(c->p32_ctl, kCtlBytes))) return rc;
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    for (uint64_t b0 = 0; b0 < n; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        sdk::Reduce32Args a{};
        a.p.in = d_in + b0 * 81;
        a.p.out = d_out + b0 * 81;
        a.p.n = m;
        a.p.heads = static_cast<uint32_t*>(c->p32_ctl.p);
        a.order = d_order + b0 * 81;
        a.status = d_status + b0;
        a.level = (uint32_t)level;
        HIPCALL(hipMemsetAsync(c->p32_ctl.p, 0, kCtlBytes, c->stream));
        // three waves per SIMD (reduce32_kernel's registers), one wave per group of 64 boards
        if (sdk::launch_reduce32(a, grid_for(c, m, 64, 12), c->stream) != hipSuccess) {
            rc = fail(SDK_EHIP, "level minimise launch failed");
            break;
        }
    }
    return span.end(rc);
}

// Level-minimal puzzles (sdk_generate_level): per slice of kDnCapBoards rows, the grids and their
// removal orders (into the context's gen_order), then the level minimiser over them -- as
// launch_generate_puzzles with the other minimiser.  One span under SDK_OPT_TIMING.
int launch_generate_level(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, int level, uint8_t* d_puzzles,
                          uint8_t* d_grids, int8_t* d_status) {
    if (n == 0) return SDK_OK;
    if ((reinterpret_cast<uintptr_t>(d_puzzles) | reinterpret_cast<uintptr_t>(d_grids)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    int rc;
    if ((rc = ensure(c->gen_order, std::min<uint64_t>(n, kDnCapBoards) * 81))) return rc;
    uint8_t* d_order = static_cast<uint8_t*>(c->gen_order.p);
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    for (uint64_t b0 = 0; b0 < n && !rc; b0 += kDnCapBoards) {
        const uint64_t m = std::min<uint64_t>(n - b0, kDnCapBoards);
        if ((rc = launch_generate(c, seed, first + b0, m, d_grids + b0 * 81, d_order, nullptr))) break;
        rc = launch_reduce_level(c, d_grids + b0 * 81, d_order, level, d_puzzles + b0 * 81, d_status + b0, m);
    }
    return span.end(rc);
}

int check_level_arg(int level) {
    if (level < SDK_GRADE_NAKED || level > SDK_GRADE_LOCKED)
        return fail(SDK_EINVAL, "level must be SDK_GRADE_NAKED..SDK_GRADE_LOCKED (1..3), got %d", level);
    return SDK_OK;
}

// argument checks of the four generate calls
int check_generate_args(uint64_t first, size_t n) {
    int rc;
    if ((rc = check_board_count(n))) return rc;
    if (first > UINT64_MAX - (uint64_t)n) return fail(SDK_EINVAL, "first + n overflows the stream index");
    return SDK_OK;
}

// Graded generation (sdk_generate_graded; select_kernel.h): the window [first, first + max_scan) in
// rounds of m stream indices.  A round is launch_generate_puzzles into the context's work buffers,
// launch_grade of those puzzles with no budget (completions and verdicts to scratch: grading in place
// would overwrite the puzzles), the three selection launches behind the hits of the earlier rounds,
// and ONE 8-byte readback of the call's device word -- the only host round trip.  The scan stops when
// the word's total reaches n or the window ends.  The outputs depend on the rounds in no way: a
// round's hits are ranked behind all earlier ones, ranks >= n are never written, and `scanned` comes
// from the position of the hit of rank n - 1 (SelWord::last), not from the rounds run.
//   chunk != 0: every round is min(chunk, rest of the window) indices.
//   chunk == 0: the first round is 4 n indices, a later one what the hit rate so far asks for the
//               missing hits plus a quarter (twice the last round while nothing was hit), each within
//               kGradedAutoMin .. kGradedAutoMax.
// The work buffers hold whole tiles of 64 rows (the selection kernels load whole tiles).  One span
// under SDK_OPT_TIMING.  The outputs are device pointers; *found / *scanned are the host's.
constexpr uint64_t kGradedChunkMax = 1ull << 24;   // = kDnCapBoards: a round is one slice of generate and grade
constexpr uint64_t kGradedAutoMin = 4096, kGradedAutoMax = 1ull << 20;

struct GradedCall {
    uint64_t seed, first;
    uint32_t n;
    uint32_t level_mask, clues_lo, clues_hi;
    uint64_t max_scan, chunk;
    uint8_t *puzzles, *grids, *level, *open;
    uint64_t* index;
    // sdk_generate_rated: a level-4 candidate is a hit only with bd_lo <= backdoors <= bd_hi; a round's
    // grade then runs the rate stage (skipped when level 4 is not asked for: nothing would be filtered,
    // and the outputs of levels 1..3 are SDK_RATE_NONE anyway)
    bool rated = false;
    uint32_t bd_lo = 0, bd_hi = 64;
    uint8_t *backdoors = nullptr, *key = nullptr;
    // sdk_generate_subsets: the same with o4_lo <= open4 <= o4_hi and the subsets stage
    bool subsets = false;
    uint32_t o4_lo = 0, o4_hi = 64;
    uint8_t* open4 = nullptr;
    // sdk_generate_fish: both o4_lo <= open4 <= o4_hi and o5_lo <= open5 <= o5_hi, and the fish stage
    bool fish = false;
    uint32_t o5_lo = 0, o5_hi = 64;
    uint8_t* open5 = nullptr;
    // sdk_generate_wings: both o5_lo <= open5 <= o5_hi and o6_lo <= open6 <= o6_hi, and the wings stage
    bool wings = false;
    uint32_t o6_lo = 0, o6_hi = 64;
    uint8_t* open6 = nullptr;
    // sdk_generate_chains: both o6_lo <= open6 <= o6_hi and o7_lo <= open7 <= o7_hi, and the chains stage
    bool chains = false;
    uint32_t o7_lo = 0, o7_hi = 64;
    uint8_t* open7 = nullptr;
};

// One round's selection (select_kernel.h): rows [0, m) of caller-supplied buffers -- a round of
// launch_generate_graded, or the rows of sdk_select_rows_dev -- ranked behind the d_word->total hits of
// the earlier rounds.  This is the only place that fills the three argument structs and makes the
// three launches; it enqueues, and neither allocates, reads back nor synchronizes: the caller sizes the
// per-tile buffers (ballot, popcount, offset) before its first launch and its timing span -- a grow is a
// hipFree, which waits for the device -- and reads the word.  puzzles and grids hold whole tiles.
struct SelectRound {
    const uint8_t *puzzles, *grids;
    const int8_t* status;
    const uint8_t *level, *open;
    const uint8_t *backdoors, *key, *open4;     // nullable
    uint32_t m;
    uint64_t first;                             // stream index of row 0
    uint32_t n;                                 // the quota
    uint32_t level_mask, clues_lo, clues_hi, bd_lo, bd_hi, o4_lo, o4_hi;
    uint8_t *out_puzzles, *out_grids;
    uint8_t *out_level, *out_open;              // nullable, as the rest
    uint64_t* out_index;
    uint8_t *out_backdoors, *out_key, *out_open4;
};

int launch_select_round(sdk_ctx* c, const SelectRound& r, sdk::SelWord* d_word) {
    const uint32_t tiles = (r.m + sdk::kSelTileRows - 1) / sdk::kSelTileRows;
    if (c->gg_ballot.bytes < (size_t)tiles * 8 || c->gg_count.bytes < (size_t)tiles * 4 ||
        c->gg_offset.bytes < (size_t)tiles * 4)
        return fail(SDK_EINVAL, "selection buffers not sized before the round");
    sdk::SelFlagArgs fa{};
    fa.puzzles = r.puzzles;
    fa.status = r.status;
    fa.level = r.level;
    fa.m = r.m;
    fa.level_mask = r.level_mask;
    fa.clues_lo = r.clues_lo;
    fa.clues_hi = r.clues_hi;
    fa.backdoors = r.backdoors;
    fa.bd_lo = r.bd_lo;
    fa.bd_hi = r.bd_hi;
    fa.open4 = r.open4;
    fa.o4_lo = r.o4_lo;
    fa.o4_hi = r.o4_hi;
    fa.ballot = static_cast<unsigned long long*>(c->gg_ballot.p);
    fa.count = static_cast<uint32_t*>(c->gg_count.p);
    sdk::SelScanArgs sa{};
    sa.count = fa.count;
    sa.offset = static_cast<uint32_t*>(c->gg_offset.p);
    sa.tiles = tiles;
    sa.word = d_word;
    sdk::SelScatterArgs ca{};
    ca.puzzles = r.puzzles;
    ca.grids = r.grids;
    ca.level = r.level;
    ca.open = r.open;
    ca.ballot = fa.ballot;
    ca.offset = sa.offset;
    ca.first = r.first;
    ca.n = r.n;
    ca.out_puzzles = r.out_puzzles;
    ca.out_grids = r.out_grids;
    ca.out_level = r.out_level;
    ca.out_open = r.out_open;
    ca.out_index = r.out_index;
    ca.backdoors = r.backdoors;
    ca.key = r.key;
    ca.out_backdoors = r.out_backdoors;
    ca.out_key = r.out_key;
    ca.open4 = r.open4;
    ca.out_open4 = r.out_open4;
    ca.word = d_word;
    HIPCALL(sdk::launch_select_flag(fa, tiles, c->stream));
    HIPCALL(sdk::launch_select_scan(sa, c->stream));
    HIPCALL(sdk::launch_select_scatter(ca, tiles, c->stream));
    return SDK_OK;
}

int launch_generate_graded(sdk_ctx* c, const GradedCall& g, uint64_t* found, uint64_t* scanned) {
    if ((reinterpret_cast<uintptr_t>(g.puzzles) | reinterpret_cast<uintptr_t>(g.grids)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(g.index) & 7u) return fail(SDK_EINVAL, "index must be 8-byte aligned");
    int rc;
    if ((rc = ensure(c->gg_word, sizeof(sdk::SelWord)))) return rc;
    sdk::SelWord* d_word = static_cast<sdk::SelWord*>(c->gg_word.p);
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    HIPCALL(hipMemsetAsync(d_word, 0, sizeof(sdk::SelWord), c->stream));
    uint64_t done = 0, hits = 0, last_m = 0;
    while (done < g.max_scan) {
        const uint64_t rest = g.max_scan - done;
        uint64_t m = g.chunk;
        if (!m) {
            if (!done)
                m = 4ull * g.n;
            else if (!hits)
                m = 2 * last_m;
            else {
                // (n - hits) < 2^31 and done < 2^64 / 2^31 whenever the product matters: the quotient is
                // clamped to 2^20 anyway, so saturate instead of overflowing
                const uint64_t miss = g.n - hits;
                const uint64_t need = done > UINT64_MAX / miss ? kGradedAutoMax : miss * done / hits;
                m = need + need / 4;
            }
            m = std::min(std::max(m, kGradedAutoMin), kGradedAutoMax);
        }
        m = std::min(m, rest);
        last_m = m;
        const uint32_t tiles = (uint32_t)((m + sdk::kSelTileRows - 1) / sdk::kSelTileRows);
        const size_t rows = (size_t)tiles * sdk::kSelTileRows;
        if ((rc = ensure(c->gg_puz, rows * 81)) || (rc = ensure(c->gg_grid, rows * 81)) ||
            (rc = ensure(c->gg_sol, rows * 81)) || (rc = ensure(c->gg_st, rows)) || (rc = ensure(c->gg_gst, rows)) ||
            (rc = ensure(c->gg_level, rows)) || (rc = ensure(c->gg_open, rows)) ||
            // (launch_select_round's per-tile buffers)
            (rc = ensure(c->gg_ballot, (size_t)tiles * 8)) || (rc = ensure(c->gg_count, (size_t)tiles * 4)) ||
            (rc = ensure(c->gg_offset, (size_t)tiles * 4)))
            return rc;
        const bool rate = g.rated && (g.level_mask >> SDK_GRADE_SEARCH & 1u);
        if (rate && ((rc = ensure(c->gg_bd, rows)) || (rc = ensure(c->gg_key, rows)))) return rc;
        uint8_t* bd = rate ? static_cast<uint8_t*>(c->gg_bd.p) : nullptr;
        uint8_t* key = rate ? static_cast<uint8_t*>(c->gg_key.p) : nullptr;
        const bool fish = g.fish && (g.level_mask >> SDK_GRADE_SEARCH & 1u);
        const bool subsets = fish || (g.subsets && (g.level_mask >> SDK_GRADE_SEARCH & 1u));
        const bool wings = g.wings && (g.level_mask >> SDK_GRADE_SEARCH & 1u);
        const bool chains = g.chains && (g.level_mask >> SDK_GRADE_SEARCH & 1u);
        if ((subsets && (rc = ensure(c->gg_o4, rows))) || ((fish || wings) && (rc = ensure(c->gg_o5, rows))) ||
            ((wings || chains) && (rc = ensure(c->gg_o6, rows))) || (chains && (rc = ensure(c->gg_o7, rows))))
            return rc;
        uint8_t* o4 = subsets ? static_cast<uint8_t*>(c->gg_o4.p) : nullptr;
        uint8_t* o5 = (fish || wings) ? static_cast<uint8_t*>(c->gg_o5.p) : nullptr;
        uint8_t* o6 = (wings || chains) ? static_cast<uint8_t*>(c->gg_o6.p) : nullptr;
        uint8_t* o7 = chains ? static_cast<uint8_t*>(c->gg_o7.p) : nullptr;
        uint8_t* puz = static_cast<uint8_t*>(c->gg_puz.p);
        uint8_t* grid = static_cast<uint8_t*>(c->gg_grid.p);
        int8_t* st = static_cast<int8_t*>(c->gg_st.p);
        uint8_t* level = static_cast<uint8_t*>(c->gg_level.p);
        uint8_t* open = static_cast<uint8_t*>(c->gg_open.p);
        if ((rc = launch_generate_puzzles(c, g.seed, g.first + done, m, puz, grid, st)) ||
            (rc = launch_grade(c, puz, static_cast<uint8_t*>(c->gg_sol.p), static_cast<int8_t*>(c->gg_gst.p),
                               GradeCols{level, open, bd, key, o4, o5, o6, o7}, m, 0)))
            return rc;
        SelectRound r{};
        r.puzzles = puz;
        r.grids = grid;
        r.status = st;
        r.level = level;
        r.open = open;
        r.backdoors = bd;
        r.key = key;
        r.open4 = o4;
        r.m = (uint32_t)m;
        r.first = g.first + done;
        r.n = g.n;
        r.level_mask = g.level_mask;
        r.clues_lo = g.clues_lo;
        r.clues_hi = g.clues_hi;
        r.bd_lo = g.bd_lo;
        r.bd_hi = g.bd_hi;
        r.o4_lo = g.o4_lo;
        r.o4_hi = g.o4_hi;
        r.out_puzzles = g.puzzles;
        r.out_grids = g.grids;
        r.out_level = g.level;
        r.out_open = g.open;
        r.out_index = g.index;
        r.out_backdoors = g.backdoors;
        r.out_key = g.key;
        r.out_open4 = g.open4;
        if (g.fish) {
            // The selection kernels carry two nullable rating columns with a range each, and both "none"
            // markers are 0xFF: a fish call's open5 column and range go through the `backdoors` slot with
            // `key` null (a fish call is never rated), its open4 through the `open4` slot as above.
            r.backdoors = o5;
            r.bd_lo = g.o5_lo;
            r.bd_hi = g.o5_hi;
            r.out_backdoors = g.open5;
        }
        if (g.wings) {
            // The same slots once more: a wings call's open6 column and range go through the `backdoors` slot
            // with `key` null, its open5 and range through the `open4` slot (open4 itself is not filtered).
            r.backdoors = o6;
            r.bd_lo = g.o6_lo;
            r.bd_hi = g.o6_hi;
            r.out_backdoors = g.open6;
            r.open4 = o5;
            r.o4_lo = g.o5_lo;
            r.o4_hi = g.o5_hi;
            r.out_open4 = g.open5;
        }
        if (g.chains) {
            // And once more: a chains call's open7 column and range go through the `backdoors` slot with `key`
            // null, its open6 and range through the `open4` slot (open4 and open5 are not filtered).
            r.backdoors = o7;
            r.bd_lo = g.o7_lo;
            r.bd_hi = g.o7_hi;
            r.out_backdoors = g.open7;
            r.open4 = o6;
            r.o4_lo = g.o6_lo;
            r.o4_hi = g.o6_hi;
            r.out_open4 = g.open6;
        }
        if ((rc = launch_select_round(c, r, d_word))) return rc;
        sdk::SelWord word;
        HIPCALL(hipMemcpyAsync(&word, d_word, sizeof word, hipMemcpyDeviceToHost, c->stream));
        HIPCALL(hipStreamSynchronize(c->stream));
        hits = word.total;
        if (hits >= g.n) {
            if (word.last == 0 || word.last > m) return fail(SDK_EHIP, "graded selection lost the position of its last hit");
            *found = g.n;
            *scanned = done + word.last;
            return span.end(SDK_OK);
        }
        done += m;
    }
    *found = hits;
    *scanned = g.max_scan;
    return span.end(SDK_OK);
}

// argument checks of sdk_generate_graded and its _dev form
int check_graded_args(uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                      uint64_t max_scan, uint64_t chunk) {
    int rc;
    if ((rc = check_board_count(n))) return rc;
    if (level_mask == 0 || (level_mask & ~0x1Eu)) return fail(SDK_EINVAL, "level_mask must be a non-empty set of bits 1..4");
    if (clues_lo > clues_hi || clues_hi > 81) return fail(SDK_EINVAL, "clue range must be clues_lo <= clues_hi <= 81");
    if (max_scan == 0) return fail(SDK_EINVAL, "max_scan must be at least 1");
    if (first > UINT64_MAX - max_scan) return fail(SDK_EINVAL, "first + max_scan overflows the stream index");
    if (chunk > kGradedChunkMax) return fail(SDK_EINVAL, "chunk must be 0 (automatic) or 1..2^24");
    return SDK_OK;
}

// ... and the backdoor range of sdk_generate_rated
int check_rated_range(uint32_t lo, uint32_t hi) {
    if (lo > hi || hi > 64) return fail(SDK_EINVAL, "backdoor range must be backdoors_lo <= backdoors_hi <= 64");
    return SDK_OK;
}

// ... and the open4 range of sdk_generate_subsets
int check_subsets_range(uint32_t lo, uint32_t hi) {
    if (lo > hi || hi > 64) return fail(SDK_EINVAL, "open4 range must be open4_lo <= open4_hi <= 64");
    return SDK_OK;
}

// ... and the open5 range of sdk_generate_fish
int check_fish_range(uint32_t lo, uint32_t hi) {
    if (lo > hi || hi > 64) return fail(SDK_EINVAL, "open5 range must be open5_lo <= open5_hi <= 64");
    return SDK_OK;
}

// ... and the open6 range of sdk_generate_wings
int check_wings_range(uint32_t lo, uint32_t hi) {
    if (lo > hi || hi > 64) return fail(SDK_EINVAL, "open6 range must be open6_lo <= open6_hi <= 64");
    return SDK_OK;
}

// ... and the open7 range of sdk_generate_chains
int check_chains_range(uint32_t lo, uint32_t hi) {
    if (lo > hi || hi > 64) return fail(SDK_EINVAL, "open7 range must be open7_lo <= open7_hi <= 64");
    return SDK_OK;
}

uint8_t* u8(void* p) { return static_cast<uint8_t*>(p); }

// sdk_grade_batch, sdk_rate_batch, sdk_subsets_batch, sdk_fish_batch, sdk_wings_batch, sdk_chains_batch and their _dev forms, behind each
// one's own test of its required pointers: `cols` holds the columns the entry point has, the others null.  host: the pointers
// are the caller's arrays, staged through the context's buffers (the same ones whichever family calls);
// else they are device pointers and the call only enqueues.
int grade_call(sdk_ctx* c, bool host, const void* in, void* out, void* status, const GradeCols& cols, size_t n,
               uint64_t node_budget) {
    int rc;
    if ((rc = check_budget_arg(node_budget))) return rc;
    if (n == 0) return SDK_OK;
    if ((rc = check_board_count(n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if (!host)
        return launch_grade(c, static_cast<const uint8_t*>(in), u8(out), static_cast<int8_t*>(status), cols, n,
                            budget_arg(node_budget));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->out, n * 81)) || (rc = ensure(c->status, n)) ||
        (rc = ensure(c->gr_level, n)) || (cols.open && (rc = ensure(c->gr_open, n))) ||
        (cols.backdoors && (rc = ensure(c->rt_bd, n))) || (cols.key && (rc = ensure(c->rt_key, n))) ||
        (cols.open4 && (rc = ensure(c->s4_open4, n))) || (cols.open5 && (rc = ensure(c->f5_open5, n))) ||
        (cols.open6 && (rc = ensure(c->w6_open6, n))) || (cols.open7 && (rc = ensure(c->c7_open7, n))))
        return rc;
    uint8_t* d_in = u8(c->in.p);
    uint8_t* d_out = u8(c->out.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    const GradeCols d{u8(c->gr_level.p), cols.open ? u8(c->gr_open.p) : nullptr,
                      cols.backdoors ? u8(c->rt_bd.p) : nullptr, cols.key ? u8(c->rt_key.p) : nullptr,
                      cols.open4 ? u8(c->s4_open4.p) : nullptr, cols.open5 ? u8(c->f5_open5.p) : nullptr,
                      cols.open6 ? u8(c->w6_open6.p) : nullptr, cols.open7 ? u8(c->c7_open7.p) : nullptr};
    // a column comes back iff the caller has it (a slot each, present or not)
    auto column = [n](const uint8_t* dev, uint8_t* dst) { return Piece{dst ? n : 0, nullptr, nullptr, dev, dst}; };
    Staging io(c, {{n * 81, in, d_in, d_out, out},
                   {n, nullptr, nullptr, d_status, status},
                   column(d.level, cols.level),
                   column(d.open, cols.open),
                   column(d.backdoors, cols.backdoors),
                   column(d.key, cols.key),
                   column(d.open4, cols.open4),
                   column(d.open5, cols.open5),
                   column(d.open6, cols.open6),
                   column(d.open7, cols.open7)});
    if ((rc = io.send()) || (rc = launch_grade(c, d_in, d_out, d_status, d, n, budget_arg(node_budget)))) return rc;
    return io.fetch();
}

// sdk_generate_graded, sdk_generate_rated, sdk_generate_subsets, sdk_generate_fish, sdk_generate_wings, sdk_generate_chains and their _dev forms:
// `g` is the call with the caller's pointers (its n is set here, from the checked `n`).  host: they are host arrays, and the
// rows found come back through the context's gg_out_* buffers; else they are device pointers.  The order
// of the checks is the order of the errors a caller with several bad arguments sees.
int graded_call(sdk_ctx* c, bool host, size_t n, GradedCall g, uint64_t* found, uint64_t* scanned) {
    if (!c || !found || (n && (!g.puzzles || !g.grids))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_graded_args(g.first, n, g.level_mask, g.clues_lo, g.clues_hi, g.max_scan, g.chunk)) ||
        (g.rated && (rc = check_rated_range(g.bd_lo, g.bd_hi))) ||
        (g.subsets && (rc = check_subsets_range(g.o4_lo, g.o4_hi))) ||
        (g.fish && ((rc = check_subsets_range(g.o4_lo, g.o4_hi)) || (rc = check_fish_range(g.o5_lo, g.o5_hi)))) ||
        (g.wings && ((rc = check_fish_range(g.o5_lo, g.o5_hi)) || (rc = check_wings_range(g.o6_lo, g.o6_hi)))) ||
        (g.chains && ((rc = check_wings_range(g.o6_lo, g.o6_hi)) || (rc = check_chains_range(g.o7_lo, g.o7_hi)))))
        return rc;
    if (!host) {
        if ((reinterpret_cast<uintptr_t>(g.puzzles) | reinterpret_cast<uintptr_t>(g.grids)) & 15u)
            return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(g.index) & 7u) return fail(SDK_EINVAL, "d_index must be 8-byte aligned");
    }
    g.n = (uint32_t)n;
    uint64_t f = 0, s = 0;
    if (n) {
        std::lock_guard<std::mutex> lk(c->mu);
        HIPCALL(hipSetDevice(c->device));
        GradedCall d = g;   // the call on device pointers
        if (host) {
            // at most min(n, max_scan) rows can come back
            const size_t rows = (size_t)std::min<uint64_t>(n, g.max_scan);
            if ((rc = ensure(c->gg_out_puz, rows * 81)) || (rc = ensure(c->gg_out_grid, rows * 81)) ||
                (g.level && (rc = ensure(c->gg_out_level, rows))) || (g.open && (rc = ensure(c->gg_out_open, rows))) ||
                (g.backdoors && (rc = ensure(c->gg_out_bd, rows))) || (g.key && (rc = ensure(c->gg_out_key, rows))) ||
                (g.open4 && (rc = ensure(c->gg_out_o4, rows))) || (g.open5 && (rc = ensure(c->gg_out_o5, rows))) ||
                (g.open6 && (rc = ensure(c->gg_out_o6, rows))) || (g.open7 && (rc = ensure(c->gg_out_o7, rows))) ||
                (g.index && (rc = ensure(c->gg_out_index, rows * 8))))
                return rc;
            d.puzzles = u8(c->gg_out_puz.p);
            d.grids = u8(c->gg_out_grid.p);
            d.level = g.level ? u8(c->gg_out_level.p) : nullptr;
            d.open = g.open ? u8(c->gg_out_open.p) : nullptr;
            d.backdoors = g.backdoors ? u8(c->gg_out_bd.p) : nullptr;
            d.key = g.key ? u8(c->gg_out_key.p) : nullptr;
            d.open4 = g.open4 ? u8(c->gg_out_o4.p) : nullptr;
            d.open5 = g.open5 ? u8(c->gg_out_o5.p) : nullptr;
            d.open6 = g.open6 ? u8(c->gg_out_o6.p) : nullptr;
            d.open7 = g.open7 ? u8(c->gg_out_o7.p) : nullptr;
            d.index = g.index ? static_cast<uint64_t*>(c->gg_out_index.p) : nullptr;
        }
        if ((rc = launch_generate_graded(c, d, &f, &s))) return rc;
        if (host && f) {
            // the rows found, and nothing behind them
            auto column = [f](const uint8_t* dev, uint8_t* dst) { return Piece{dst ? f : 0, nullptr, nullptr, dev, dst}; };
            Staging io(c, {{g.index ? f * 8 : 0, nullptr, nullptr, d.index, g.index},
                           {f * 81, nullptr, nullptr, d.puzzles, g.puzzles},
                           {f * 81, nullptr, nullptr, d.grids, g.grids},
                           column(d.level, g.level),
                           column(d.open, g.open),
                           column(d.backdoors, g.backdoors),
                           column(d.key, g.key),
                           column(d.open4, g.open4),
                           column(d.open5, g.open5),
                           column(d.open6, g.open6),
                           column(d.open7, g.open7)});
            if ((rc = io.fetch())) return rc;
        }
    }
    *found = f;
    if (scanned) *scanned = s;
    return SDK_OK;
}

// the arguments every graded family has, as a call without a stage
GradedCall graded_args(uint64_t seed, uint64_t first, uint32_t level_mask, uint32_t clues_lo, uint32_t clues_hi,
                       uint64_t max_scan, uint64_t chunk, void* puzzles, void* grids, void* level, void* open,
                       void* index) {
    return GradedCall{seed, first, 0, level_mask, clues_lo, clues_hi, max_scan, chunk, u8(puzzles), u8(grids),
                      u8(level), u8(open), static_cast<uint64_t*>(index)};
}
GradedCall rated_args(GradedCall g, uint32_t lo, uint32_t hi, void* backdoors, void* key) {
    g.rated = true;
    g.bd_lo = lo;
    g.bd_hi = hi;
    g.backdoors = u8(backdoors);
    g.key = u8(key);
    return g;
}
GradedCall subsets_args(GradedCall g, uint32_t lo, uint32_t hi, void* open4) {
    g.subsets = true;
    g.o4_lo = lo;
    g.o4_hi = hi;
    g.open4 = u8(open4);
    return g;
}
GradedCall fish_args(GradedCall g, uint32_t lo4, uint32_t hi4, uint32_t lo5, uint32_t hi5, void* open4, void* open5) {
    g.fish = true;
    g.o4_lo = lo4;
    g.o4_hi = hi4;
    g.o5_lo = lo5;
    g.o5_hi = hi5;
    g.open4 = u8(open4);
    g.open5 = u8(open5);
    return g;
}

GradedCall wings_args(GradedCall g, uint32_t lo5, uint32_t hi5, uint32_t lo6, uint32_t hi6, void* open5, void* open6) {
    g.wings = true;
    g.o5_lo = lo5;
    g.o5_hi = hi5;
    g.o6_lo = lo6;
    g.o6_hi = hi6;
    g.open5 = u8(open5);
    g.open6 = u8(open6);
    return g;
}

GradedCall chains_args(GradedCall g, uint32_t lo6, uint32_t hi6, uint32_t lo7, uint32_t hi7, void* open6, void* open7) {
    g.chains = true;
    g.o6_lo = lo6;
    g.o6_hi = hi6;
    g.o7_lo = lo7;
    g.o7_hi = hi7;
    g.open6 = u8(open6);
    g.open7 = u8(open7);
    return g;
}

// Deterministic breadth-first frontier of one board, left in c->fr_a.
// Every rank that builds it from the same board gets the same boards in the same
// order, so ranks can split it without exchanging boards.
//   SDK_FRONTIER_COUNT: MRV branching; solved leaves are counted (fr_leaves) and dropped.
//   SDK_FRONTIER_FIRST: lex branching, solved leaves kept in place, so the frontier is
//                       in lex order of completions (see frontier_kernel.h).
// Expansion stops once the frontier holds >= target boards (or nothing branches).
// Breadth-first expansion of the frontier in fr_a (m0 boards; level 0 applies the
// first-cell mask in fr_mask when `use_mask`) until it reaches `target` boards.  Buffers
// are sized once for the whole build, so the levels are enqueued without the host: a level
// is expanded only while the frontier is below `target` (or at level 0), and a level with
// more than `cap` children is rejected.
constexpr uint64_t kFrontierCap = 1ull << 25;  // 32M boards (2.6 GB) per frontier buffer

// boards a frontier buffer must hold for a build from m0 boards towards `target`
uint64_t frontier_capacity(uint64_t m0, uint64_t target) {
    const uint64_t m_exp = std::max<uint64_t>(m0, std::min(target, kFrontierCap));
    return std::max<uint64_t>(1, std::min(kFrontierCap, 9 * m_exp));
}

// The caller has put the m0 boards in fr_a, sized for frontier_capacity(m0, target) boards
// BEFORE seeding it (a later grow would drop them).
// use_mask: fr_mask holds one first-cell mask per seed board (level 0 applies them);
// force0: level 0 is expanded whatever the seed count (a seed board's mask lives only in that
// level, and sdk_expand_boards always wants at least one level).
int run_frontier_levels(sdk_ctx* c, uint64_t m0, bool use_mask, int mode, uint64_t target, bool force0) {
    int rc;
    const bool first = mode == SDK_FRONTIER_FIRST;
    const uint64_t m_exp = std::max<uint64_t>(m0, std::min(target, kFrontierCap));
    const uint64_t c_out = frontier_capacity(m0, target);
    const uint64_t tiles = (m_exp + sdk::kScanTile - 1) / sdk::kScanTile;
    if (c->fr_a.bytes < c_out * 81) return fail(SDK_EINVAL, "frontier buffer not sized before seeding");
    if ((rc = ensure(c->fr_b, c_out * 81)) || (rc = ensure(c->fr_mask, 16)) ||
        (rc = ensure(c->prop, m_exp * 81)) || (rc = ensure(c->bcell, m_exp)) || (rc = ensure(c->bmask, m_exp * 2)) ||
        (rc = ensure(c->nchild, m_exp * 4)) || (rc = ensure(c->offs, m_exp * 8)) || (rc = ensure(c->tsum, tiles * 8)) ||
        (rc = ensure(c->fr_ctl, sizeof(sdk::FrontierCtl))))
        return rc;
    sdk::FrontierCtl* ctl = static_cast<sdk::FrontierCtl*>(c->fr_ctl.p);
    sdk::FrontierCtl h{};
    h.m = m0;
    HIPCALL(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    void* buf[2] = {c->fr_a.p, c->fr_b.p};
    const unsigned eg = grid_for(c, m_exp, sdk::kChunk, c->waves_per_cu);
    const bool quad = c->solver == SDK_SOLVER_QUAD;
    const unsigned eg4 = grid_for(c, m_exp, 4, c->waves_per_cu2);
    const unsigned sg = grid_for(c, m_exp, sdk::kScanTile, 4);   // (m_exp >= 1: no grid is empty)
    const unsigned gg = grid_for(c, m_exp, 1, 32);
    hipEvent_t stop;
    if ((rc = timer_begin(c, &stop))) return rc;
    constexpr int kLevelsPerSync = 4;
    for (int level = 0; level < 81; ++level) {
        const int in = level & 1;
        HIPCALL(sdk::launch_frontier_begin(ctl, target, level == 0 && force0 ? 1 : 0, c->stream));
        sdk::ExpandArgs ea;
        ea.in = static_cast<const uint8_t*>(buf[in]);
        ea.ctl = ctl;
        ea.prop = static_cast<uint8_t*>(c->prop.p);
        ea.bcell = static_cast<uint8_t*>(c->bcell.p);
        ea.bmask = static_cast<uint16_t*>(c->bmask.p);
        ea.nchild = static_cast<uint32_t*>(c->nchild.p);
        ea.order = first ? sdk::ORDER_LEX : sdk::ORDER_MRV;
        ea.mask = (level == 0 && use_mask) ? static_cast<const uint16_t*>(c->fr_mask.p) : nullptr;
        ea.keep_leaves = first ? 1 : 0;
        if (quad)   // four boards per wave (expand4_kernel.h): the same frontier, byte for byte
            HIPCALL(sdk::launch_expand4(ea, eg4, c->stream));
        else
            HIPCALL(sdk::launch_expand(ea, eg, c->stream));
        uint64_t* offs = static_cast<uint64_t*>(c->offs.p);
        uint64_t* tsum = static_cast<uint64_t*>(c->tsum.p);
        HIPCALL(sdk::launch_scan_tiles(ea.nchild, offs, ctl, tsum, sg, c->stream));
        HIPCALL(sdk::launch_scan_top(tsum, ctl, c_out, c->stream));
        HIPCALL(sdk::launch_emit(ea.prop, ea.bcell, ea.bmask, offs, tsum, ctl, static_cast<uint8_t*>(buf[in ^ 1]), gg,
                                 c->stream));
        HIPCALL(sdk::launch_frontier_end(ctl, first ? 1 : 0, c->stream));
        if (level % kLevelsPerSync == kLevelsPerSync - 1 || level == 80) {
            HIPCALL(hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, c->stream));
            HIPCALL(hipStreamSynchronize(c->stream));
            if (h.done) break;
        }
    }
    if ((rc = timer_end(c, stop))) return rc;
    HIPCALL(hipStreamSynchronize(c->stream));
    if (h.level & 1) std::swap(c->fr_a, c->fr_b);   // the final frontier lives in fr_a
    c->fr_size = h.m;
    c->fr_leaves = h.leaves;
    c->fr_levels = h.level;
    c->fr_valid = true;
    return SDK_OK;
}

int build_frontier(sdk_ctx* c, const uint8_t* h_board, const uint16_t* h_mask, int mode, uint64_t target) {
    c->fr_valid = false;
    c->fr_mode = mode;
    if (target == 0) target = (uint64_t)c->cus * (uint64_t)c->waves_per_cu * 8ull;
    int rc;
    if ((rc = ensure(c->fr_a, frontier_capacity(1, target) * 81)) || (rc = ensure(c->fr_mask, 16))) return rc;
    HIPCALL(hipMemcpyAsync(c->fr_a.p, h_board, 81, hipMemcpyHostToDevice, c->stream));
    if (h_mask) HIPCALL(hipMemcpyAsync(c->fr_mask.p, h_mask, 2, hipMemcpyHostToDevice, c->stream));
    return run_frontier_levels(c, 1, h_mask != nullptr, mode, target, h_mask != nullptr);
}

// Keep frontier boards first, first+step, ... < end of the current (count-mode) frontier and
// expand them further, on this device alone, until they number `target`: the second,
// rank-local stage of a frontier split, so a rank's share of a replicated frontier can be
// small and cheap to build; with step 1 and a short range, a rank's last heavy subtrees
// split into second-level records for the rebalanced count.  The leaves reported are those
// met during this refinement.
int refine_frontier(sdk_ctx* c, uint64_t first, uint64_t step, uint64_t end, uint64_t target) {
    if (!c->fr_valid) return fail(SDK_EINVAL, "no frontier: call sdk_frontier_build first");
    if (step == 0) return fail(SDK_EINVAL, "step must be >= 1");
    const uint64_t m = std::min(end, c->fr_size);
    const uint64_t n = first < m ? (m - first + step - 1) / step : 0;
    c->fr_valid = false;
    target = std::max<uint64_t>(target, n);
    int rc;
    // fr_b takes the share and becomes fr_a: size it for the whole refinement now
    if ((rc = ensure(c->fr_b, frontier_capacity(std::max<uint64_t>(n, 1), target) * 81))) return rc;
    if (n) {
        HIPCALL(sdk::launch_gather_boards(static_cast<const uint8_t*>(c->fr_a.p), first, step, n,
                                          static_cast<uint8_t*>(c->fr_b.p), grid_for(c, n, 4, 16), c->stream));
    }
    std::swap(c->fr_a, c->fr_b);
    if (n == 0) {
        c->fr_size = 0;
        c->fr_leaves = 0;
        c->fr_levels = 0;
        c->fr_valid = true;
        return SDK_OK;
    }
    return run_frontier_levels(c, n, false, c->fr_mode, target, false);
}

// Boards [lo, mid) of the current frontier refined as refine_frontier does (step 1), followed by
// boards [mid, hi) unchanged: a first-solution search splits the one board that hit its node
// budget (mid = lo + 1) without expanding the rest of its live range.  In first mode the result
// is still sorted by completion (the refined boards' children keep their order and precede
// board mid's completions).
int refine_head(sdk_ctx* c, uint64_t lo, uint64_t mid, uint64_t hi, uint64_t target) {
    if (!c->fr_valid) return fail(SDK_EINVAL, "no frontier: call sdk_frontier_build first");
    hi = std::min(hi, c->fr_size);
    lo = std::min(lo, hi);
    mid = std::min(std::max(mid, lo), hi);
    const uint64_t tail = hi - mid;
    int rc;
    if (tail) {   // the kept boards go aside first: the refinement reuses both frontier buffers
        if ((rc = ensure(c->fr_tail, tail * 81))) return rc;
        HIPCALL(hipMemcpyAsync(c->fr_tail.p, static_cast<const char*>(c->fr_a.p) + mid * 81, tail * 81,
                               hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = refine_frontier(c, lo, 1, mid, target))) return rc;
    if (!tail) return SDK_OK;
    const uint64_t h = c->fr_size;
    c->fr_valid = false;
    if (c->fr_a.bytes < (h + tail) * 81) {
        DevBuf nb;
        if ((rc = ensure(nb, (h + tail) * 81))) return rc;
        if (h) HIPCALL(hipMemcpyAsync(nb.p, c->fr_a.p, h * 81, hipMemcpyDeviceToDevice, c->stream));
        HIPCALL(hipStreamSynchronize(c->stream));
        c->fr_a.swap(nb);          // the old buffer goes with nb
    }
    HIPCALL(hipMemcpyAsync(static_cast<char*>(c->fr_a.p) + h * 81, c->fr_tail.p, tail * 81, hipMemcpyDeviceToDevice,
                           c->stream));
    c->fr_size = h + tail;
    c->fr_valid = true;
    return SDK_OK;
}

// Lex-ordered (SDK_FRONTIER_FIRST) breadth-first expansion of n seed boards, each with its own
// first-cell mask, at least one level deep and on until the frontier holds >= target boards;
// the frontier is copied to the host.  Children keep their parents' order, so the result is
// sorted by the completions below each board (see frontier_kernel.h): the worklist step of a
// resumable lex-first search (search.py), which expands the boards that hit the node budget.
int expand_boards(sdk_ctx* c, const uint8_t* h_in, const uint16_t* h_masks, uint64_t n, uint64_t target,
                  uint8_t* h_out, uint64_t cap, uint64_t* out_n) {
    c->fr_valid = false;
    c->fr_mode = SDK_FRONTIER_FIRST;
    *out_n = 0;
    if (n == 0) return SDK_OK;
    if (n > kFrontierCap) return fail(SDK_EINVAL, "at most %llu seed boards", (unsigned long long)kFrontierCap);
    int rc;
    if ((rc = ensure(c->fr_a, frontier_capacity(n, target) * 81)) || (rc = ensure(c->fr_mask, n * 2))) return rc;
    // (the seed boards sit at offset 0, where every type is aligned; the masks after them, at 81 n,
    // are copied as bytes)
    Staging seeds(c, {{n * 81, h_in, c->fr_a.p}, {n * 2, h_masks, c->fr_mask.p}});
    // run_frontier_levels synchronizes before returning, so the area is free for the frontier, whose
    // size is known only then: a staging of its own (nothing comes back through the seeds' one,
    // whose fetch() only ends it)
    if ((rc = seeds.send()) || (rc = run_frontier_levels(c, n, h_masks != nullptr, SDK_FRONTIER_FIRST, target, true)) ||
        (rc = seeds.fetch()))
        return rc;
    if (c->fr_size > cap)
        return fail(SDK_EINVAL, "frontier of %llu boards exceeds cap %llu (pass cap >= 9 * max(n, target))",
                    (unsigned long long)c->fr_size, (unsigned long long)cap);
    if (c->fr_size) {
        Staging frontier(c, {{c->fr_size * 81, nullptr, nullptr, c->fr_a.p, h_out}});
        if ((rc = frontier.fetch())) return rc;
    }
    *out_n = c->fr_size;
    return SDK_OK;
}

// Count the completions below frontier boards first, first+step, ... < end into
// d_result = {count (u64), boards that hit the node budget (u64)}.
int frontier_count(sdk_ctx* c, uint64_t first, uint64_t step, uint64_t end, uint64_t limit,
                   unsigned long long* d_result) {
    if (!c->fr_valid) return fail(SDK_EINVAL, "no frontier: call sdk_frontier_build first");
    if (step == 0) return fail(SDK_EINVAL, "step must be >= 1");
    end = std::min(end, c->fr_size);
    const uint64_t n = first < end ? (end - first + step - 1) / step : 0;
    int rc;
    if ((rc = ensure(c->counter, 256)) || (rc = ensure(c->fr_status, std::max<uint64_t>(n, 1)))) return rc;
    unsigned long long* d_count = static_cast<unsigned long long*>(c->counter.p) + 3;
    HIPCALL(hipMemsetAsync(d_count, 0, 8, c->stream));
    if (n) {
        SolveCall s{static_cast<uint8_t*>(c->fr_a.p), nullptr, nullptr, static_cast<int8_t*>(c->fr_status.p), nullptr, n};
        s.in_first = first;
        s.in_step = step;
        s.count_mode = 1;
        s.limit = limit;
        s.count = d_count;
        if ((rc = launch_solve(c, s))) return rc;
    }
    HIPCALL(sdk::launch_count_result(static_cast<int8_t*>(c->fr_status.p), n, d_count, d_result, c->stream));
    return SDK_OK;
}

// Lex-ordered scan step of a first-solution search: solve frontier boards [lo, hi)
// and leave the lowest hit in d_found / d_best (first_hit_kernel).
int frontier_first(sdk_ctx* c, uint64_t lo, uint64_t hi, long long* d_found, uint8_t* d_best) {
    if (!c->fr_valid) return fail(SDK_EINVAL, "no frontier: call sdk_frontier_build first");
    hi = std::min(hi, c->fr_size);
    const uint64_t n = lo < hi ? hi - lo : 0;
    int rc;
    if ((rc = ensure(c->out, std::max<uint64_t>(n, 1) * 81)) || (rc = ensure(c->status, std::max<uint64_t>(n, 1))))
        return rc;
    if (n) {
        // boards above the lowest hit are cancelled inside the launch (solve4_kernel<.., FS>):
        // d_found is its found word until first_hit_kernel writes the answer.  The plain kernel
        // (no subtree donation: a heavy board is split by the caller, shard.sharded_solve)
        HIPCALL(sdk::launch_first_init(d_found, c->stream));
        SolveCall s{static_cast<uint8_t*>(c->fr_a.p), nullptr, static_cast<uint8_t*>(c->out.p),
                    static_cast<int8_t*>(c->status.p), nullptr, n};
        s.in_first = lo;
        s.donate = 0;
        s.found = d_found;
        if ((rc = launch_solve(c, s))) return rc;
    }
    HIPCALL(sdk::launch_first_hit(static_cast<int8_t*>(c->status.p), static_cast<uint8_t*>(c->out.p), n, lo, d_found,
                                  d_best, c->stream));
    return SDK_OK;
}

// Single-process form of the frontier count (sdk_count_solutions[_slice]): this
// rank's contiguous slice; rank 0 adds the leaves met during expansion.
int count_slice(sdk_ctx* c, const uint8_t* h_board, uint64_t limit, int rank, int world, uint64_t* local_count,
                uint64_t* frontier_size, int8_t* status) {
    if (world < 1 || rank < 0 || rank >= world) return fail(SDK_EINVAL, "bad rank %d / world %d", rank, world);
    int rc = build_frontier(c, h_board, nullptr, SDK_FRONTIER_COUNT,
                            (uint64_t)c->cus * (uint64_t)c->waves_per_cu * 8ull * (uint64_t)world);
    if (rc) return rc;
    const uint64_t m = c->fr_size;
    const uint64_t lo = (rank * m) / world, hi = ((rank + 1) * m) / world;
    if ((rc = ensure(c->counter, 256))) return rc;   // before taking an address inside it
    unsigned long long* d_res = static_cast<unsigned long long*>(c->counter.p) + 6;
    if ((rc = frontier_count(c, lo, 1, hi, limit, d_res))) return rc;
    unsigned long long res[2] = {0, 0};
    HIPCALL(hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    uint64_t cnt = res[0] + (rank == 0 ? c->fr_leaves : 0);
    if (limit && cnt > limit) cnt = limit;
    *local_count = cnt;
    if (frontier_size) *frontier_size = m;
    *status = res[1] ? (int8_t)-2 : (cnt > 0 ? (int8_t)1 : (int8_t)0);
    return SDK_OK;
}

#define NCCLCALL(expr)                                                                        \
    do {                                                                                      \
        ncclResult_t r_ = (expr);                                                             \
        if (r_ != ncclSuccess)                                                                \
            return fail(SDK_ECOMM, "%s: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

}  // namespace

extern "C" {

int sdk_abi_version(void) { return SDK_ABI_VERSION; }

const char* sdk_last_error(void) { return g_last_error.c_str(); }

int sdk_device_count(int* count) {
    if (!count) return fail(SDK_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return SDK_OK;
}

int sdk_create(int device, sdk_ctx** out) {
    if (!out) return fail(SDK_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIPCALL(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(SDK_EINVAL, "device %d out of range (%d devices)", device, n);
    HIPCALL(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCALL(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SDK_EINVAL, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    sdk_ctx* c = new (std::nothrow) sdk_ctx();
    if (!c) return fail(SDK_ENOMEM, "context allocation failed");
    c->device = device;
    c->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(SDK_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    (void)stage_host(c->stage, kStageInit);   // best effort: a failure leaves the pageable path
    *out = c;
    return SDK_OK;
}

int sdk_destroy(sdk_ctx* c) {
    if (!c) return SDK_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    // every DevBuf member frees itself in `delete c` below (on this device)
    if (c->stage.p) (void)hipHostFree(c->stage.p);
    for (auto& pr : c->events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    (void)hipStreamDestroy(c->stream);
    delete c;
    return SDK_OK;
}

// diagnostics (not in the header): the donation control block of the last donating launch
extern "C" int sdk_debug_dn_ctl(sdk_ctx* c, uint32_t* out16) {
    if (!c || !out16) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    std::memset(out16, 0, 64);
    if (!c->dn.p) return SDK_OK;
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipMemcpyAsync(out16, c->dn.p, 64, hipMemcpyDeviceToHost, c->stream));   // the global words
    HIPCALL(hipStreamSynchronize(c->stream));
    return SDK_OK;
}

// diagnostics (not in the header): the in-kernel clock of the prop32 pass.  Armed, the context's
// prop32 passes run prop32_clock_kernel, which stamps s_memtime / s_memrealtime at each workgroup's
// entry and exit; _read waits for the last such pass and returns the shader clock of its workgroups
// (GHz: shader ticks per 10 ns of the 100 MHz real-time counter) as median, 10th and 90th percentile
// and mean (out4), and how many workgroups it had.  (MI355X_MICROARCH.md, "DVFS give-back" item 6.)
extern "C" int sdk_debug_clock_arm(sdk_ctx* c, int on) {
    if (!c) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    c->clock_probe = on ? 1 : 0;
    return SDK_OK;
}

extern "C" int sdk_debug_clock_read(sdk_ctx* c, double* out4, int64_t* workgroups) {
    if (!c || !out4 || !workgroups) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *workgroups = 0;
    for (int i = 0; i < 4; ++i) out4[i] = 0.0;
    if (!c->p32_stamp_wgs || !c->p32_stamps.p) return SDK_OK;
    HIPCALL(hipSetDevice(c->device));
    std::vector<uint64_t> h((size_t)c->p32_stamp_wgs * 4);
    HIPCALL(hipMemcpyAsync(h.data(), c->p32_stamps.p, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    std::vector<double> ghz;
    ghz.reserve(c->p32_stamp_wgs);
    for (size_t w = 0; w < c->p32_stamp_wgs; ++w) {
        const uint64_t dt = h[4 * w + 2] - h[4 * w], dr = h[4 * w + 3] - h[4 * w + 1];
        if (dr >= 10 && h[4 * w + 2] > h[4 * w]) ghz.push_back((double)dt / (double)dr / 10.0);   // >= 0.1 us
    }
    if (ghz.empty()) return SDK_OK;
    std::sort(ghz.begin(), ghz.end());
    double sum = 0.0;
    for (double v : ghz) sum += v;
    out4[0] = ghz[ghz.size() / 2];
    out4[1] = ghz[ghz.size() / 10];
    out4[2] = ghz[(ghz.size() * 9) / 10];
    out4[3] = sum / (double)ghz.size();
    *workgroups = (int64_t)ghz.size();
    return SDK_OK;
}

// diagnostics (not in the header): what the last solve's prop32 pass left to the search.  Waits for
// that solve on the context's stream; *count = the boards the pass listed (p32_list[0]; 0 when the
// last solve did not run the pass), and the first min(*count, cap) of them come back in list order
// (not deterministic: workgroups reserve list slots with an atomic add) -- index[i] the board's
// index in the batch, grids[81 i ..] what the search was given for it (p32_in: the propagated grid
// under handover, else the input; the fallback only reads that buffer -- launch_solve takes it as
// its const input and dn_collect copies from it into dn_tail[0].in).
extern "C" int sdk_debug_p32_list(sdk_ctx* c, uint32_t* index, uint8_t* grids, int64_t cap, int64_t* count) {
    if (!c || !count || cap < 0 || (cap > 0 && (!index || !grids))) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *count = 0;
    if (!c->prop32_ran || !c->p32_list.p || !c->p32_in.p) return SDK_OK;
    HIPCALL(hipSetDevice(c->device));
    uint32_t v = 0;
    HIPCALL(hipMemcpyAsync(&v, c->p32_list.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    *count = v;
    const size_t k = (size_t)std::min<int64_t>((int64_t)v, cap);
    if (k == 0) return SDK_OK;
    HIPCALL(hipMemcpyAsync(index, static_cast<const uint32_t*>(c->p32_list.p) + 1, k * 4, hipMemcpyDeviceToHost,
                           c->stream));
    HIPCALL(hipMemcpyAsync(grids, c->p32_in.p, k * 81, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    return SDK_OK;
}

namespace {
// a phased solve's board counts (dn_stat) wait for it on the context's stream
int read_dn_stat(sdk_ctx* c, int k, int64_t* value) {
    *value = 0;
    if (!c->dn_ran || !c->dn_stat.p) return SDK_OK;
    HIPCALL(hipSetDevice(c->device));
    uint32_t v = 0;
    HIPCALL(hipMemcpyAsync(&v, static_cast<uint32_t*>(c->dn_stat.p) + k, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    *value = v;
    return SDK_OK;
}

// The sticky error words of the two donation areas (a bounded wait on another wave inside a
// donation launch ran out, solve4_kernel.h kDnWaitTicks): read once after a phased solve,
// cleared, and turned into SDK_EHIP -- the solve's boards are then not valid.
int dn_check_error(sdk_ctx* c) {
    if (!c->dn_err_check || !c->dn.p) return SDK_OK;
    c->dn_err_check = false;
    uint32_t e[2] = {0u, 0u};
    for (int k = 0; k < 2; ++k)
        HIPCALL(hipMemcpyAsync(&e[k], static_cast<char*>(c->dn.p) + (size_t)k * sdk::kDnBytes + offsetof(sdk::DnCtl, err),
                               sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    const uint32_t err = e[0] | e[1];
    if (err == 0u) return SDK_OK;
    for (int k = 0; k < 2; ++k)
        HIPCALL(hipMemsetAsync(static_cast<char*>(c->dn.p) + (size_t)k * sdk::kDnBytes + offsetof(sdk::DnCtl, err), 0,
                               sizeof(uint32_t), c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    if (err & sdk::kDnErrSeed)
        return fail(SDK_EHIP, "donation launch: a resumed board's items disagree with their reservation; the "
                    "solve's boards are not valid");
    return fail(SDK_EHIP, "donation launch: a bounded wait on another wave ran out (%s%s); the solve's boards are "
                "not valid", (err & sdk::kDnErrReg) ? "registration entry never written " : "",
                (err & sdk::kDnErrLock) ? "record lock never released" : "");
}

// The plain options: sdk_set_option stores a value in [lo, hi] in the context's field (else `msg`, which
// may print the value with %lld), sdk_get_option reads it back.  (The helper functions below are static:
// inside extern "C" the unnamed namespace alone does not keep their names out of the dynamic symbols.)
struct OptionRow {
    int key;
    int64_t sdk_ctx::*field;
    int64_t lo, hi;
    const char* msg;
};
constexpr int64_t kAny = INT64_MAX;
const OptionRow kOptions[] = {
    {SDK_OPT_ORDER, &sdk_ctx::order, SDK_ORDER_MRV_UNIQUE, SDK_ORDER_LEX, "bad order %lld"},
    {SDK_OPT_NODE_BUDGET, &sdk_ctx::budget, 0, kAny, "budget must be >= 0"},
    {SDK_OPT_WAVES_PER_CU, &sdk_ctx::waves_per_cu, 1, 32, "waves per CU must be 1..32"},
    {SDK_OPT_CHECK_BLOCKS_PER_CU, &sdk_ctx::check_blocks_per_cu, 1, 16, "check blocks per CU must be 1..16"},
    {SDK_OPT_WORK_COUNTER, &sdk_ctx::work_rounds, SDK_WORK_NODES, SDK_WORK_DEPTH, "bad work counter %lld"},
    {SDK_OPT_SOLVER, &sdk_ctx::solver, SDK_SOLVER_WAVE, SDK_SOLVER_LANE, "bad solver %lld"},
    {SDK_OPT_WAVES_PER_CU2, &sdk_ctx::waves_per_cu2, 1, 32, "waves per CU must be 1..32"},
    {SDK_OPT_CHECK_VARIANT, &sdk_ctx::check_variant, SDK_CHECK_REG1, SDK_CHECK_WAVE2, "bad check variant %lld"},
    {SDK_OPT_SOLVE_CHUNK, &sdk_ctx::solve_chunk, 0, 4096, "solve chunk must be 0..4096"},
    {SDK_OPT_TIMING, &sdk_ctx::timing, 0, 1, "timing must be 0 or 1"},
    {SDK_OPT_LOCKED, &sdk_ctx::locked, 0, 2, "locked must be 0, 1 or 2"},
    {SDK_OPT_XCD_HEADS, &sdk_ctx::xcd_heads, 0, 1, "xcd heads must be 0 or 1"},
    {SDK_OPT_DONATE, &sdk_ctx::donate, 0, 1 << 30, "donate must be 0, 1 or a split budget >= 2"},
    {SDK_OPT_DONATE_MODE, &sdk_ctx::dn_exhaustive, 0, 1, "donate mode must be 0 (LEX) or 1 (exhaustive)"},
    {SDK_OPT_DONATE_MAX, &sdk_ctx::dn_max, 0, kAny, "SDK_OPT_DONATE_MAX must be >= 0"},
    {SDK_OPT_DN_FAULT, &sdk_ctx::dn_fault, 0, 1, "SDK_OPT_DN_FAULT must be 0 or 1"},
    {SDK_OPT_DONATE_HELPERS, &sdk_ctx::dn_helpers, 1, 4096, "SDK_OPT_DONATE_HELPERS must be 1..4096"},
    {SDK_OPT_DONATE_RESUME, &sdk_ctx::dn_resume, 0, 1, "SDK_OPT_DONATE_RESUME must be 0 or 1"},
    {SDK_OPT_PROP32, &sdk_ctx::prop32, 0, 1, "SDK_OPT_PROP32 is 0 or 1"},
    {SDK_OPT_PROP32_MIN, &sdk_ctx::prop32_min, 1, kAny, "SDK_OPT_PROP32_MIN must be >= 1"},
    {SDK_OPT_PROP32_HANDOVER, &sdk_ctx::prop32_handover, 0, 1, "SDK_OPT_PROP32_HANDOVER is 0 or 1"},
    {SDK_OPT_GEN_CAP, &sdk_ctx::gen_cap, 81, 0x7FFFFFFFll, "SDK_OPT_GEN_CAP must be 81..2^31-1"},
};
static const OptionRow* option_row(int key) {
    for (const OptionRow& r : kOptions)
        if (r.key == key) return &r;
    return nullptr;
}

// The packed options: several small fields in one value.
static bool packed_option(int key) { return key == SDK_OPT_PROP32_LC || key == SDK_OPT_PROP32_TAIL; }
static int set_packed_option(sdk_ctx* c, int key, int64_t value) {
    if (key == SDK_OPT_PROP32_LC) {
        if (value < 0 || (value & 0xFF) < 1 || (value & 0xFF) > 64 || (value >> 8) > 64)
            return fail(SDK_EINVAL, "SDK_OPT_PROP32_LC: period 1..64 | first step 0..64 << 8");
        c->prop32_lc = value;
    } else {   // SDK_OPT_PROP32_TAIL
        if (value < 0 || (value & 0xFF) > 64 || (value >> 8) > 96) return fail(SDK_EINVAL, "SDK_OPT_PROP32_TAIL out of range");
        c->prop32_tail_live = value & 0xFF;
        c->prop32_tail_step = value >> 8;
    }
    return SDK_OK;
}
static int64_t get_packed_option(const sdk_ctx* c, int key) {
    return key == SDK_OPT_PROP32_LC ? c->prop32_lc : (c->prop32_tail_live | (c->prop32_tail_step << 8));
}

// The read-only options: their names (nullptr: not one of them) and their values, most of them read
// from device memory after waiting for the last solve on the context's stream.
static const char* read_only_option(int key) {
    switch (key) {
        case SDK_OPT_DEVICE_CUS: return "SDK_OPT_DEVICE_CUS";
        case SDK_OPT_TIMER_EVENTS: return "SDK_OPT_TIMER_EVENTS";
        case SDK_OPT_DONATED: return "SDK_OPT_DONATED";
        case SDK_OPT_SPLIT_BOARDS: return "SDK_OPT_SPLIT_BOARDS";
        case SDK_OPT_LEX_BOARDS: return "SDK_OPT_LEX_BOARDS";
        case SDK_OPT_RESUMED: return "SDK_OPT_RESUMED";
        case SDK_OPT_PROP32_UNDECIDED: return "SDK_OPT_PROP32_UNDECIDED";
        default: return nullptr;
    }
}
static int get_read_only_option(sdk_ctx* c, int key, int64_t* value) {
    *value = 0;
    switch (key) {
        case SDK_OPT_DEVICE_CUS: *value = c->cus; return SDK_OK;
        case SDK_OPT_TIMER_EVENTS: *value = (int64_t)c->events.size(); return SDK_OK;
        case SDK_OPT_SPLIT_BOARDS: return read_dn_stat(c, 0, value);
        case SDK_OPT_LEX_BOARDS: return read_dn_stat(c, 1, value);
        case SDK_OPT_PROP32_UNDECIDED: {
            if (!c->prop32_ran) return SDK_OK;
            HIPCALL(hipSetDevice(c->device));
            uint32_t v = 0;
            HIPCALL(hipMemcpyAsync(&v, c->p32_list.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
            HIPCALL(hipStreamSynchronize(c->stream));
            *value = v;
            return SDK_OK;
        }
        case SDK_OPT_DONATED: {
            // items handed out by the last phased solve's donation launches (of its last
            // kDnCapBoards-board pass; waits for it on the context's stream)
            if (!c->dn.p || c->dn_epoch == 0 || !c->dn_ran) return SDK_OK;
            HIPCALL(hipSetDevice(c->device));
            sdk::DnCtl h[2];
            for (int k = 0; k < 2; ++k)
                HIPCALL(hipMemcpyAsync(&h[k], static_cast<char*>(c->dn.p) + (size_t)k * sdk::kDnBytes, sizeof h[k],
                                       hipMemcpyDeviceToHost, c->stream));
            HIPCALL(hipStreamSynchronize(c->stream));
            *value = (int64_t)h[0].delivered + (int64_t)h[1].delivered;
            return SDK_OK;
        }
        default: {   // SDK_OPT_RESUMED
            // boards the last phased solve resumed (donation area 0; waits for the solve)
            if (!c->dn.p || c->dn_epoch == 0 || !c->dn_ran) return SDK_OK;
            HIPCALL(hipSetDevice(c->device));
            sdk::DnSeed h;
            HIPCALL(hipMemcpyAsync(&h, static_cast<char*>(c->dn.p) + offsetof(sdk::DnCtl, seed), sizeof h,
                                   hipMemcpyDeviceToHost, c->stream));
            HIPCALL(hipStreamSynchronize(c->stream));
            *value = (int64_t)h.boards;
            return SDK_OK;
        }
    }
}
}  // namespace

int sdk_set_option(sdk_ctx* c, int key, int64_t value) {
    if (!c) return fail(SDK_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (const OptionRow* r = option_row(key)) {
        if (value < r->lo || value > r->hi) return fail(SDK_EINVAL, r->msg, (long long)value);
        c->*(r->field) = value;
        return SDK_OK;
    }
    if (packed_option(key)) return set_packed_option(c, key, value);
    if (const char* name = read_only_option(key)) return fail(SDK_EINVAL, "%s is read-only", name);
    return fail(SDK_EINVAL, "unknown option %d", key);
}

int sdk_get_option(sdk_ctx* c, int key, int64_t* value) {
    if (!c || !value) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (const OptionRow* r = option_row(key)) {
        *value = c->*(r->field);
        return SDK_OK;
    }
    if (packed_option(key)) {
        *value = get_packed_option(c, key);
        return SDK_OK;
    }
    if (read_only_option(key)) return get_read_only_option(c, key, value);
    return fail(SDK_EINVAL, "unknown option %d", key);
}

int sdk_dev_alloc(sdk_ctx* c, size_t bytes, void** dptr) {
    if (!c || !dptr) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipMalloc(dptr, std::max(bytes, (size_t)16)));
    return SDK_OK;
}

int sdk_dev_free(sdk_ctx* c, void* dptr) {
    if (!c) return fail(SDK_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipStreamSynchronize(c->stream));
    if (dptr) HIPCALL(hipFree(dptr));
    return SDK_OK;
}

int sdk_memcpy_h2d(sdk_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (!dst && bytes) || (!src && bytes)) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    return SDK_OK;
}

int sdk_memcpy_d2h(sdk_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (!dst && bytes) || (!src && bytes)) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    return dn_check_error(c);
}

int sdk_synchronize(sdk_ctx* c) {
    if (!c) return fail(SDK_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipStreamSynchronize(c->stream));
    return dn_check_error(c);
}

int sdk_timer_reset(sdk_ctx* c) {
    if (!c) return fail(SDK_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipStreamSynchronize(c->stream));
    c->events_used = 0;
    return SDK_OK;
}

int sdk_timer_read(sdk_ctx* c, double* total_ms, int64_t* launches) {
    if (!c || !total_ms || !launches) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    double tot = 0;
    for (size_t i = 0; i < c->events_used; ++i) {
        float ms = 0.f;
        HIPCALL(hipEventElapsedTime(&ms, c->events[i].first, c->events[i].second));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int64_t)c->events_used;
    return SDK_OK;
}

// diagnostics (not in the header): durations of the timed launches since sdk_timer_reset
extern "C" int sdk_debug_timer_list(sdk_ctx* c, double* ms, int64_t cap, int64_t* n) {
    if (!c || !ms || !n) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    *n = (int64_t)c->events_used;
    for (size_t i = 0; i < c->events_used && (int64_t)i < cap; ++i) {
        float v = 0.f;
        HIPCALL(hipEventElapsedTime(&v, c->events[i].first, c->events[i].second));
        ms[i] = v;
    }
    return SDK_OK;
}

int sdk_check_batch_dev(sdk_ctx* c, const void* d_boards, void* d_verdict, size_t n) {
    if (!c || (n && (!d_boards || !d_verdict))) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_check(c, static_cast<const uint8_t*>(d_boards), static_cast<uint8_t*>(d_verdict), n);
}

int sdk_solve_batch_dev(sdk_ctx* c, const void* d_in, const void* d_mask, void* d_out, void* d_status,
                        void* d_work, size_t n) {
    if (!c || (n && (!d_in || !d_out || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_solve(c, SolveCall{static_cast<const uint8_t*>(d_in), static_cast<const uint16_t*>(d_mask),
                                     static_cast<uint8_t*>(d_out), static_cast<int8_t*>(d_status),
                                     static_cast<uint64_t*>(d_work), n});
}

int sdk_check_batch(sdk_ctx* c, const uint8_t* boards, uint8_t* verdict, size_t n) {
    if (!c || (n && (!boards || !verdict))) return fail(SDK_EINVAL, "NULL argument");
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->verdict, n))) return rc;
    HIPCALL(hipMemcpyAsync(c->in.p, boards, n * 81, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_check(c, static_cast<uint8_t*>(c->in.p), static_cast<uint8_t*>(c->verdict.p), n))) return rc;
    HIPCALL(hipMemcpyAsync(verdict, c->verdict.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    return SDK_OK;
}

int sdk_check_batch_i64(sdk_ctx* c, const int64_t* boards, uint8_t* verdict, size_t n) {
    if (!c || (n && (!boards || !verdict))) return fail(SDK_EINVAL, "NULL argument");
    if (n == 0) return SDK_OK;
    for (size_t k = 0; k < n * 81; ++k)
        if (boards[k] >= (1ll << 59) || boards[k] <= -(1ll << 59))
            return fail(SDK_EINVAL, "cell value %lld out of the checker's range (|v| < 2^59)", (long long)boards[k]);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c->in, n * 81 * sizeof(int64_t))) || (rc = ensure(c->verdict, n))) return rc;
    HIPCALL(hipMemcpyAsync(c->in.p, boards, n * 81 * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    hipEvent_t stop;
    if ((rc = timer_begin(c, &stop))) return rc;
    HIPCALL(sdk::launch_check_i64(static_cast<const int64_t*>(c->in.p), static_cast<uint8_t*>(c->verdict.p), (uint64_t)n,
                                  grid_for(c, n, sdk::kCheckI64Threads, 8), c->stream));
    if ((rc = timer_end(c, stop))) return rc;
    HIPCALL(hipMemcpyAsync(verdict, c->verdict.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    return SDK_OK;
}

int sdk_solve_batch(sdk_ctx* c, const uint8_t* in, const uint16_t* first_cell_mask, uint8_t* out, int8_t* status,
                    uint64_t* work, size_t n) {
    return sdk_solve_batch_budget(c, in, first_cell_mask, out, status, work, n, SDK_BUDGET_CONTEXT);
}

int sdk_solve_batch_budget(sdk_ctx* c, const uint8_t* in, const uint16_t* first_cell_mask, uint8_t* out,
                           int8_t* status, uint64_t* work, size_t n, uint64_t node_budget) {
    return sdk_solve_batch_ex(c, in, first_cell_mask, out, status, work, n, node_budget, SDK_DONATE_CONTEXT);
}

int sdk_solve_batch_ex(sdk_ctx* c, const uint8_t* in, const uint16_t* first_cell_mask, uint8_t* out, int8_t* status,
                       uint64_t* work, size_t n, uint64_t node_budget, int64_t donate) {
    if (!c || (n && (!in || !out || !status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_budget_arg(node_budget))) return rc;
    if (donate < SDK_DONATE_CONTEXT || donate > (1 << 30))
        return fail(SDK_EINVAL, "donate must be SDK_DONATE_CONTEXT, 0, 1 or a split budget >= 2");
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->out, n * 81)) || (rc = ensure(c->status, n))) return rc;
    if (first_cell_mask && (rc = ensure(c->mask, n * 2))) return rc;
    if (work && (rc = ensure(c->work, n * 8))) return rc;
    SolveCall s{static_cast<uint8_t*>(c->in.p), first_cell_mask ? static_cast<uint16_t*>(c->mask.p) : nullptr,
                static_cast<uint8_t*>(c->out.p), static_cast<int8_t*>(c->status.p),
                work ? static_cast<uint64_t*>(c->work.p) : nullptr, n};
    s.budget = budget_arg(node_budget);
    s.donate = donate;
    Staging io(c, {{n * 8, nullptr, nullptr, s.work, work},      // (a slot each, present or not)
                   {n * 2, first_cell_mask, c->mask.p},
                   {n * 81, in, c->in.p, s.out, out},
                   {n, nullptr, nullptr, s.status, status}});
    if ((rc = io.send()) || (rc = launch_solve(c, s)) || (rc = io.fetch())) return rc;
    return dn_check_error(c);
}

int sdk_classify_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_budget_arg(node_budget))) return rc;
    if (n == 0) return SDK_OK;
    if ((rc = check_board_count(n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_classify(c, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out),
                           static_cast<int8_t*>(d_status), n, budget_arg(node_budget));
}

int sdk_classify_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_budget_arg(node_budget))) return rc;
    if (n == 0) return SDK_OK;
    if ((rc = check_board_count(n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->out, n * 81)) || (rc = ensure(c->status, n))) return rc;
    uint8_t* d_in = static_cast<uint8_t*>(c->in.p);
    uint8_t* d_out = static_cast<uint8_t*>(c->out.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    Staging io(c, {{n * 81, in, d_in, d_out, out}, {n, nullptr, nullptr, d_status, status}});
    if ((rc = io.send()) || (rc = launch_classify(c, d_in, d_out, d_status, n, budget_arg(node_budget)))) return rc;
    return io.fetch();
}

int sdk_grade_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, void* d_level, void* d_open,
                        size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status || !d_level))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, false, d_in, d_out, d_status, {u8(d_level), u8(d_open), nullptr, nullptr, nullptr}, n,
                      node_budget);
}

int sdk_grade_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, uint8_t* level, uint8_t* open,
                    size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status || !level))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, true, in, out, status, {level, open, nullptr, nullptr, nullptr}, n, node_budget);
}

int sdk_rate_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, void* d_level, void* d_open,
                       void* d_backdoors, void* d_key, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status || !d_level || !d_backdoors))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, false, d_in, d_out, d_status, {u8(d_level), u8(d_open), u8(d_backdoors), u8(d_key), nullptr},
                      n, node_budget);
}

int sdk_rate_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, uint8_t* level, uint8_t* open,
                   uint8_t* backdoors, uint8_t* key, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status || !level || !backdoors))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, true, in, out, status, {level, open, backdoors, key, nullptr}, n, node_budget);
}

int sdk_subsets_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, void* d_level, void* d_open,
                          void* d_open4, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status || !d_level || !d_open4))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, false, d_in, d_out, d_status, {u8(d_level), u8(d_open), nullptr, nullptr, u8(d_open4)}, n,
                      node_budget);
}

int sdk_subsets_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, uint8_t* level, uint8_t* open,
                      uint8_t* open4, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status || !level || !open4))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, true, in, out, status, {level, open, nullptr, nullptr, open4}, n, node_budget);
}

int sdk_wings_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, void* d_level, void* d_open,
                        void* d_open4, void* d_open5, void* d_open6, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status || !d_level || !d_open6))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, false, d_in, d_out, d_status,
                      {u8(d_level), u8(d_open), nullptr, nullptr, u8(d_open4), u8(d_open5), u8(d_open6)}, n,
                      node_budget);
}

int sdk_wings_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, uint8_t* level, uint8_t* open,
                    uint8_t* open4, uint8_t* open5, uint8_t* open6, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status || !level || !open6))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, true, in, out, status, {level, open, nullptr, nullptr, open4, open5, open6}, n, node_budget);
}

int sdk_chains_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, void* d_level, void* d_open,
                         void* d_open4, void* d_open5, void* d_open6, void* d_open7, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status || !d_level || !d_open7))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, false, d_in, d_out, d_status,
                      {u8(d_level), u8(d_open), nullptr, nullptr, u8(d_open4), u8(d_open5), u8(d_open6), u8(d_open7)},
                      n, node_budget);
}

int sdk_chains_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, uint8_t* level, uint8_t* open,
                     uint8_t* open4, uint8_t* open5, uint8_t* open6, uint8_t* open7, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status || !level || !open7))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, true, in, out, status, {level, open, nullptr, nullptr, open4, open5, open6, open7}, n,
                      node_budget);
}

int sdk_fish_batch_dev(sdk_ctx* c, const void* d_in, void* d_out, void* d_status, void* d_level, void* d_open,
                       void* d_open4, void* d_open5, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_out || !d_status || !d_level || !d_open5))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, false, d_in, d_out, d_status,
                      {u8(d_level), u8(d_open), nullptr, nullptr, u8(d_open4), u8(d_open5)}, n, node_budget);
}

int sdk_fish_batch(sdk_ctx* c, const uint8_t* in, uint8_t* out, int8_t* status, uint8_t* level, uint8_t* open,
                   uint8_t* open4, uint8_t* open5, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !out || !status || !level || !open5))) return fail(SDK_EINVAL, "NULL argument");
    return grade_call(c, true, in, out, status, {level, open, nullptr, nullptr, open4, open5}, n, node_budget);
}

int sdk_canonical_batch_dev(sdk_ctx* c, const void* d_in, void* d_canon, void* d_solution, void* d_status,
                            void* d_gather, void* d_relabel, void* d_ties, size_t n, uint64_t node_budget) {
    if (!c || (n && (!d_in || !d_canon || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_budget_arg(node_budget))) return rc;
    if (n == 0) return SDK_OK;
    if ((rc = check_board_count(n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_canonical(c, static_cast<const uint8_t*>(d_in), u8(d_canon), static_cast<int8_t*>(d_status),
                            {u8(d_solution), u8(d_gather), u8(d_relabel), static_cast<uint16_t*>(d_ties)}, n,
                            budget_arg(node_budget));
}

int sdk_canonical_batch(sdk_ctx* c, const uint8_t* in, uint8_t* canon, uint8_t* solution, int8_t* status,
                        uint8_t* gather, uint8_t* relabel, uint16_t* ties, size_t n, uint64_t node_budget) {
    if (!c || (n && (!in || !canon || !status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_budget_arg(node_budget))) return rc;
    if (n == 0) return SDK_OK;
    if ((rc = check_board_count(n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    // the boards are canonised in place in c->in; the completions always go through c->out
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->out, n * 81)) || (rc = ensure(c->status, n)) ||
        (gather && (rc = ensure(c->cn_gather, n * 81))) || (relabel && (rc = ensure(c->cn_relabel, n * 10))) ||
        (ties && (rc = ensure(c->cn_ties, n * 2))))
        return rc;
    uint8_t* d_in = u8(c->in.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    const CanonCols d{u8(c->out.p), gather ? u8(c->cn_gather.p) : nullptr, relabel ? u8(c->cn_relabel.p) : nullptr,
                      ties ? static_cast<uint16_t*>(c->cn_ties.p) : nullptr};
    // a nullable output comes back iff the caller has it (a slot each, present or not)
    auto back = [](size_t bytes, const void* dev, void* dst) { return Piece{dst ? bytes : 0, nullptr, nullptr, dev, dst}; };
    Staging io(c, {back(n * 2, d.ties, ties),
                   {n * 81, in, d_in, d_in, canon},
                   back(n * 81, d.solution, solution),
                   back(n * 81, d.gather, gather),
                   back(n * 10, d.relabel, relabel),
                   {n, nullptr, nullptr, d_status, status}});
    if ((rc = io.send()) || (rc = launch_canonical(c, d_in, d_in, d_status, d, n, budget_arg(node_budget)))) return rc;
    return io.fetch();
}

int sdk_minimize_batch_dev(sdk_ctx* c, const void* d_in, const void* d_order, void* d_out, void* d_status, size_t n) {
    if (!c || (n && (!d_in || !d_order || !d_out || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    if (n == 0) return SDK_OK;
    int rc;
    if ((rc = check_board_count(n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_minimize(c, static_cast<const uint8_t*>(d_in), static_cast<const uint8_t*>(d_order),
                           static_cast<uint8_t*>(d_out), static_cast<int8_t*>(d_status), n);
}

int sdk_minimize_batch(sdk_ctx* c, const uint8_t* in, const uint8_t* order, uint8_t* out, int8_t* status, size_t n) {
    if (!c || (n && (!in || !order || !out || !status))) return fail(SDK_EINVAL, "NULL argument");
    if (n == 0) return SDK_OK;
    int rc;
    if ((rc = check_board_count(n))) return rc;
    if ((rc = check_order_rows(order, n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->mz_order, n * 81)) || (rc = ensure(c->out, n * 81)) ||
        (rc = ensure(c->status, n)))
        return rc;
    uint8_t* d_in = static_cast<uint8_t*>(c->in.p);
    uint8_t* d_order = static_cast<uint8_t*>(c->mz_order.p);
    uint8_t* d_out = static_cast<uint8_t*>(c->out.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    Staging io(c, {{n * 81, order, d_order}, {n * 81, in, d_in, d_out, out}, {n, nullptr, nullptr, d_status, status}});
    if ((rc = io.send()) || (rc = launch_minimize(c, d_in, d_order, d_out, d_status, n))) return rc;
    return io.fetch();
}

int sdk_generate_grids_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, void* d_grids, void* d_order,
                           void* d_placements) {
    if (!c || (n && !d_grids)) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_generate_args(first, n))) return rc;
    if (n == 0) return SDK_OK;
    if ((reinterpret_cast<uintptr_t>(d_grids) | reinterpret_cast<uintptr_t>(d_order)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_placements) & 3u) return fail(SDK_EINVAL, "d_placements must be 4-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_generate(c, seed, first, n, static_cast<uint8_t*>(d_grids), static_cast<uint8_t*>(d_order),
                           static_cast<uint32_t*>(d_placements));
}

int sdk_generate_grids(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint8_t* grids, uint8_t* order,
                       uint32_t* placements) {
    if (!c || (n && !grids)) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_generate_args(first, n))) return rc;
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->out, n * 81)) || (order && (rc = ensure(c->mz_order, n * 81))) ||
        (placements && (rc = ensure(c->gen_plc, n * 4))))
        return rc;
    uint8_t* d_grids = static_cast<uint8_t*>(c->out.p);
    uint8_t* d_order = order ? static_cast<uint8_t*>(c->mz_order.p) : nullptr;
    uint32_t* d_plc = placements ? static_cast<uint32_t*>(c->gen_plc.p) : nullptr;
    Staging io(c, {{placements ? n * 4 : 0, nullptr, nullptr, d_plc, placements},
                   {n * 81, nullptr, nullptr, d_grids, grids},
                   {order ? n * 81 : 0, nullptr, nullptr, d_order, order}});
    if ((rc = launch_generate(c, seed, first, n, d_grids, d_order, d_plc))) return rc;
    return io.fetch();
}

int sdk_generate_puzzles_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, void* d_puzzles, void* d_grids,
                             void* d_status) {
    if (!c || (n && (!d_puzzles || !d_grids || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_generate_args(first, n))) return rc;
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_generate_puzzles(c, seed, first, n, static_cast<uint8_t*>(d_puzzles), static_cast<uint8_t*>(d_grids),
                                   static_cast<int8_t*>(d_status));
}

int sdk_generate_puzzles(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint8_t* puzzles, uint8_t* grids,
                         int8_t* status) {
    if (!c || (n && (!puzzles || !grids || !status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_generate_args(first, n))) return rc;
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->out, n * 81)) || (rc = ensure(c->status, n))) return rc;
    uint8_t* d_grids = static_cast<uint8_t*>(c->in.p);
    uint8_t* d_puzzles = static_cast<uint8_t*>(c->out.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    Staging io(c, {{n * 81, nullptr, nullptr, d_puzzles, puzzles},
                   {n * 81, nullptr, nullptr, d_grids, grids},
                   {n, nullptr, nullptr, d_status, status}});
    if ((rc = launch_generate_puzzles(c, seed, first, n, d_puzzles, d_grids, d_status))) return rc;
    return io.fetch();
}

int sdk_minimize_level_batch_dev(sdk_ctx* c, const void* d_in, const void* d_order, int level, void* d_out,
                                 void* d_status, size_t n) {
    if (!c || (n && (!d_in || !d_order || !d_out || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_level_arg(level)) || (rc = check_board_count(n))) return rc;
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_reduce_level(c, static_cast<const uint8_t*>(d_in), static_cast<const uint8_t*>(d_order), level,
                               static_cast<uint8_t*>(d_out), static_cast<int8_t*>(d_status), n);
}

int sdk_minimize_level_batch(sdk_ctx* c, const uint8_t* in, const uint8_t* order, int level, uint8_t* out,
                             int8_t* status, size_t n) {
    if (!c || (n && (!in || !order || !out || !status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_level_arg(level)) || (rc = check_board_count(n))) return rc;
    if (n == 0) return SDK_OK;
    if ((rc = check_order_rows(order, n))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->mz_order, n * 81)) || (rc = ensure(c->out, n * 81)) ||
        (rc = ensure(c->status, n)))
        return rc;
    uint8_t* d_in = static_cast<uint8_t*>(c->in.p);
    uint8_t* d_order = static_cast<uint8_t*>(c->mz_order.p);
    uint8_t* d_out = static_cast<uint8_t*>(c->out.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    Staging io(c, {{n * 81, order, d_order}, {n * 81, in, d_in, d_out, out}, {n, nullptr, nullptr, d_status, status}});
    if ((rc = io.send()) || (rc = launch_reduce_level(c, d_in, d_order, level, d_out, d_status, n))) return rc;
    return io.fetch();
}

int sdk_generate_level_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, int level, void* d_puzzles,
                           void* d_grids, void* d_status) {
    if (!c || (n && (!d_puzzles || !d_grids || !d_status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_level_arg(level)) || (rc = check_generate_args(first, n))) return rc;
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return launch_generate_level(c, seed, first, n, level, static_cast<uint8_t*>(d_puzzles),
                                 static_cast<uint8_t*>(d_grids), static_cast<int8_t*>(d_status));
}

int sdk_generate_level(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, int level, uint8_t* puzzles,
                       uint8_t* grids, int8_t* status) {
    if (!c || (n && (!puzzles || !grids || !status))) return fail(SDK_EINVAL, "NULL argument");
    int rc;
    if ((rc = check_level_arg(level)) || (rc = check_generate_args(first, n))) return rc;
    if (n == 0) return SDK_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    if ((rc = ensure(c->in, n * 81)) || (rc = ensure(c->out, n * 81)) || (rc = ensure(c->status, n))) return rc;
    uint8_t* d_grids = static_cast<uint8_t*>(c->in.p);
    uint8_t* d_puzzles = static_cast<uint8_t*>(c->out.p);
    int8_t* d_status = static_cast<int8_t*>(c->status.p);
    Staging io(c, {{n * 81, nullptr, nullptr, d_puzzles, puzzles},
                   {n * 81, nullptr, nullptr, d_grids, grids},
                   {n, nullptr, nullptr, d_status, status}});
    if ((rc = launch_generate_level(c, seed, first, n, level, d_puzzles, d_grids, d_status))) return rc;
    return io.fetch();
}

int sdk_generate_graded_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask,
                            uint32_t clues_lo, uint32_t clues_hi, uint64_t max_scan, uint64_t chunk, void* d_puzzles,
                            void* d_grids, void* d_level, void* d_open, void* d_index, uint64_t* found,
                            uint64_t* scanned) {
    return graded_call(c, false, n,
                       graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, d_puzzles, d_grids,
                                   d_level, d_open, d_index),
                       found, scanned);
}

int sdk_generate_graded(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                        uint32_t clues_hi, uint64_t max_scan, uint64_t chunk, uint8_t* puzzles, uint8_t* grids,
                        uint8_t* level, uint8_t* open, uint64_t* index, uint64_t* found, uint64_t* scanned) {
    return graded_call(c, true, n,
                       graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, puzzles, grids, level,
                                   open, index),
                       found, scanned);
}

int sdk_generate_rated_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask,
                           uint32_t clues_lo, uint32_t clues_hi, uint32_t backdoors_lo, uint32_t backdoors_hi,
                           uint64_t max_scan, uint64_t chunk, void* d_puzzles, void* d_grids, void* d_level,
                           void* d_open, void* d_backdoors, void* d_key, void* d_index, uint64_t* found,
                           uint64_t* scanned) {
    return graded_call(c, false, n,
                       rated_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, d_puzzles,
                                              d_grids, d_level, d_open, d_index),
                                  backdoors_lo, backdoors_hi, d_backdoors, d_key),
                       found, scanned);
}

int sdk_generate_rated(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                       uint32_t clues_hi, uint32_t backdoors_lo, uint32_t backdoors_hi, uint64_t max_scan,
                       uint64_t chunk, uint8_t* puzzles, uint8_t* grids, uint8_t* level, uint8_t* open,
                       uint8_t* backdoors, uint8_t* key, uint64_t* index, uint64_t* found, uint64_t* scanned) {
    return graded_call(c, true, n,
                       rated_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, puzzles,
                                              grids, level, open, index),
                                  backdoors_lo, backdoors_hi, backdoors, key),
                       found, scanned);
}

int sdk_generate_subsets_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask,
                             uint32_t clues_lo, uint32_t clues_hi, uint32_t open4_lo, uint32_t open4_hi,
                             uint64_t max_scan, uint64_t chunk, void* d_puzzles, void* d_grids, void* d_level,
                             void* d_open, void* d_open4, void* d_index, uint64_t* found, uint64_t* scanned) {
    return graded_call(c, false, n,
                       subsets_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk,
                                                d_puzzles, d_grids, d_level, d_open, d_index),
                                    open4_lo, open4_hi, d_open4),
                       found, scanned);
}

int sdk_generate_subsets(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                         uint32_t clues_hi, uint32_t open4_lo, uint32_t open4_hi, uint64_t max_scan, uint64_t chunk,
                         uint8_t* puzzles, uint8_t* grids, uint8_t* level, uint8_t* open, uint8_t* open4,
                         uint64_t* index, uint64_t* found, uint64_t* scanned) {
    return graded_call(c, true, n,
                       subsets_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, puzzles,
                                                grids, level, open, index),
                                    open4_lo, open4_hi, open4),
                       found, scanned);
}

int sdk_generate_wings_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                           uint32_t clues_hi, uint32_t open5_lo, uint32_t open5_hi, uint32_t open6_lo,
                           uint32_t open6_hi, uint64_t max_scan, uint64_t chunk, void* d_puzzles, void* d_grids,
                           void* d_level, void* d_open, void* d_open5, void* d_open6, void* d_index, uint64_t* found,
                           uint64_t* scanned) {
    return graded_call(c, false, n,
                       wings_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, d_puzzles,
                                              d_grids, d_level, d_open, d_index),
                                  open5_lo, open5_hi, open6_lo, open6_hi, d_open5, d_open6),
                       found, scanned);
}

int sdk_generate_wings(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                       uint32_t clues_hi, uint32_t open5_lo, uint32_t open5_hi, uint32_t open6_lo, uint32_t open6_hi,
                       uint64_t max_scan, uint64_t chunk, uint8_t* puzzles, uint8_t* grids, uint8_t* level,
                       uint8_t* open, uint8_t* open5, uint8_t* open6, uint64_t* index, uint64_t* found,
                       uint64_t* scanned) {
    return graded_call(c, true, n,
                       wings_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, puzzles,
                                              grids, level, open, index),
                                  open5_lo, open5_hi, open6_lo, open6_hi, open5, open6),
                       found, scanned);
}

int sdk_generate_chains_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                            uint32_t clues_hi, uint32_t open6_lo, uint32_t open6_hi, uint32_t open7_lo,
                            uint32_t open7_hi, uint64_t max_scan, uint64_t chunk, void* d_puzzles, void* d_grids,
                            void* d_level, void* d_open, void* d_open6, void* d_open7, void* d_index, uint64_t* found,
                            uint64_t* scanned) {
    return graded_call(c, false, n,
                       chains_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, d_puzzles,
                                               d_grids, d_level, d_open, d_index),
                                   open6_lo, open6_hi, open7_lo, open7_hi, d_open6, d_open7),
                       found, scanned);
}

int sdk_generate_chains(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                        uint32_t clues_hi, uint32_t open6_lo, uint32_t open6_hi, uint32_t open7_lo, uint32_t open7_hi,
                        uint64_t max_scan, uint64_t chunk, uint8_t* puzzles, uint8_t* grids, uint8_t* level,
                        uint8_t* open, uint8_t* open6, uint8_t* open7, uint64_t* index, uint64_t* found,
                        uint64_t* scanned) {
    return graded_call(c, true, n,
                       chains_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, puzzles,
                                               grids, level, open, index),
                                   open6_lo, open6_hi, open7_lo, open7_hi, open6, open7),
                       found, scanned);
}

int sdk_generate_fish_dev(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                          uint32_t clues_hi, uint32_t open4_lo, uint32_t open4_hi, uint32_t open5_lo,
                          uint32_t open5_hi, uint64_t max_scan, uint64_t chunk, void* d_puzzles, void* d_grids,
                          void* d_level, void* d_open, void* d_open4, void* d_open5, void* d_index, uint64_t* found,
                          uint64_t* scanned) {
    return graded_call(c, false, n,
                       fish_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, d_puzzles,
                                             d_grids, d_level, d_open, d_index),
                                 open4_lo, open4_hi, open5_lo, open5_hi, d_open4, d_open5),
                       found, scanned);
}

int sdk_generate_fish(sdk_ctx* c, uint64_t seed, uint64_t first, size_t n, uint32_t level_mask, uint32_t clues_lo,
                      uint32_t clues_hi, uint32_t open4_lo, uint32_t open4_hi, uint32_t open5_lo, uint32_t open5_hi,
                      uint64_t max_scan, uint64_t chunk, uint8_t* puzzles, uint8_t* grids, uint8_t* level,
                      uint8_t* open, uint8_t* open4, uint8_t* open5, uint64_t* index, uint64_t* found,
                      uint64_t* scanned) {
    return graded_call(c, true, n,
                       fish_args(graded_args(seed, first, level_mask, clues_lo, clues_hi, max_scan, chunk, puzzles,
                                             grids, level, open, index),
                                 open4_lo, open4_hi, open5_lo, open5_hi, open4, open5),
                       found, scanned);
}

int sdk_select_rows_dev(sdk_ctx* c, const sdk_select_rows* a, uint64_t* total, uint64_t* last) {
    if (!c || !a || !total || !last) return fail(SDK_EINVAL, "NULL argument");
    if (!a->puzzles || !a->grids || !a->status || !a->level || !a->open || !a->out_puzzles || !a->out_grids)
        return fail(SDK_EINVAL, "NULL argument: the rows, status, level, open and both board outputs are required");
    if (a->m == 0 || a->m > kGradedChunkMax) return fail(SDK_EINVAL, "m must be 1..2^24");
    if (a->first > UINT64_MAX - a->m) return fail(SDK_EINVAL, "first + m overflows the stream index");
    int rc;
    if (a->n == 0) return fail(SDK_EINVAL, "n must be at least 1");
    if (a->n > 0x7FFFFFFFull) return fail(SDK_EINVAL, "n must be at most 2^31-1 rows");
    if (a->base >= a->n) return fail(SDK_EINVAL, "base must be below n (a round starts only below the quota)");
    if ((rc = check_graded_args(a->first, (size_t)a->n, a->level_mask, a->clues_lo, a->clues_hi, a->m, 0)) ||
        (rc = check_rated_range(a->backdoors_lo, a->backdoors_hi)) ||
        (rc = check_subsets_range(a->open4_lo, a->open4_hi)))
        return rc;
    if ((reinterpret_cast<uintptr_t>(a->puzzles) | reinterpret_cast<uintptr_t>(a->grids)) & 15u)
        return fail(SDK_EINVAL, "the rows must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a->out_puzzles) | reinterpret_cast<uintptr_t>(a->out_grids)) & 15u)
        return fail(SDK_EINVAL, "device boards must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(a->out_index) & 7u) return fail(SDK_EINVAL, "out_index must be 8-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    const uint32_t tiles = (uint32_t)((a->m + sdk::kSelTileRows - 1) / sdk::kSelTileRows);
    if ((rc = ensure(c->gg_word, sizeof(sdk::SelWord))) || (rc = ensure(c->gg_ballot, (size_t)tiles * 8)) ||
        (rc = ensure(c->gg_count, (size_t)tiles * 4)) || (rc = ensure(c->gg_offset, (size_t)tiles * 4)))
        return rc;
    sdk::SelWord* d_word = static_cast<sdk::SelWord*>(c->gg_word.p);
    SelectRound r{};
    r.puzzles = static_cast<const uint8_t*>(a->puzzles);
    r.grids = static_cast<const uint8_t*>(a->grids);
    r.status = static_cast<const int8_t*>(a->status);
    r.level = static_cast<const uint8_t*>(a->level);
    r.open = static_cast<const uint8_t*>(a->open);
    r.backdoors = static_cast<const uint8_t*>(a->backdoors);
    r.key = static_cast<const uint8_t*>(a->key);
    r.open4 = static_cast<const uint8_t*>(a->open4);
    r.m = (uint32_t)a->m;
    r.first = a->first;
    r.n = (uint32_t)a->n;
    r.level_mask = a->level_mask;
    r.clues_lo = a->clues_lo;
    r.clues_hi = a->clues_hi;
    r.bd_lo = a->backdoors_lo;
    r.bd_hi = a->backdoors_hi;
    r.o4_lo = a->open4_lo;
    r.o4_hi = a->open4_hi;
    r.out_puzzles = static_cast<uint8_t*>(a->out_puzzles);
    r.out_grids = static_cast<uint8_t*>(a->out_grids);
    r.out_level = static_cast<uint8_t*>(a->out_level);
    r.out_open = static_cast<uint8_t*>(a->out_open);
    r.out_index = static_cast<uint64_t*>(a->out_index);
    r.out_backdoors = static_cast<uint8_t*>(a->out_backdoors);
    r.out_key = static_cast<uint8_t*>(a->out_key);
    r.out_open4 = static_cast<uint8_t*>(a->out_open4);
    TimedSpan span(c);
    if ((rc = span.begin())) return rc;
    // the word: {base, 0}
    HIPCALL(hipMemsetAsync(d_word, 0, sizeof(sdk::SelWord), c->stream));
    if (a->base) HIPCALL(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&d_word->total), (int)(uint32_t)a->base, 1, c->stream));
    if ((rc = launch_select_round(c, r, d_word))) return rc;
    sdk::SelWord word;
    HIPCALL(hipMemcpyAsync(&word, d_word, sizeof word, hipMemcpyDeviceToHost, c->stream));
    HIPCALL(hipStreamSynchronize(c->stream));
    if (word.total >= r.n && (word.last == 0 || word.last > r.m))
        return fail(SDK_EHIP, "selection lost the position of its last hit");
    *total = word.total;
    *last = word.last;
    return span.end(SDK_OK);
}

int sdk_count_solutions(sdk_ctx* c, const uint8_t* board, uint64_t limit, uint64_t* count, int8_t* status) {
    if (!c || !board || !count || !status) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return count_slice(c, board, limit, 0, 1, count, nullptr, status);
}

int sdk_count_solutions_slice(sdk_ctx* c, const uint8_t* board, uint64_t limit, int rank, int world,
                              uint64_t* count, uint64_t* frontier_size, int8_t* status) {
    if (!c || !board || !count || !status) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return count_slice(c, board, limit, rank, world, count, frontier_size, status);
}

int sdk_frontier_build(sdk_ctx* c, const uint8_t* board, const uint16_t* first_cell_mask, int mode, uint64_t target,
                       uint64_t* size, uint64_t* leaves) {
    if (!c || !board) return fail(SDK_EINVAL, "NULL argument");
    if (mode != SDK_FRONTIER_COUNT && mode != SDK_FRONTIER_FIRST) return fail(SDK_EINVAL, "bad frontier mode %d", mode);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    int rc = build_frontier(c, board, first_cell_mask, mode, target);
    if (rc) return rc;
    if (size) *size = c->fr_size;
    if (leaves) *leaves = c->fr_leaves;
    return SDK_OK;
}

int sdk_expand_boards(sdk_ctx* c, const uint8_t* boards, const uint16_t* first_cell_masks, size_t n,
                      uint64_t target, uint8_t* out, size_t cap, uint64_t* out_n) {
    if (!c || !out_n || (n && (!boards || !out))) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return expand_boards(c, boards, first_cell_masks, n, target, out, cap, out_n);
}

int sdk_frontier_refine(sdk_ctx* c, uint64_t first, uint64_t step, uint64_t target, uint64_t* size,
                        uint64_t* leaves) {
    if (!c) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    int rc = refine_frontier(c, first, step, UINT64_MAX, target);
    if (rc) return rc;
    if (size) *size = c->fr_size;
    if (leaves) *leaves = c->fr_leaves;
    return SDK_OK;
}

int sdk_frontier_refine_range(sdk_ctx* c, uint64_t lo, uint64_t hi, uint64_t target, uint64_t* size,
                              uint64_t* leaves) {
    if (!c) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    int rc = refine_frontier(c, lo, 1, hi, target);
    if (rc) return rc;
    if (size) *size = c->fr_size;
    if (leaves) *leaves = c->fr_leaves;
    return SDK_OK;
}

int sdk_frontier_refine_head(sdk_ctx* c, uint64_t lo, uint64_t mid, uint64_t hi, uint64_t target, uint64_t* size,
                             uint64_t* leaves) {
    if (!c) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    int rc = refine_head(c, lo, mid, hi, target);
    if (rc) return rc;
    if (size) *size = c->fr_size;
    if (leaves) *leaves = c->fr_leaves;
    return SDK_OK;
}

int sdk_frontier_boards_dev(sdk_ctx* c, void** d_boards, uint64_t* size) {
    if (!c || !d_boards || !size) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->fr_valid) return fail(SDK_EINVAL, "no frontier: call sdk_frontier_build first");
    *d_boards = c->fr_a.p;
    *size = c->fr_size;
    return SDK_OK;
}

int sdk_frontier_load_dev(sdk_ctx* c, const void* d_boards, uint64_t n) {
    if (!c || (n && !d_boards)) return fail(SDK_EINVAL, "NULL argument");
    if (n > kFrontierCap) return fail(SDK_EINVAL, "at most %llu frontier boards", (unsigned long long)kFrontierCap);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    c->fr_valid = false;
    const char* src = static_cast<const char*>(d_boards);
    const char* a0 = static_cast<const char*>(c->fr_a.p);
    if (n && src == a0) {
        c->fr_size = n;                     // already in place
    } else if (n && a0 && src > a0 && src < a0 + c->fr_a.bytes) {
        // a range of the current frontier (overlapping copy): through fr_b
        int rc;
        if ((rc = ensure(c->fr_b, n * 81))) return rc;
        HIPCALL(hipMemcpyAsync(c->fr_b.p, d_boards, n * 81, hipMemcpyDeviceToDevice, c->stream));
        std::swap(c->fr_a, c->fr_b);
        c->fr_size = n;
    } else {
        int rc;
        if ((rc = ensure(c->fr_a, std::max<uint64_t>(n, 1) * 81))) return rc;
        if (n) HIPCALL(hipMemcpyAsync(c->fr_a.p, d_boards, n * 81, hipMemcpyDeviceToDevice, c->stream));
        c->fr_size = n;
    }
    c->fr_leaves = 0;
    c->fr_levels = 0;
    c->fr_valid = true;
    return SDK_OK;
}

int sdk_frontier_count_dev(sdk_ctx* c, uint64_t first, uint64_t step, uint64_t end, uint64_t limit, void* d_result) {
    if (!c || !d_result) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return frontier_count(c, first, step, end, limit, static_cast<unsigned long long*>(d_result));
}

int sdk_frontier_first_dev(sdk_ctx* c, uint64_t lo, uint64_t hi, void* d_found, void* d_best) {
    if (!c || !d_found || !d_best) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCALL(hipSetDevice(c->device));
    return frontier_first(c, lo, hi, static_cast<long long*>(d_found), static_cast<uint8_t*>(d_best));
}

int sdk_comm_unique_id(uint8_t* id) {
    if (!id) return fail(SDK_EINVAL, "NULL argument");
    ncclUniqueId u;
    NCCLCALL(ncclGetUniqueId(&u));
    std::memcpy(id, u.internal, SDK_COMM_ID_BYTES);
    return SDK_OK;
}

int sdk_comm_init(sdk_ctx* c, const uint8_t* id, int rank, int world) {
    if (!c || !id) return fail(SDK_EINVAL, "NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(SDK_EINVAL, "bad rank %d / world %d", rank, world);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->comm) return fail(SDK_EINVAL, "context already has a communicator");
    HIPCALL(hipSetDevice(c->device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, SDK_COMM_ID_BYTES);
    NCCLCALL(ncclCommInitRank(&c->comm, world, u, rank));
    c->comm_rank = rank;
    c->comm_world = world;
    return SDK_OK;
}

int sdk_comm_init_all(const int* devices, int ndev, sdk_ctx** ctxs) {
    if (!devices || !ctxs || ndev < 1) return fail(SDK_EINVAL, "need ndev >= 1 devices and contexts");
    for (int k = 0; k < ndev; ++k) {
        ctxs[k] = nullptr;
        for (int j = 0; j < k; ++j)
            if (devices[j] == devices[k]) return fail(SDK_EINVAL, "device %d listed twice", devices[k]);
    }
    int rc = SDK_OK;
    for (int k = 0; k < ndev && rc == SDK_OK; ++k) rc = sdk_create(devices[k], &ctxs[k]);
    std::vector<ncclComm_t> comms(ndev, nullptr);
    if (rc == SDK_OK) {
        const ncclResult_t r = ncclCommInitAll(comms.data(), ndev, devices);
        if (r != ncclSuccess) rc = fail(SDK_ECOMM, "ncclCommInitAll: %s", ncclGetErrorString(r));
    }
    if (rc != SDK_OK) {
        const std::string msg = g_last_error;
        for (int k = 0; k < ndev; ++k) {
            if (ctxs[k]) (void)sdk_destroy(ctxs[k]);
            ctxs[k] = nullptr;
        }
        g_last_error = msg;
        return rc;
    }
    for (int k = 0; k < ndev; ++k) {
        ctxs[k]->comm = comms[k];
        ctxs[k]->comm_rank = k;
        ctxs[k]->comm_world = ndev;
    }
    return SDK_OK;
}

int sdk_comm_destroy(sdk_ctx* c) {
    if (!c) return fail(SDK_EINVAL, "ctx is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->comm) return SDK_OK;
    HIPCALL(hipSetDevice(c->device));
    HIPCALL(hipStreamSynchronize(c->stream));
    ncclComm_t comm = c->comm;
    c->comm = nullptr;
    c->comm_rank = 0;
    c->comm_world = 1;
    NCCLCALL(ncclCommDestroy(comm));
    return SDK_OK;
}

int sdk_comm_allreduce_dev(sdk_ctx* c, void* d_buf, size_t count, int dtype, int op) {
    if (!c || (count && !d_buf)) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->comm) return fail(SDK_EINVAL, "no communicator: call sdk_comm_init first");
    ncclDataType_t t;
    switch (dtype) {
        case SDK_COMM_U64: t = ncclUint64; break;
        case SDK_COMM_I64: t = ncclInt64; break;
        case SDK_COMM_U8: t = ncclUint8; break;
        default: return fail(SDK_EINVAL, "bad dtype %d", dtype);
    }
    ncclRedOp_t o;
    switch (op) {
        case SDK_COMM_SUM: o = ncclSum; break;
        case SDK_COMM_MIN: o = ncclMin; break;
        case SDK_COMM_MAX: o = ncclMax; break;
        default: return fail(SDK_EINVAL, "bad op %d", op);
    }
    HIPCALL(hipSetDevice(c->device));
    NCCLCALL(ncclAllReduce(d_buf, d_buf, count, t, o, c->comm, c->stream));
    return SDK_OK;
}

int sdk_comm_broadcast_dev(sdk_ctx* c, void* d_buf, size_t bytes, int root) {
    if (!c || (bytes && !d_buf)) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->comm) return fail(SDK_EINVAL, "no communicator: call sdk_comm_init first");
    if (root < 0 || root >= c->comm_world) return fail(SDK_EINVAL, "bad root %d", root);
    HIPCALL(hipSetDevice(c->device));
    NCCLCALL(ncclBroadcast(d_buf, d_buf, bytes, ncclUint8, root, c->comm, c->stream));
    return SDK_OK;
}

int sdk_comm_p2p_dev(sdk_ctx* c, int nops, const int* ops, const int* peers, void* const* bufs, const size_t* bytes) {
    if (!c || nops < 0 || (nops && (!ops || !peers || !bufs || !bytes))) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->comm) return fail(SDK_EINVAL, "no communicator: call sdk_comm_init first");
    for (int k = 0; k < nops; ++k) {
        if (ops[k] != SDK_COMM_SEND && ops[k] != SDK_COMM_RECV) return fail(SDK_EINVAL, "bad p2p op %d", ops[k]);
        if (peers[k] < 0 || peers[k] >= c->comm_world || peers[k] == c->comm_rank)
            return fail(SDK_EINVAL, "bad p2p peer %d (rank %d of %d)", peers[k], c->comm_rank, c->comm_world);
        if (bytes[k] && !bufs[k]) return fail(SDK_EINVAL, "NULL p2p buffer");
    }
    HIPCALL(hipSetDevice(c->device));
    NCCLCALL(ncclGroupStart());
    ncclResult_t r = ncclSuccess;
    for (int k = 0; k < nops && r == ncclSuccess; ++k) {
        if (!bytes[k]) continue;   // both sides of a pair agree on the size, so both skip
        r = ops[k] == SDK_COMM_SEND ? ncclSend(bufs[k], bytes[k], ncclUint8, peers[k], c->comm, c->stream)
                                    : ncclRecv(bufs[k], bytes[k], ncclUint8, peers[k], c->comm, c->stream);
    }
    const ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess) return fail(SDK_ECOMM, "ncclSend/ncclRecv: %s", ncclGetErrorString(r));
    if (r2 != ncclSuccess) return fail(SDK_ECOMM, "ncclGroupEnd: %s", ncclGetErrorString(r2));
    return SDK_OK;
}

int sdk_comm_send_dev(sdk_ctx* c, const void* d_buf, size_t bytes, int peer) {
    const int op = SDK_COMM_SEND;
    void* buf = const_cast<void*>(d_buf);
    return sdk_comm_p2p_dev(c, 1, &op, &peer, &buf, &bytes);
}

int sdk_comm_recv_dev(sdk_ctx* c, void* d_buf, size_t bytes, int peer) {
    const int op = SDK_COMM_RECV;
    return sdk_comm_p2p_dev(c, 1, &op, &peer, &d_buf, &bytes);
}

int sdk_comm_allgather_dev(sdk_ctx* c, const void* d_send, void* d_recv, size_t bytes) {
    if (!c || (bytes && (!d_send || !d_recv))) return fail(SDK_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->comm) return fail(SDK_EINVAL, "no communicator: call sdk_comm_init first");
    HIPCALL(hipSetDevice(c->device));
    NCCLCALL(ncclAllGather(d_send, d_recv, bytes, ncclUint8, c->comm, c->stream));
    return SDK_OK;
}

}  // extern "C"
