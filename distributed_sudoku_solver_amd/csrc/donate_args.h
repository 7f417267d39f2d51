// donate_args.h -- the layout of a subtree-donation area (solve4_kernel.h, "subtree donation", has the protocol)
// and of the split phase's saved stacks.  The host sizes, zeroes and reads these areas
// (sudoku_hip.hip); the list kernels that feed a donation launch are donate_launch.hip's.  Plain C++.
#pragma once
#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>

namespace sdk {

constexpr int kDnXcds = 8;
struct DnXcd {
    uint32_t done;            // boards finished on this XCD
    uint32_t reg_tail;        // registrations of idle waves
    uint32_t reg_head;        // registrations taken by donors (<= reg_tail)
    uint32_t pad[29];
};
// Resumed split boards (round 4).  The split phase leaves the stack of a board that reaches
// the split budget (split_save4); the collect kernel reserves records and items for it, and
// dn_seed_kernel (donate_launch.hip) turns its open subtrees -- the current node's and every
// level's untried digits -- into items of a board record before the donation launch.  Idle
// waves take those items from the seed queue first (dn_idle4), so the heavy boards go on
// from where the split phase left them, spread over the grid, instead of restarting.
struct DnSeed {
    uint32_t next;            // seed-queue entries taken by idle waves
    uint32_t total;           // seed-queue entries (items of the resumed boards)
    uint32_t boards;          // resumed boards: each ends as a record (counted at the exit)
    uint32_t res_boards, res_items;   // the collect kernel's reservations (<= kSeedBoards / kSeedItems)
    uint32_t pad[27];
};
struct DnCtl {
    uint32_t epoch;           // launch number (host): mailbox and registration entries carry it
    uint32_t delivered;       // items handed out by the launch

    uint32_t item_alloc;      // item records handed out
    uint32_t nrec;            // board records handed out
    uint32_t exit_all, parts_ended, finalized;   // diagnostics
    uint32_t next;            // the launch's board dequeue counter
    uint32_t err;             // sticky (not cleared by the prep launch; the host reads and clears
                              // it): kDnErrReg / kDnErrLock, a bounded wait ran out
    uint32_t fault;           // test only (SDK_OPT_DN_FAULT): registrations are not written
    uint32_t started;         // diagnostics: waves taking part (written by workgroup 0)
    uint32_t helpers;         // waves taking part per listed board (SDK_OPT_DONATE_HELPERS), plus 64
    uint32_t pad[20];
    DnXcd x[kDnXcds];
    DnSeed seed;              // own cache line: idle waves take seed items at the launch's start
};
constexpr uint32_t kDnErrReg = 1u, kDnErrLock = 2u, kDnErrSeed = 4u;
// ticket reservation: an add, then the tickets past reg_tail handed back by one compare-and-swap
// (round 4 A/B, profiles/r04 via tools/gpu_r04j.sh: a compare-and-swap loop never passes reg_tail,
// but under contention most donation checks fail -- 1,300 instead of 1,765 items on the heavy-1000
// launch, 1.25 vs 1.08 ms).  SDK_DN_ERRCHECK=0: no error-word read (measurement)
#ifndef SDK_DN_ERRCHECK
#define SDK_DN_ERRCHECK 1
#endif
// bound of every wait on another wave, in s_memrealtime ticks (100 MHz): 0.2 s -- a
// registration is written right after its ticket is drawn and a lock is held for a few
// hundred cycles, so only a wave that cannot run (a fault, or a preempted queue) gets near it
constexpr uint64_t kDnWaitTicks = 20000000ull;
#ifndef SDK_DN_HELP_CAP
#define SDK_DN_HELP_CAP 256
#endif
constexpr uint64_t kDnHelpCap = SDK_DN_HELP_CAP;   // listed boards that get helper waves
constexpr uint32_t kDnItems = 1u << 16;
constexpr uint32_t kDnRecs = 1u << 14;
constexpr uint32_t kDnRegX = 1u << 14;        // registrations per XCD
constexpr uint32_t kDnReg = kDnRegX * kDnXcds;
constexpr uint32_t kDnMbox = 1u << 14;        // workgroups of a donating launch, at most
constexpr int kDnList = 16;
constexpr uint32_t kDnNone = 0xFFFFFFFFu, kDnOwner = 0xFFFFFFFEu;
#ifndef SDK_DN_EVERY
#define SDK_DN_EVERY 16
#endif
constexpr uint32_t kDnEvery = SDK_DN_EVERY;   // nodes between a part's donation / pruning checks
#ifndef SDK_DN_SLEEP
// s_sleep argument between an idle wave's mailbox polls (x 64 clocks: ~3.4 us).  Shorter
// sleeps let the ~23 idle waves of a CU take issue slots and memory bandwidth from the one
// that still searches (s_sleep 4: the 64 heaviest hard boards 1.5 -> 9.7 ms).
#define SDK_DN_SLEEP 127
#endif
constexpr int kDnPruned = 3;                  // part status: stopped above a known completion
constexpr int kDnRetryLex = 3;                // board status of an exhaustive launch: solve again in LEX
struct DnItem {
    uint32_t board, rec, plen, pad0;
    uint32_t pad[4];
    uint2 w[27];              // root state, lane j: (y0 | y1 << 16, y2), snapshot encoding
    uint8_t sol[96];          // the part's completion
    uint32_t pad2[10];
};
struct DnRec {                // one per donating board
    uint32_t board, open, nhit, flags, maxd;
    uint32_t lock;            // LEX: guards `best` (taken by one half-wave at a time, see dn_finish_part4)
    uint32_t version;         // LEX: seqlock of `best` (odd while it is rewritten)
    uint32_t have;            // LEX: `best` holds a completion
    unsigned long long work;
    uint32_t first;           // exhaustive: the part that met the board's first completion
    uint32_t total;           // exhaustive: completions met by all parts
    uint32_t hit[kDnList];    // parts that hit the node budget (more: flags bit 0, undecided)
    uint8_t best[96];         // LEX: the smallest completion any part met
    uint8_t owner_sol[96];    // the board's own slot's completion
    uint32_t pad[20];
};
static_assert(sizeof(DnItem) == 384 && sizeof(DnRec) == 384 && sizeof(DnCtl) == 128 * (2 + kDnXcds), "donation layout");
constexpr size_t kDnRecOffset = sizeof(DnCtl);
constexpr size_t kDnItemOffset = kDnRecOffset + (size_t)kDnRecs * sizeof(DnRec);
constexpr size_t kDnRegOffset = kDnItemOffset + (size_t)kDnItems * sizeof(DnItem);
constexpr size_t kDnMboxOffset = kDnRegOffset + (size_t)kDnReg * 8;
constexpr size_t kDnSeedQOffset = kDnMboxOffset + (size_t)kDnMbox * 8;
constexpr size_t kDnBytes = kDnSeedQOffset + (size_t)kDnItems * 4;
constexpr uint32_t kSeedBoards = kDnRecs / 2;   // the other half stays for the launch's own donations
constexpr uint32_t kSeedItems = kDnItems / 2;
// the split phase's saved stacks: a board's levels 0..depth-1, the 32 lanes of its half each
constexpr uint32_t kSaveLv = 16;
constexpr uint32_t kSaveCap = 8192;
struct SplitSave {
    uint32_t count;           // saves claimed (those past kSaveCap are not written)
    uint32_t pad[31];
    uint2 hdr[kSaveCap];      // (board, depth)
    uint2 lv[kSaveCap][kSaveLv][32];
};

// What dn_collect_kernel needs to resume split boards (`save` null: every listed board restarts): the
// split phase's saved stacks and each board's entry, the donation area whose DnSeed takes the
// reservations, and the seed list.
struct DnResume {
    const SplitSave* save;
    const uint32_t* save_idx;
    DnCtl* ctl;
    uint32_t* seeds;          // [0] seeded boards, [1] restarted boards, then (board, entry) pairs
};
// A phased solve's control words, zeroed in one launch before its first phase: the split
// phase's dequeue counter and heads, the statistics, both donation launches' control blocks
// (their epochs set) and list lengths.
struct DnPrep {
    uint32_t* counter;
    uint32_t* heads;
    uint32_t heads_words;
    uint32_t* stat;
    uint32_t* ctl[2];
    uint32_t epoch[2];
    uint32_t fault;      // DnCtl.fault (SDK_OPT_DN_FAULT, test only)
    uint32_t helpers;    // DnCtl.helpers (SDK_OPT_DONATE_HELPERS)
    uint32_t* list[2];
    uint32_t* seeds;     // the seed list's two length words (nullable)
    uint32_t* save;      // SplitSave::count (nullable)
};

}  // namespace sdk
