// prop32_args.h -- what the host and the two propagation passes (prop32_kernel.h; the grading pass,
// grade32_kernel.h) share: their arguments and the dequeue-counter layout.  Plain C++.
#pragma once
#include <cstdint>

namespace sdk {

constexpr uint32_t kP32Heads = 8;        // dequeue counters, one per XCD segment of the groups
constexpr uint32_t kP32HeadStride = 32;  // words between counters (own cache lines)

// the step limit of the passes that run to a fixpoint (the grading pass, grade32_kernel.h, where the
// bound is derived; the rating pass, rate32_kernel.h): a termination guard, never a hand-off
constexpr uint32_t kG32MaxSteps = 768;   // > 729 + 3

struct Prop32Args {
    const uint8_t* in;       // boards [n][81]; 16-byte aligned
    uint8_t* out;            // [n][81]; 16-byte aligned
    int8_t* status;          // [n]: 1 solved, 0 no completion, kStUndecided
    uint64_t n;
    uint32_t* heads;         // kP32Heads counters kP32HeadStride words apart (zeroed)
    uint32_t* list;          // [0] undecided boards, then their indices (list[0] zeroed)
    uint8_t* list_in;        // the undecided boards' inputs, dense, in list order
    uint32_t lc_every;       // a locked-candidates pass after step lc_first, then every lc_every-th
    uint32_t lc_first;       // step (lc_first = lc_every: after every lc_every-th step)
    uint32_t max_steps;      // boards still live after this many steps are undecided
    int handover;            // the list gets an undecided board's propagated grid (its closed cells
                             // filled in: the same completions) instead of its input; not for
                             // boards with a duplicated or out-of-domain given
    uint32_t tail_live;      // handover: from step tail_step on, a group with at most this many
    uint32_t tail_step;      // live boards hands them to the search and ends (0 = never)
};

struct Grade32Args {
    Prop32Args p;        // in, out, status, n, heads, list, list_in, handover (no schedule, no tail)
    uint8_t* level;      // [n]
    uint8_t* open;       // [n]
};

}  // namespace sdk
