// rate_args.h -- what the host and the rating pass (rate32_kernel.h) share: its arguments.  Plain C++.
#pragma once
#include <cstdint>

namespace sdk {

// One slice of sdk_rate_batch, after its grade pass, search, scatter and verdict kernel: the work items
// are the entries of the grade pass's undecided list whose board came out at level 4 (the listed boards
// with search verdict 1 and clean givens).  The list's length stays on the device.
struct Rate32Args {
    const uint8_t* in;       // the slice's boards [n][81] (the parents)
    const uint8_t* sol;      // the slice's answers [n][81]: row j of a level-4 board is its completion
    const uint8_t* level;    // [n] the slice's final grades
    const uint32_t* list;    // the grade pass's list: [0] its length, then board indices
    uint64_t n;              // boards of the slice (every list entry is below it)
    uint32_t* next;          // the dequeue counter (zeroed per slice)
    uint8_t* backdoors;      // [n], filled with 0xFF before the launch
    uint8_t* key;            // [n] or null, filled with 0xFF before the launch
    uint32_t lc_every;       // the fast pass's schedule: a locked-candidates pass after step lc_first,
    uint32_t lc_first;       // then every lc_every-th (any schedule reaches the same fixpoints)
};

}  // namespace sdk
