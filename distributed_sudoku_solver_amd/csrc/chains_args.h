// chains_args.h -- what the host and the chains stage (chains_kernel.h) share: its arguments.  Plain C++.
#pragma once
#include <cstdint>

namespace sdk {

// One slice of sdk_chains_batch, after its grade pass, search, scatter and verdict kernel: the work items are
// the wings stage's (wings_args.h) -- the entries of the grade pass's undecided list whose board came out at
// level 4.  The list's length stays on the device.
struct Chains32Args {
    const uint8_t* in;       // the slice's boards [n][81]
    const uint8_t* level;    // [n] the slice's final grades
    const uint32_t* list;    // the grade pass's list: [0] its length, then board indices
    uint64_t n;              // boards of the slice (every list entry is below it)
    uint32_t* next;          // the dequeue counter (zeroed per slice)
    uint8_t* open4;          // [n], filled with 0xFF before the launch: the open cells of F_4
    uint8_t* open5;          // [n], filled with 0xFF before the launch: the open cells of F_5
    uint8_t* open6;          // [n], filled with 0xFF before the launch: the open cells of F_6
    uint8_t* open7;          // [n], filled with 0xFF before the launch: the open cells of F_7
};

}  // namespace sdk
