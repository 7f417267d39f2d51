// reduce_args.h -- what the host and the level-minimising pass (reduce32_kernel.h) share: its
// arguments.  Plain C++.
#pragma once
#include <cstdint>

#include "prop32_args.h"

namespace sdk {

struct Reduce32Args {
    Prop32Args p;            // in, out, n, heads (zeroed); status, the list and the schedule are unused
    const uint8_t* order;    // [n][81]: row i is the cell order of board i's rounds; a byte >= 81 is no cell
    int8_t* status;          // [n]: 1 eligible (out = the level-minimal puzzle), 0 not (out = the input)
    uint32_t level;          // 1..3: the technique set R_level
};

}  // namespace sdk
