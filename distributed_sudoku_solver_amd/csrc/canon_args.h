// canon_args.h -- what the host and the canonical-form stage (canon_kernel.h) share: its arguments.  Plain C++.
#pragma once
#include <cstdint>

namespace sdk {

// One slice of sdk_canonical_batch, after its classify path: one wave per board.
struct CanonArgs {
    const uint8_t* in;       // the slice's boards [n][81]
    const uint8_t* sol;      // classify's out [n][81]: the completion of a board of status SDK_SOLVED
    const int8_t* status;    // [n] classify's verdicts
    uint64_t n;              // boards of the slice
    uint8_t* canon;          // [n][81]; may be `in`
    uint8_t* solution;       // [n][81] or null; may be `sol` (only eligible boards' rows are written)
    uint8_t* gather;         // [n][81] or null
    uint8_t* relabel;        // [n][10] or null
    uint16_t* ties;          // [n] or null
};

}  // namespace sdk
