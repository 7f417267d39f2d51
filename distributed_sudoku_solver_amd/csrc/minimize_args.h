// minimize_args.h -- the arguments of minimize_round_kernel (minimize_kernel.h has the rounds' protocol)
// and the bytes of the batch a workgroup covers in one pass, which the host sizes the grid by.  Plain C++.
#pragma once
#include <cstdint>

namespace sdk {

struct MinRoundArgs {
    const uint8_t* src;      // launch 0: the input boards; later: cur
    uint8_t* cur;            // the boards so far (the call's `out`)
    uint8_t* cand;           // round q's candidates (null at q = 81)
    const uint8_t* order;    // uint8[n][81]
    const int8_t* status;    // the inputs' verdicts
    const int8_t* cst;       // round q - 1's candidate verdicts (unread at q = 0)
    uint64_t n;
    uint32_t q;              // 0..81
};

constexpr int kMinThreads = 256;
constexpr int kMinBlockBytes = 4 * kMinThreads;   // one thread per four bytes of the batch

}  // namespace sdk
