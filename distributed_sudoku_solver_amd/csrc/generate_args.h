// generate_args.h -- the arguments of generate_kernel (generate_kernel.h) and the constants the host sizes
// its grid and its fill bound by.  Plain C++.
#pragma once
#include <cstdint>

namespace sdk {

constexpr int kGenThreads = 64;             // one wave per workgroup (waves share nothing)
constexpr int kGenWavesPerCu = 6;           // what the LDS holds
constexpr uint32_t kGenFloor = 1u << 20;    // the fill's own bound is never below this (= the default cap)

struct GenArgs {
    uint64_t seed_mul;       // seed * 0x100000001B3
    uint64_t first;          // row i is stream index first + i
    uint32_t n;              // rows of this launch (<= 2^24)
    uint32_t cap;            // a grid is kept iff its placements are <= cap
    uint32_t hard;           // max(cap, kGenFloor): the fill stops before placement hard + 1
    uint8_t* grids;          // uint8[n][81]
    uint8_t* order;          // uint8[n][81], nullable
    uint32_t* placements;    // uint32[n], nullable
    uint32_t* next;          // the dequeue counter (zeroed before the launch)
};

}  // namespace sdk
