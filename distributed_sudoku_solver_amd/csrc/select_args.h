// select_args.h -- arguments of the selection kernels (select_kernel.h, select_launch.hip): the
// order-preserving compaction of a round of sdk_generate_graded / _rated / _subsets, shared with its driver in
// sudoku_hip.hip (launch_generate_graded).
#pragma once
#include <cstdint>

namespace sdk {

constexpr uint32_t kSelTileRows = 64;                    // rows per tile: one wave, one row per lane
constexpr uint32_t kSelTileBytes = kSelTileRows * 81;    // 5,184: a multiple of 16, so every tile of a
                                                         // 16-byte aligned round buffer is aligned too
constexpr uint32_t kSelTileVecs = kSelTileBytes / 16;    // 324 16-byte pieces
constexpr uint32_t kSelScanThreads = 1024;               // the scan's one workgroup

// The call's device word, read back once per round (8 bytes).  `total` < 2^32: a round starts only
// below the quota (n <= 2^31-1) and adds at most 2^24 hits.
struct SelWord {
    uint32_t total;     // hits found so far in the window, whatever the quota (the scan adds a round's)
    uint32_t last;      // 1 + the round row of the hit of rank n-1, written by the scatter of the round
                        // that holds it (0 until then)
};

// A round's rows are rows [0, m) of the work buffers; every buffer holds whole tiles (the rows from m
// to the end of the last tile are read and ignored).
struct SelFlagArgs {
    const uint8_t* puzzles;      // [tiles][64][81], 16-byte aligned
    const int8_t* status;        // [m] generator status
    const uint8_t* level;        // [m] grade
    uint32_t m;
    uint32_t level_mask, clues_lo, clues_hi;
    const uint8_t* backdoors;    // [m] rating, nullable (sdk_generate_rated): a level-4 row is a hit only
    uint32_t bd_lo, bd_hi;       // with bd_lo <= backdoors <= bd_hi; rows of other levels are not filtered
    const uint8_t* open4;        // [m] subsets count, nullable (sdk_generate_subsets): a level-4 row is a hit
    uint32_t o4_lo, o4_hi;       // only with o4_lo <= open4 <= o4_hi; rows of other levels are not filtered
    unsigned long long* ballot;  // [tiles] bit l = row 64 t + l is a hit
    uint32_t* count;             // [tiles] its popcount
};

struct SelScanArgs {
    const uint32_t* count;       // [tiles]
    uint32_t* offset;            // [tiles] hits before the tile, the earlier rounds' included
    uint32_t tiles;
    SelWord* word;
};

struct SelScatterArgs {
    const uint8_t* puzzles;      // the round's rows, as SelFlagArgs
    const uint8_t* grids;
    const uint8_t* level;
    const uint8_t* open;
    const unsigned long long* ballot;
    const uint32_t* offset;
    uint64_t first;              // stream index of round row 0
    uint32_t n;                  // the quota: ranks >= n are not written
    uint8_t* out_puzzles;        // [n][81], 16-byte aligned
    uint8_t* out_grids;          // [n][81], 16-byte aligned
    uint8_t* out_level;          // [n], nullable
    uint8_t* out_open;           // [n], nullable
    uint64_t* out_index;         // [n], nullable
    const uint8_t* backdoors;    // the round's ratings, nullable: SDK_RATE_NONE goes out instead
    const uint8_t* key;
    uint8_t* out_backdoors;      // [n], nullable
    uint8_t* out_key;            // [n], nullable
    const uint8_t* open4;        // the round's subsets counts, nullable: SDK_SUBSETS_NONE goes out instead
    uint8_t* out_open4;          // [n], nullable
    SelWord* word;
};

}  // namespace sdk
