// select_kernel.h -- the selection kernels of sdk_generate_graded: an order-preserving stream
// compaction of 81-byte rows.
//
// A round of the call leaves m candidate rows in work buffers (puzzles, grids, generator status,
// level, open count).  Three launches keep the hits, in stream order, behind the hits of the earlier
// rounds:
//   flag     one wave per tile of 64 consecutive rows.  The tile (5,184 bytes, 16-byte aligned) goes
//            to LDS in 16-byte pieces; each lane then counts the clues of its own row, evaluates the
//            predicate (status SDK_SOLVED, bit `level` of the mask, clues_lo <= clues <= clues_hi; with
//            ratings, sdk_generate_rated: a level-4 row also bd_lo <= backdoors <= bd_hi; with
//            subsets counts, sdk_generate_subsets: a level-4 row also o4_lo <= open4 <= o4_hi) and
//            the wave stores its 64-bit ballot and the ballot's popcount.
//   scan     ONE workgroup loops over the tile counts (a round of 2^24 rows has 262,144 of them): an
//            exclusive prefix sum that starts at the hits found so far (SelWord::total) and leaves
//            the new total there.  It is a launch of its own, so no wave ever waits for another
//            workgroup's partial sum: the launch boundary orders flag before scan before scatter.
//   scatter  one wave per tile.  A hit's rank is the tile's offset plus the hits below it in the
//            ballot (v_mbcnt); ranks >= n are dropped.  The tile's kept rows are consecutive output
//            rows, i.e. ONE byte range [81 rank0, 81 (rank0 + kept)) of the output, which usually
//            starts and ends inside a dword whose other bytes belong to the tiles before and after
//            -- written by other workgroups at the same time.  So the rows are packed in LDS at the
//            output's own 16-byte phase, the 16-byte pieces that lie wholly inside the range are
//            stored as such, and the (at most 15 + 15) bytes before and after them one byte each:
//            no store touches a byte outside the tile's range and nothing is read-modify-written.
//            Level, open count, stream index and the ratings go out per hit; the hit of rank n - 1 also leaves
//            its round row (+ 1) in SelWord::last, from which the host computes `scanned`.
//
// Bounds: the work buffers hold whole tiles, so the 16-byte tile loads stay inside them for a last
// partial tile as well; rows >= m are never hits.  Every output index is a rank < n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select_args.h"

namespace sdk {

// a tile into LDS, 16 bytes per lane and step (both sides 16-byte aligned)
__device__ __forceinline__ void sel_load_tile(uint8_t* lds, const uint8_t* rows, uint32_t tile, uint32_t lane) {
    const uint4* src = reinterpret_cast<const uint4*>(rows + (size_t)tile * kSelTileBytes);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (uint32_t i = lane; i < kSelTileVecs; i += kSelTileRows) dst[i] = src[i];
}

__global__ __launch_bounds__(64) void select_flag_kernel(SelFlagArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kSelTileBytes];
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    sel_load_tile(tile, a.puzzles, t, lane);
    __syncthreads();
    const uint8_t* r = tile + 81u * lane;
    uint32_t clues = 0;
#pragma unroll 9
    for (uint32_t q = 0; q < 81u; ++q) clues += r[q] != 0;
    const uint32_t row = t * kSelTileRows + lane;
    bool hit = false;
    if (row < a.m && a.status[row] == 1) {
        const uint32_t lv = a.level[row];
        hit = lv < 32u && ((a.level_mask >> lv) & 1u) && clues >= a.clues_lo && clues <= a.clues_hi;
        if (hit && a.backdoors && lv == 4u) {       // rated generation: the search-level rows by their rating
            const uint32_t bd = a.backdoors[row];
            hit = bd >= a.bd_lo && bd <= a.bd_hi;
        }
        if (hit && a.open4 && lv == 4u) {           // ... or by what the subsets leave open
            const uint32_t o4 = a.open4[row];
            hit = o4 >= a.o4_lo && o4 <= a.o4_hi;
        }
    }
    const unsigned long long b = __ballot(hit);
    if (lane == 0) {
        a.ballot[t] = b;
        a.count[t] = (uint32_t)__popcll(b);
    }
}

__global__ __launch_bounds__(1024) void select_scan_kernel(SelScanArgs a) {
    __shared__ uint32_t wsum[kSelScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    uint32_t run = a.word->total;       // read by every thread; written once, after the last barrier
    for (uint32_t base = 0; base < a.tiles; base += kSelScanThreads) {
        const uint32_t i = base + tid;
        const uint32_t v = i < a.tiles ? a.count[i] : 0u;
        uint32_t x = v;                 // inclusive scan inside the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wsum[w] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < kSelScanThreads / 64; ++k) {
            const uint32_t s = wsum[k];
            before += k < w ? s : 0u;
            all += s;
        }
        if (i < a.tiles) a.offset[i] = run + before + (x - v);
        run += all;
        __syncthreads();                // wsum is rewritten by the next step
    }
    if (tid == 0) a.word->total = run;
}

__global__ __launch_bounds__(64) void select_scatter_kernel(SelScatterArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kSelTileBytes];
    __shared__ __attribute__((aligned(16))) uint8_t pack[kSelTileBytes + 16];
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    const unsigned long long b = a.ballot[t];
    const uint32_t rank0 = a.offset[t];
    if (b == 0ull || rank0 >= a.n) return;          // (the whole wave: nothing of this tile is kept)
    const uint32_t kept = min((uint32_t)__popcll(b), a.n - rank0);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    const bool keep = ((b >> lane) & 1ull) && below < kept;
    const uint32_t row = t * kSelTileRows + lane;
    if (keep) {
        const uint32_t rank = rank0 + below;
        if (a.out_level) a.out_level[rank] = a.level[row];
        if (a.out_open) a.out_open[rank] = a.open[row];
        if (a.out_index) a.out_index[rank] = a.first + row;
        if (a.out_backdoors) a.out_backdoors[rank] = a.backdoors ? a.backdoors[row] : (uint8_t)0xFFu;
        if (a.out_key) a.out_key[rank] = a.key ? a.key[row] : (uint8_t)0xFFu;
        if (a.out_open4) a.out_open4[rank] = a.open4 ? a.open4[row] : (uint8_t)0xFFu;
        if (rank == a.n - 1u) a.word->last = row + 1u;
    }
    // the tile's byte range of an output, seen from the 16-byte boundary at or before its start
    const size_t byte0 = (size_t)81u * rank0;
    const uint32_t head = (uint32_t)(byte0 & 15u);
    const uint32_t end = head + 81u * kept;
    const uint32_t in0 = (head + 15u) & ~15u, in1 = end & ~15u;     // in0 <= 16 < 81 <= end: in0 <= in1
    for (int pass = 0; pass < 2; ++pass) {
        sel_load_tile(stage, pass ? a.grids : a.puzzles, t, lane);
        __syncthreads();
        if (keep) {
            const uint8_t* s = stage + 81u * lane;
            uint8_t* d = pack + head + 81u * below;
#pragma unroll 9
            for (uint32_t q = 0; q < 81u; ++q) d[q] = s[q];
        }
        __syncthreads();
        uint8_t* base = (pass ? a.out_grids : a.out_puzzles) + (byte0 - head);   // 16-byte aligned
        for (uint32_t o = in0 + 16u * lane; o < in1; o += 16u * kSelTileRows)
            *reinterpret_cast<uint4*>(base + o) = *reinterpret_cast<const uint4*>(pack + o);
        if (lane < in0 - head) base[head + lane] = pack[head + lane];
        if (lane < end - in1) base[in1 + lane] = pack[in1 + lane];
        __syncthreads();                // stage and pack are rewritten by the next pass
    }
}

}  // namespace sdk
