// minimize_kernel.h -- the round kernel of sdk_minimize_batch (greedy clue removal on the GPU).
//
// A minimise call is 81 rounds over the batch, enqueued without the host.  Round q tries cell
// order[i][q] of board i: this kernel writes the candidates (the current boards with that cell
// cleared), the classify path (sdk_classify_batch's, budget 0) gives every candidate its verdict,
// and the next round's launch of this kernel commits it -- verdict 1 (still exactly one
// completion) means the removal stays.  One launch does both in one pass over the batch:
//   commit round q - 1 into `cur`, then write round q's candidates from the committed boards.
// Launch 0 also copies the inputs into `cur` (src = the inputs; later launches src = cur), and
// launch 81 commits only.
//
// A board has no live candidate in a round when its input is not unique (status != 1: it must
// come back unchanged), when its cell is already empty, or when the order byte is >= 81 (no
// cell; the host entry point refuses such rows, the device entry point cannot).  It then gets
// kRefuted instead -- cells 0..7 hold 1..8 and cell 17 holds 9, so cell 8 has no candidate: both
// the propagation pass and the search refute it at their first step, and verdict 0 never commits.
//
// One thread per four bytes of the batch, plain dword accesses (the last dword of an odd batch
// byte by byte).  A thread reads two more bytes of its board that other threads may be writing:
// the committed cell (written only with 0, and read here only to decide "is it empty", which the
// commit flag already answers) -- so no ordering between threads is needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minimize_args.h"

namespace sdk {

__device__ __forceinline__ uint32_t min_refuted_cell(uint32_t c) {
    return c < 8u ? c + 1u : (c == 17u ? 9u : 0u);
}

__global__ __launch_bounds__(kMinThreads) void minimize_round_kernel(MinRoundArgs a) {
    const uint64_t total = a.n * 81u;
    const uint64_t stride = 4ull * gridDim.x * blockDim.x;
    for (uint64_t e0 = 4ull * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x); e0 < total; e0 += stride) {
        const bool whole = e0 + 4u <= total;
        uint32_t word = 0u;
        if (whole) {
            word = *reinterpret_cast<const uint32_t*>(a.src + e0);
        } else {
            for (uint32_t b = 0; e0 + b < total; ++b) word |= (uint32_t)a.src[e0 + b] << (8u * b);
        }
        uint32_t cur_w = 0u, cand_w = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint64_t e = e0 + b;
            if (e >= total) break;
            const uint64_t i = e / 81u;
            const uint32_t c = (uint32_t)(e - 81u * i);
            uint32_t v = (word >> (8u * b)) & 0xFFu;
            const bool unique = a.status[i] == 1;
            // round q - 1: its removal stays if the candidate still had exactly one completion
            uint32_t pc = 0xFFu;
            bool kept = false;
            if (a.q > 0u) {
                pc = a.order[i * 81u + (a.q - 1u)];
                kept = unique && a.cst[i] == 1;
            }
            if (kept && c == pc) v = 0u;
            cur_w |= v << (8u * b);
            if (a.q < 81u) {
                const uint32_t cell = a.order[i * 81u + a.q];
                bool live = false;
                if (unique && cell < 81u) live = !(kept && cell == pc) && a.src[i * 81u + cell] != 0;
                const uint32_t cv = live ? (c == cell ? 0u : v) : min_refuted_cell(c);
                cand_w |= cv << (8u * b);
            }
        }
        if (whole) {
            *reinterpret_cast<uint32_t*>(a.cur + e0) = cur_w;
            if (a.q < 81u) *reinterpret_cast<uint32_t*>(a.cand + e0) = cand_w;
        } else {
            for (uint32_t b = 0; e0 + b < total; ++b) {
                a.cur[e0 + b] = (uint8_t)(cur_w >> (8u * b));
                if (a.q < 81u) a.cand[e0 + b] = (uint8_t)(cand_w >> (8u * b));
            }
        }
    }
}

}  // namespace sdk
