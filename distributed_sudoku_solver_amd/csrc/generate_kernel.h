// generate_kernel.h -- random complete grids (and their clue-removal orders) on the GPU, ONE GRID
// PER LANE: the kernel of sdk_generate_grids / sdk_generate_puzzles.
//
// Grid k of seed S is the one csrc/gen_minimal.c makes (gen_grid_one), byte for byte: a randomised
// backtracking fill of the empty board in row-major order, driven by one splitmix64 stream whose
// state starts at S * 0x100000001B3 ^ (k + 1) * 0x9E3779B97F4A7C15.  On every entry to a cell (a
// re-entered cell draws afresh) the cell's candidates, in ascending-digit order, are shuffled by
// `for k = n-1 .. 1: j = splitmix() % (k + 1); swap(d[k], d[j])` and tried in that order.  After
// the fill the same stream draws the 81-entry removal order (`for i = 80 .. 1: j = splitmix() %
// (i + 1)`), the order gen_minimal_one's greedy removal follows: with it, the minimiser
// (minimize_kernel.h) turns the grid into exactly make_minimal's puzzle k.
//
// The recursion as a step machine.  A level of fill() only needs the digits it has not tried yet:
// at most eight after the first is placed, a nibble each with 0 as the end, one dword per cell.
// Together with the digit placed in each cell (a nibble per cell, as LaneLds::dig) and the 27 unit
// masks that is 419 bytes per lane, kept in LDS lane-interleaved ([entry][lane]); 26 816 bytes per
// wave, so six waves share a CU's 160 KiB.  Registers hold the stream, the cell, the placement
// count and the phase.  One fill step = one entry to a cell (shuffle its candidates, place the
// first, go on to the next cell -- or, with none, go back) or one return into a cell (take its
// digit back, place the next untried one or go further back).  The shuffle lives in a packed
// nibble vector in registers (a runtime-indexed local array would go to scratch), and `z % m`
// is reduced through the 32-bit halves of z, with m a compile-time constant in the shuffle, so no
// 64-bit division is emitted.  Once a lane's fill ends, its steps draw the order, one swap per
// step, in the dwords its stack no longer needs (byte q of the order = byte q & 3 of dword q >> 2).
//
// Waves are persistent.  Every kGenSteps steps the lanes that finished write their rows -- the
// wave together, a row at a time, 81 consecutive bytes from 64 lanes -- and the free lanes take new
// indices with one atomic per wave (solve_lane_kernel.h's refill).
//
// Bounds.  `placed` counts the digits written into a cell (gen_grid_order_batch's count).  A grid
// is kept iff its count is <= cap (SDK_OPT_GEN_CAP); one that is not kept is written as 81 zeros
// with the count 0xFFFFFFFF.  Its order row is still the stream's -- the order continues the
// stream where the fill leaves it, so the lane has to finish the fill to know it -- which is why
// the fill itself stops at `hard` = max(cap, kGenFloor) placements and not at a smaller cap: that
// is the bound of every loop here (a lane takes at most 2 * hard + 81 fill steps, then 80 order
// steps).  A fill stopped at `hard` draws its order from the stream as it stands.  No lane waits
// for another wave, and the only cross-lane traffic is through the wave's own LDS, in program
// order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "generate_args.h"

namespace sdk {

constexpr int kGenSteps = 32;               // steps between refills
constexpr uint32_t kGenAll = 0x3FEu;        // digits 1..9 as bits 1..9 (gen_minimal.c's layout)

struct GenLds {
    uint32_t stk[81][64];                   // untried digits of each level; after the fill, the order bytes
    uint16_t mask[27][64];                  // units: rows 0..8, columns 9..17, boxes 18..26
    uint8_t dig[41][64];                    // digit placed in cell c: nibble c & 1 of byte c >> 1
};
static_assert(sizeof(GenLds) == 26816, "six waves per CU");

enum : uint32_t { kGenIdle = 0, kGenFill = 1, kGenOrder = 2, kGenFin = 3 };

// a lane's registers
struct GenLane {
    uint64_t rng;
    uint32_t p;              // fill: the cell; order: the entry being drawn (80 .. 1)
    uint32_t placed;
    uint32_t phase;
    bool enter;              // fill: the cell is entered (else: returned into from the next one)
    bool lost;               // the fill did not complete (stopped at `hard`)
};

__host__ __device__ __forceinline__ uint64_t gen_splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// z % M through z's 32-bit halves (M a constant: multiplies, no division)
template <uint32_t M>
__host__ __device__ __forceinline__ uint32_t gen_mod_c(uint64_t z) {
    constexpr uint32_t t = (uint32_t)((1ull << 32) % M);
    return (((uint32_t)(z >> 32) % M) * t + (uint32_t)z % M) % M;
}

// z % m for 2 <= m <= 81, the same way with 32-bit divisions
__host__ __device__ __forceinline__ uint32_t gen_mod(uint64_t z, uint32_t m) {
    uint32_t t = 0xFFFFFFFFu % m + 1u;      // 2^32 % m
    if (t == m) t = 0u;
    return (((uint32_t)(z >> 32) % m) * t + (uint32_t)z % m) % m;
}

// one iteration of fill()'s shuffle: for k = K, swap nibbles K and j = splitmix() % (K + 1)
template <uint32_t K>
__host__ __device__ __forceinline__ void gen_shuffle_step(uint64_t& w, uint32_t n, uint64_t& rng) {
    if (K < n) {
        const uint32_t j = gen_mod_c<K + 1>(gen_splitmix(rng));
        const uint64_t x = ((w >> (4u * K)) ^ (w >> (4u * j))) & 15ull;
        w ^= (x << (4u * K)) | (x << (4u * j));
    }
}

// One fill step of lane state `s` over its LDS view `m` (stk(e), mask(u), dig(k) give references).
// Returns true when the fill has ended: all 81 cells placed, or s.lost.
template <class View>
__host__ __device__ __forceinline__ bool gen_fill_step(GenLane& s, const View& m, uint32_t hard) {
    const uint32_t p = s.p;
    const uint32_t r = (p * 57u) >> 9, c = p - 9u * r;                 // p / 9, p % 9 for p < 81
    const uint32_t b = ((r * 11u) >> 5) * 3u + ((c * 11u) >> 5);       // x / 3 for x < 9
    uint32_t mr = m.mask(r), mc = m.mask(9u + c), mb = m.mask(18u + b);
    const uint32_t sh = (p & 1u) * 4u;
    uint32_t byte = m.dig(p >> 1);
    uint64_t w;                            // the digits to try from here on: a nibble each, 0 ends
    if (s.enter) {
        uint32_t cand = kGenAll & ~(mr | mc | mb);
        uint32_t n = 0;
        w = 0;
        while (cand) {                     // ascending digits (at most nine)
            w |= (uint64_t)(uint32_t)__builtin_ctz(cand) << (4u * n);
            cand &= cand - 1u;
            ++n;
        }
        gen_shuffle_step<8>(w, n, s.rng);
        gen_shuffle_step<7>(w, n, s.rng);
        gen_shuffle_step<6>(w, n, s.rng);
        gen_shuffle_step<5>(w, n, s.rng);
        gen_shuffle_step<4>(w, n, s.rng);
        gen_shuffle_step<3>(w, n, s.rng);
        gen_shuffle_step<2>(w, n, s.rng);
        gen_shuffle_step<1>(w, n, s.rng);
    } else {                               // the next cell failed: take this cell's digit back
        const uint32_t old = ~(1u << ((byte >> sh) & 15u));
        mr &= old;
        mc &= old;
        mb &= old;
        w = m.stk(p);
    }
    const uint32_t d = (uint32_t)w & 15u;
    if (d && s.placed >= hard) {           // the bound of the fill: no placement hard + 1
        s.lost = true;
        return true;
    }
    if (d) {
        const uint32_t bit = 1u << d;
        mr |= bit;
        mc |= bit;
        mb |= bit;
        byte = (byte & ~(15u << sh)) | (d << sh);
    }
    m.mask(r) = (uint16_t)mr;
    m.mask(9u + c) = (uint16_t)mc;
    m.mask(18u + b) = (uint16_t)mb;
    if (d) {
        m.dig(p >> 1) = (uint8_t)byte;
        m.stk(p) = (uint32_t)(w >> 4);     // at most eight digits are left
        ++s.placed;
        s.enter = true;
        return ++s.p == 81u;
    }
    if (p == 0u) {                         // nothing left at cell 0 (fill() returning 0: no such grid)
        s.lost = true;
        return true;
    }
    s.p = p - 1u;
    s.enter = false;
    return false;
}

// the order starts as the identity (dword e holds bytes 4e .. 4e + 3)
template <class View>
__host__ __device__ __forceinline__ void gen_order_begin(GenLane& s, const View& m) {
#pragma unroll
    for (uint32_t e = 0; e < 21u; ++e) m.stk(e) = 0x03020100u + 0x04040404u * e;
    s.p = 80u;
    s.phase = kGenOrder;
}

// one swap of the Fisher-Yates draw; the last one ends the phase
template <class View>
__host__ __device__ __forceinline__ void gen_order_step(GenLane& s, const View& m) {
    const uint32_t i = s.p, j = gen_mod(gen_splitmix(s.rng), i + 1u);
    const uint8_t x = m.ord(i), y = m.ord(j);
    m.ord(i) = y;
    m.ord(j) = x;
    if (--s.p == 0u) s.phase = kGenFin;
}

#ifdef __HIPCC__
struct GenView {
    GenLds& L;
    const int lane;
    __device__ __forceinline__ uint32_t& stk(uint32_t e) const { return L.stk[e][lane]; }
    __device__ __forceinline__ uint16_t& mask(uint32_t u) const { return L.mask[u][lane]; }
    __device__ __forceinline__ uint8_t& dig(uint32_t k) const { return L.dig[k][lane]; }
    __device__ __forceinline__ uint8_t& ord(uint32_t q) const {
        return reinterpret_cast<uint8_t*>(&L.stk[q >> 2][lane])[q & 3u];
    }
};

__global__ __launch_bounds__(kGenThreads) void generate_kernel(GenArgs a) {
    __shared__ GenLds L;
    const int lane = threadIdx.x;
    const GenView m{L, lane};
    GenLane s{};
    s.phase = kGenIdle;
    uint32_t row = 0;                      // the lane's row of this launch
    bool more = true;                      // the queue may still hold rows (wave-uniform)

    for (;;) {
        // ---- the rows that are finished, one at a time by the whole wave ----
        uint64_t fin = __builtin_amdgcn_ballot_w64(s.phase == kGenFin);
        if (fin) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            while (fin) {
                const int src = __builtin_ctzll(fin);
                fin &= fin - 1ull;
                const uint32_t i = (uint32_t)__builtin_amdgcn_readlane((int)row, src);
                const uint32_t placed = (uint32_t)__builtin_amdgcn_readlane((int)s.placed, src);
                const bool keep = !__builtin_amdgcn_readlane((int)s.lost, src) && placed <= a.cap;
                const uint64_t at = (uint64_t)i * 81u;           // i < a.n: inside the outputs
                for (uint32_t t = (uint32_t)lane; t < 81u; t += 64u) {
                    const uint32_t byte = L.dig[t >> 1][src];
                    a.grids[at + t] = keep ? (uint8_t)((t & 1u) ? (byte >> 4) : (byte & 15u)) : (uint8_t)0;
                    if (a.order) a.order[at + t] = reinterpret_cast<const uint8_t*>(&L.stk[t >> 2][src])[t & 3u];
                }
                if (lane == 0 && a.placements) a.placements[i] = keep ? placed : 0xFFFFFFFFu;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (s.phase == kGenFin) s.phase = kGenIdle;
        }
        // ---- new rows for all lanes that are free: one atomic per wave ----
        if (more) {
            const uint64_t freem = __builtin_amdgcn_ballot_w64(s.phase == kGenIdle);
            if (freem) {
                const uint32_t take = (uint32_t)__popcll(freem);
                const int leader = __builtin_ctzll(freem);
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(a.next, take);
                base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
                if ((uint64_t)base + take >= a.n) more = false;
                if (s.phase == kGenIdle) {
                    const uint64_t idx = (uint64_t)base + (uint32_t)__popcll(freem & ((1ull << lane) - 1ull));
                    if (idx < a.n) {
                        row = (uint32_t)idx;
                        s.rng = a.seed_mul ^ (a.first + idx + 1ull) * 0x9E3779B97F4A7C15ull;
#pragma unroll
                        for (uint32_t u = 0; u < 27u; ++u) L.mask[u][lane] = 0;
                        s.p = 0;
                        s.placed = 0;
                        s.enter = true;
                        s.lost = false;
                        s.phase = kGenFill;
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(s.phase != kGenIdle) == 0 && !more) break;
        // ---- steps ----
#pragma nounroll
        for (int k = 0; k < kGenSteps; ++k) {
            if (s.phase == kGenFill) {
                if (gen_fill_step(s, m, a.hard)) {
                    if (a.order) gen_order_begin(s, m);
                    else s.phase = kGenFin;
                }
            } else if (s.phase == kGenOrder) {
                gen_order_step(s, m);
            }
            if (__builtin_amdgcn_ballot_w64(s.phase == kGenFill || s.phase == kGenOrder) == 0) break;
        }
    }
}
#endif  // __HIPCC__

}  // namespace sdk
