// canon_kernel.h -- the canonical form of a board under the Sudoku symmetries (sdk_canonical_batch;
// include/sudoku_hip.h has the contract, DESIGN.md "Canonical form" the reduction and the measurements)
//
// An eligible board P has exactly one completion S, a valid grid.  M is the smallest image of S over the
// 2 * 6^8 cell maps times 9! relabellings, C the smallest image of P over the symmetries that take S to
// M.  M is the minimum over 2 * 9 * 1296 constructed candidates k = (t * 9 + r0) * 1296 + q: G is S or its
// transpose (t), row r0 of G becomes row 0, q arranges the columns; the relabelling is forced by "row 0 is
// 1..9" and the other rows by sorting on their relabelled first cell (see canon_rows).
//
// One board per wave.  Everything about a candidate is kept in nibble-packed words -- nine 4-bit entries
// in a uint64_t, read with a shift -- so nothing is an array: no scratch, no dynamically indexed registers.
//   tables   per (t, r0), for the two band-mates r of r0: W[c] = the column in which row r0 holds the digit
//            G[r][c].  With the columns cc and their inverse, the image of row r is inv[W[cc[j]]] + 1: a
//            row of the image costs two shifts per cell and never touches a digit.  36 words in LDS.
//   phase 1  lane l takes q = l, l + 64, ... (21 values; the columns are decoded once per q) and walks the
//            18 (t, r0): the key of a candidate is row 1 of its image, the band-mate with the smaller first
//            cell.  At the minimum that cell is 4 (it lies in the box of 1, 2, 3, and the stacks and columns
//            that hold 4..9 in row 0 can be arranged to make it 4), so a candidate whose row 1 starts
//            higher is dropped and the key is the other eight nibbles: 32 bits.  A lane keeps its smallest
//            key, the last four candidates that have it (16 bits each in one word) and how many have it;
//            the wave's minimum is a DPP reduction.
//   phase 2  the candidates that hold the minimal key -- every symmetry that takes S to M is among them --
//            are processed one at a time by the whole wave (canon_take): the rows are sorted in uniform
//            code, lane l builds cells l and l + 64 of the images of S and P, and the comparison with the
//            best so far is two ballots per half and a bit scan.  Equal images of S count a tie; among
//            those the smaller image of P wins, then the lower k, whatever the order of processing.
//            Where every lane holds at most four survivors they are read from the lanes' slots; where some
//            lane holds more, the exact fallback walks all candidates again with the minimal key known and
//            processes each hit as it is met.  Nothing is capped silently.
//
// Eligibility comes first: status SDK_SOLVED and the 27 units of S each hold 1..9 (a completion keeps
// its givens, so inert or duplicated givens show in S).  An ineligible board's wave writes the identity
// outputs and indexes nothing by a cell value.  Bounds: a board index is below n; a cell index is 0..80 by
// construction (lane, lane + 64 clamped to 80, 9 * r + c with r, c in 0..8, a unit's cells); every shift
// is 4 * (value & 15); the table index is below 36.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "canon_args.h"

namespace sdk {

#define SDK_CANON_FN __host__ __device__ inline

constexpr uint32_t kCanonColumns = 1296;                 // arrangements of the columns
constexpr uint32_t kCanonLines = 18;                     // (t, r0)
constexpr uint32_t kCanonRounds = (kCanonColumns + 63) / 64;
constexpr uint32_t kCanonNoKey = 0xFFFFFFFFu;            // above every key (a key's nibbles are 0..8)
constexpr uint32_t kCanonSlots = 4;                      // survivors a lane keeps (k < 23,328 fits 16 bits)
// synth._P3's six permutations of (0, 1, 2), two bits per entry, six bits per permutation
constexpr uint64_t canon_p3(uint64_t a, uint64_t b, uint64_t c) { return a | b << 2 | c << 4; }
constexpr uint64_t kCanonP3 = canon_p3(0, 1, 2) | canon_p3(0, 2, 1) << 6 | canon_p3(1, 0, 2) << 12 |
                              canon_p3(1, 2, 0) << 18 | canon_p3(2, 0, 1) << 24 | canon_p3(2, 1, 0) << 30;

SDK_CANON_FN uint32_t canon_nib(uint64_t x, uint32_t i) { return (uint32_t)(x >> (4u * (i & 15u))) & 15u; }
SDK_CANON_FN uint32_t canon_perm(uint32_t p, uint32_t m) { return (uint32_t)(kCanonP3 >> (6u * p + 2u * m)) & 3u; }

// cell of S that is G[r][c]: G is S (t = 0) or its transpose
SDK_CANON_FN uint32_t canon_cell(uint32_t t, uint32_t r, uint32_t c) { return t ? 9u * c + r : 9u * r + c; }

// the columns of arrangement q < 1296, nibble j = the column of G that becomes image column j
SDK_CANON_FN uint64_t canon_columns(uint32_t q) {
    const uint32_t s = q / 216u, i0 = q / 36u % 6u, i1 = q / 6u % 6u, i2 = q % 6u;
    uint64_t cc = 0;
#pragma unroll
    for (uint32_t b = 0; b < 3; ++b) {
        const uint32_t ib = b == 0 ? i0 : b == 1 ? i1 : i2;
        const uint32_t stack = 3u * canon_perm(s, b);
#pragma unroll
        for (uint32_t m = 0; m < 3; ++m) cc |= (uint64_t)(stack + canon_perm(ib, m)) << (4u * (3u * b + m));
    }
    return cc;
}

// the inverse of nine packed entries 0..8
SDK_CANON_FN uint64_t canon_inverse(uint64_t cc) {
    uint64_t inv = 0;
#pragma unroll
    for (uint32_t j = 0; j < 9; ++j) inv |= (uint64_t)j << (4u * canon_nib(cc, j));
    return inv;
}

// the band-mates of row r0, ascending
SDK_CANON_FN void canon_mates(uint32_t r0, uint32_t* r1, uint32_t* r2) {
    const uint32_t m = r0 % 3u, base = r0 - m;
    *r1 = base + (m == 0u ? 1u : 0u);
    *r2 = base + (m == 2u ? 1u : 2u);
}

// phase 1's table entry: row r of G in the columns of row r0 (nibble c = the column where row r0 holds
// G[r][c]).  sol: the 81 cells of a valid grid.
SDK_CANON_FN uint64_t canon_row_in_columns(const uint8_t* sol, uint32_t t, uint32_t r0, uint32_t r) {
    uint64_t pos = 0, w = 0;
#pragma unroll
    for (uint32_t c = 0; c < 9; ++c) pos |= (uint64_t)c << (4u * (sol[canon_cell(t, r0, c)] & 15u));
#pragma unroll
    for (uint32_t c = 0; c < 9; ++c) w |= (uint64_t)canon_nib(pos, sol[canon_cell(t, r, c)]) << (4u * c);
    return w;
}

// the key of a candidate: cells 1..8 of row 1 of its image (digits less one), or kCanonNoKey when that
// row does not start with 4.  wa, wb: the table entries of row 0's band-mates.
SDK_CANON_FN uint32_t canon_key(uint64_t wa, uint64_t wb, uint64_t cc, uint64_t inv) {
    const uint32_t c0 = canon_nib(cc, 0);
    const uint32_t fa = canon_nib(inv, canon_nib(wa, c0)), fb = canon_nib(inv, canon_nib(wb, c0));
    const uint64_t w = fa < fb ? wa : wb;
    uint32_t key = 0;
#pragma unroll
    for (uint32_t j = 1; j < 9; ++j) key = key << 4 | canon_nib(inv, canon_nib(w, canon_nib(cc, j)));
    return (fa < fb ? fa : fb) == 3u ? key : kCanonNoKey;
}

// the relabelling of a candidate: nibble v = the image of digit v (nibble 0 stays 0)
SDK_CANON_FN uint64_t canon_relabel(const uint8_t* sol, uint32_t t, uint32_t r0, uint64_t cc) {
    uint64_t rho = 0;
#pragma unroll
    for (uint32_t j = 0; j < 9; ++j)
        rho |= (uint64_t)(j + 1u) << (4u * (sol[canon_cell(t, r0, canon_nib(cc, j))] & 15u));
    return rho;
}

// a band's three rows in ascending order of their first cells (nibbles 3b.. of f), 12 bits; *low = the smallest
SDK_CANON_FN uint32_t canon_sort_band(uint64_t f, uint32_t b, uint32_t* low) {
    const uint32_t x0 = canon_nib(f, 3u * b), x1 = canon_nib(f, 3u * b + 1u), x2 = canon_nib(f, 3u * b + 2u);
    const uint32_t p0 = (x0 > x1) + (x0 > x2), p1 = (x1 > x0) + (x1 > x2), p2 = (x2 > x0) + (x2 > x1);
    const uint32_t m = x0 < x1 ? x0 : x1;
    *low = m < x2 ? m : x2;
    return (3u * b) << (4u * p0) | (3u * b + 1u) << (4u * p1) | (3u * b + 2u) << (4u * p2);
}

// the rows of a candidate: nibble i = the row of G that becomes image row i.  Rows of a band differ in
// column 0, so they compare by their relabelled first cell: row 0's band-mates follow in ascending order of
// it, each other band is sorted the same way, and the band that holds the smaller first cell comes first.
SDK_CANON_FN uint64_t canon_rows(const uint8_t* sol, uint32_t t, uint32_t r0, uint64_t cc, uint64_t rho) {
    const uint32_t c0 = canon_nib(cc, 0);
    uint64_t f = 0;
#pragma unroll
    for (uint32_t r = 0; r < 9; ++r) f |= (uint64_t)canon_nib(rho, sol[canon_cell(t, r, c0)]) << (4u * r);
    uint32_t r1, r2;
    canon_mates(r0, &r1, &r2);
    const bool swap = canon_nib(f, r2) < canon_nib(f, r1);
    const uint32_t b0 = r0 / 3u, ba = b0 == 0u ? 1u : 0u, bb = b0 == 2u ? 1u : 2u;
    uint32_t la, lb;
    const uint64_t sa = canon_sort_band(f, ba, &la), sb = canon_sort_band(f, bb, &lb);
    const uint64_t first = lb < la ? sb : sa, second = lb < la ? sa : sb;
    return (uint64_t)r0 | (uint64_t)(swap ? r2 : r1) << 4 | (uint64_t)(swap ? r1 : r2) << 8 | first << 12 |
           second << 24;
}

#if defined(__HIPCC__)

// the minimum over the wave, in every lane: four rotations inside the rows of 16, then the four rows
__device__ inline uint32_t canon_wave_min(uint32_t x) {
    uint32_t y;
    y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xF, 0xF, false);   // row_ror:1
    x = x < y ? x : y;
    y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xF, 0xF, false);   // row_ror:2
    x = x < y ? x : y;
    y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xF, 0xF, false);   // row_ror:4
    x = x < y ? x : y;
    y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xF, 0xF, false);   // row_ror:8
    x = x < y ? x : y;
    const uint32_t a = __builtin_amdgcn_readlane(x, 0), b = __builtin_amdgcn_readlane(x, 16);
    const uint32_t c = __builtin_amdgcn_readlane(x, 32), d = __builtin_amdgcn_readlane(x, 48);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// -1, 0, 1: the wave's 81 cells (bit l of the first pair: cell l; of the second: cell 64 + l) against the
// best so far, from the ballots of "smaller" and "larger"
__device__ inline int canon_compare(uint64_t lt0, uint64_t gt0, uint64_t lt1, uint64_t gt1) {
    const uint64_t ne0 = lt0 | gt0, ne1 = lt1 | gt1;
    if (ne0) return (lt0 & (ne0 & (0 - ne0))) ? -1 : 1;
    if (ne1) return (lt1 & (ne1 & (0 - ne1))) ? -1 : 1;
    return 0;
}

// what a wave knows of the best candidate so far; the cells are lane l's: l and 64 + l (l < 17)
struct CanonBest {
    uint32_t m0, m1;      // image of S
    uint32_t c0, c1;      // image of P
    uint32_t g0, g1;      // gather
    uint64_t rho;
    uint32_t k, ties;
};

// Phase 2, one candidate (k is wave-uniform): its images against the best.  s_sol: a valid grid.
__device__ inline void canon_take(const uint8_t* s_sol, const uint8_t* s_puz, uint32_t k, uint32_t lane, CanonBest& b) {
    const uint32_t t = k / (9u * kCanonColumns), r0 = k / kCanonColumns % 9u, q = k % kCanonColumns;
    const uint64_t cc = canon_columns(q);
    const uint64_t rho = canon_relabel(s_sol, t, r0, cc);
    const uint64_t rr = canon_rows(s_sol, t, r0, cc, rho);
    const bool has1 = lane < 17u;
    const uint32_t cell1 = has1 ? lane + 64u : 80u;
    // (on a valid grid the rows are 0..8 and so is every cell below 81; the clamp holds for any bytes)
    const uint32_t g0 = min(canon_cell(t, canon_nib(rr, lane / 9u), canon_nib(cc, lane % 9u)), 80u);
    const uint32_t g1 = min(canon_cell(t, canon_nib(rr, cell1 / 9u), canon_nib(cc, cell1 % 9u)), 80u);
    const uint32_t m0 = canon_nib(rho, s_sol[g0]), m1 = canon_nib(rho, s_sol[g1]);
    const uint32_t c0 = canon_nib(rho, s_puz[g0]), c1 = canon_nib(rho, s_puz[g1]);
    const int cm = canon_compare(__ballot(m0 < b.m0), __ballot(m0 > b.m0), __ballot(has1 && m1 < b.m1),
                                 __ballot(has1 && m1 > b.m1));
    if (cm > 0) return;
    bool take = true;
    if (cm == 0) {
        const int cp = canon_compare(__ballot(c0 < b.c0), __ballot(c0 > b.c0), __ballot(has1 && c1 < b.c1),
                                     __ballot(has1 && c1 > b.c1));
        take = cp < 0 || (cp == 0 && k < b.k);
        b.ties += 1u;
    } else {
        b.m0 = m0, b.m1 = m1, b.ties = 1u;
    }
    if (take) b.c0 = c0, b.c1 = c1, b.g0 = g0, b.g1 = g1, b.rho = rho, b.k = k;
}

__global__ __launch_bounds__(64) void canon_kernel(const CanonArgs a) {
    __shared__ uint8_t s_sol[96], s_puz[96];
    __shared__ uint64_t s_w[2u * kCanonLines];
    const uint32_t lane = threadIdx.x;
    const bool has1 = lane < 17u;
    const uint32_t cell1 = has1 ? lane + 64u : 80u;
    // the unit of lanes 0..26: nine rows, nine columns, nine boxes
    const uint32_t u = lane < 27u ? lane : 26u, v = u % 9u;
    const uint32_t ubase = u < 9u ? 9u * v : u < 18u ? v : 27u * (v / 3u) + 3u * (v % 3u);
    for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const uint8_t* in = a.in + i * 81u;
        const uint32_t p0 = in[lane], p1 = in[cell1];
        const uint32_t s0 = a.sol[i * 81u + lane], s1 = a.sol[i * 81u + cell1];
        const int st = a.status[i];
        __syncthreads();         // the board before: its last reads
        s_sol[lane] = (uint8_t)s0, s_puz[lane] = (uint8_t)p0;
        if (has1) s_sol[cell1] = (uint8_t)s1, s_puz[cell1] = (uint8_t)p1;
        __syncthreads();
        // eligibility: exactly one completion, and it is a valid grid
        uint32_t seen = 0;
#pragma unroll
        for (uint32_t j = 0; j < 9; ++j) {
            const uint32_t c = u < 9u ? j : u < 18u ? 9u * j : 9u * (j / 3u) + j % 3u;
            const uint32_t d = s_sol[ubase + c];
            seen |= d <= 9u ? 1u << d : 1u;
        }
        const bool eligible = st == 1 && __ballot(lane < 27u && seen != 0x3FEu) == 0;
        uint8_t* canon = a.canon + i * 81u;
        if (!eligible) {
            canon[lane] = (uint8_t)p0;
            if (has1) canon[cell1] = (uint8_t)p1;
            if (a.gather) {
                a.gather[i * 81u + lane] = (uint8_t)lane;
                if (has1) a.gather[i * 81u + cell1] = (uint8_t)cell1;
            }
            if (a.relabel && lane < 10u) a.relabel[i * 10u + lane] = (uint8_t)lane;
            if (a.ties && lane == 0u) a.ties[i] = 0;
            continue;
        }
        // the tables: lane 2 * line + e holds band-mate e of row r0 in the columns of row r0
        {
            const uint32_t e = lane < 2u * kCanonLines ? lane : 0u, line = e >> 1, t = line / 9u, r0 = line % 9u;
            uint32_t r1, r2;
            canon_mates(r0, &r1, &r2);
            const uint64_t w = canon_row_in_columns(s_sol, t, r0, (e & 1u) ? r2 : r1);
            if (lane < 2u * kCanonLines) s_w[e] = w;
        }
        __syncthreads();
        // phase 1: the smallest key of the lane's candidates, one candidate that has it, how many have it
        // (the candidates are a shift register of 16-bit indices: the last kCanonSlots that have the key)
        uint32_t best = kCanonNoKey, count = 0;
        uint64_t slots = 0;
#pragma unroll 1
        for (uint32_t m = 0; m < kCanonRounds; ++m) {
            const uint32_t q = 64u * m + lane;
            const bool valid = q < kCanonColumns;
            const uint64_t cc = canon_columns(valid ? q : 0u), inv = canon_inverse(cc);
#pragma unroll 2
            for (uint32_t line = 0; line < kCanonLines; ++line) {
                const uint32_t key = valid ? canon_key(s_w[2u * line], s_w[2u * line + 1u], cc, inv) : kCanonNoKey;
                const uint64_t k = line * kCanonColumns + q;
                count = key < best ? 1u : count + (key == best ? 1u : 0u);
                slots = key < best ? k : key == best ? slots << 16 | k : slots;
                best = key < best ? key : best;
            }
        }
        const uint32_t low = canon_wave_min(best);     // below kCanonNoKey: M's own candidate has a key
        const bool win = best == low;
        CanonBest b;
        b.m0 = b.m1 = b.c0 = b.c1 = 0xFFu, b.g0 = b.g1 = 0u, b.rho = 0u, b.k = 0u, b.ties = 0u;
        if (__ballot(win && count > kCanonSlots) == 0) {
            // every lane's survivors are in its slots
#pragma unroll
            for (uint32_t j = 0; j < kCanonSlots; ++j) {
                const uint32_t kj = (uint32_t)(slots >> (16u * j)) & 0xFFFFu;
                for (uint64_t left = __ballot(win && count > j); left; left &= left - 1u) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(left);
                    canon_take(s_sol, s_puz, (uint32_t)__builtin_amdgcn_readlane((int)kj, (int)l), lane, b);
                }
            }
        } else {
            // the exact fallback: every candidate again, the hits processed as they are met
#pragma unroll 1
            for (uint32_t m = 0; m < kCanonRounds; ++m) {
                const uint32_t q = 64u * m + lane;
                const bool valid = q < kCanonColumns;
                const uint64_t cc = canon_columns(valid ? q : 0u), inv = canon_inverse(cc);
#pragma unroll 1
                for (uint32_t line = 0; line < kCanonLines; ++line) {
                    const uint32_t key = valid ? canon_key(s_w[2u * line], s_w[2u * line + 1u], cc, inv) : kCanonNoKey;
                    for (uint64_t left = __ballot(key == low); left; left &= left - 1u)
                        canon_take(s_sol, s_puz, line * kCanonColumns + 64u * m + (uint32_t)__builtin_ctzll(left), lane, b);
                }
            }
        }
        canon[lane] = (uint8_t)b.c0;
        if (has1) canon[cell1] = (uint8_t)b.c1;
        if (a.solution) {
            a.solution[i * 81u + lane] = (uint8_t)b.m0;
            if (has1) a.solution[i * 81u + cell1] = (uint8_t)b.m1;
        }
        if (a.gather) {
            a.gather[i * 81u + lane] = (uint8_t)b.g0;
            if (has1) a.gather[i * 81u + cell1] = (uint8_t)b.g1;
        }
        if (a.relabel && lane < 10u) a.relabel[i * 10u + lane] = (uint8_t)canon_nib(b.rho, lane);
        if (a.ties && lane == 0u) a.ties[i] = (uint16_t)b.ties;
    }
}

#endif  // __HIPCC__

}  // namespace sdk
