// subsets_kernel.h -- the subsets stage: how many cells does a search-level board keep open once naked
// and hidden pairs, triples and quads join the three techniques?  (sdk_subsets_batch; include/sudoku_hip.h
// has the contract, DESIGN.md "Subsets" the measurements)
//
// A board of level SDK_GRADE_SEARCH has exactly one completion and clean givens.  F_4 is the fixpoint of
// R4 = R3 + {naked and hidden S_2, S_3, S_4} on its candidate sets; the output is the number of open
// cells of F_4.  Every rule only removes candidates and never a digit of the completion, and a premise
// that holds keeps holding after further removals, so F_4 is one state whatever the order: the kernel
// starts from the input row and applies, per round, every rule to one snapshot.
//
// Not bit-sliced: a subset search is per unit.  One board per 32-lane half, 81 candidate words per
// board in LDS, lanes 0..26 of a half own one unit each (9 rows, 9 columns, 9 boxes).  A round, per lane:
//   1  read the unit's nine masks (cell -> digits) and form the transpose (digit -> positions);
//   2  on each of the two 9 x 9 bit matrices run ONE primitive (subsets_device.h, shared with the fish
//      stage: s4_singles, then s4_subset over the table): rows
//      with one bit (a closed cell; a digit with one place) clear that bit from the other rows -- N and
//      H -- and for every subset of 2..4 of the other rows whose union has at most as many bits as the
//      subset has rows, the union goes from the rows outside it.  The 246 subsets come from a table in
//      constant memory (three select masks for the packed rows and the size: scalar loads, the loop
//      counter is uniform); the nine rows are packed three to a register at a stride of 10 bits, so a
//      union is three AND-ORs and a fold, and a subset that fires is applied to all nine rows by SWAR
//      arithmetic (a row that is not inside the union loses it: on a state that holds a completion
//      the rows inside a tight union are exactly the subset's).  Nothing is indexed dynamically;
//   3  locked candidates from the position masks: a digit whose positions lie in one third of the
//      unit (a line's box segment; a box's row or column) goes from the rest of the crossing unit;
//   4  all removals go to LDS by atomic AND: the rules only remove, so the order cannot matter.
// A heavy round (with the 246 subsets) runs only when the light rules (singles and locked candidates)
// changed nothing on some unfinished board; a board is finished when a heavy round changes nothing
// on it.  Change is seen by the row lanes at the next round's read (every cell lies in a row).
// `heavy` is one flag per wave: a board still moving under the light rules walks the subsets too when
// its wave-mate stalls (a heavy round applies every rule, so the result cannot differ), and a finished
// or idle half keeps executing, without effect, until the other half ends.
//
// Termination: a round that changes a board removes at least one of its 729 candidates, and an
// unchanged light round is followed by a heavy one, an unchanged heavy one ends the board: at most
// 2 * 729 + 2 rounds.  kS4MaxRounds is the guard above that; a board that reached it would report the
// open count it has.  Bounds: a wave that dequeues at or past the list's length exits, an entry past
// it idles its half, every list entry is checked against n, every LDS index is a cell 0..80.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "subsets_args.h"
#include "subsets_device.h"

namespace sdk {

constexpr uint32_t kS4MaxRounds = 1536;                          // above 2 * 729 + 2 (see above)

__global__ __launch_bounds__(64) void subsets32_kernel(Subsets32Args a) {
    __shared__ uint32_t s_c[2][kS4LdsWords];
    const uint32_t t = threadIdx.x, hl = t & 31u, half = t >> 5;
    uint32_t* const c = s_c[half];
    // the lane's unit: cell(q) = base + (q / 3) sa + (q % 3) sb; the cells that lose what is confined to
    // third s of the unit, by rows (A) and -- a box's columns -- by position in the row (B):
    // tb + s ts + o[i] + k tt, i < 2, k < 3
    const bool lane_unit = hl < 27u;
    const uint32_t u = lane_unit ? hl : 0u, kind = u / 9u, v = u % 9u, v3 = v / 3u, vr = v % 3u;
    const uint32_t n1 = (vr + 1u) % 3u, n2 = (vr + 2u) % 3u, m1 = (v3 + 1u) % 3u, m2 = (v3 + 2u) % 3u;
    uint32_t base, sa, sb, tbA, tsA, ttA, oA0, oA1;
    if (kind == 0u) {            // row v: the rest of the box of each of its three segments
        base = 9u * v, sa = 3u, sb = 1u;
        tbA = 0u, tsA = 3u, ttA = 1u, oA0 = 9u * (3u * v3 + n1), oA1 = 9u * (3u * v3 + n2);
    } else if (kind == 1u) {     // column v
        base = v, sa = 27u, sb = 9u;
        tbA = 0u, tsA = 27u, ttA = 9u, oA0 = 3u * v3 + n1, oA1 = 3u * v3 + n2;
    } else {                     // box v = (band v3, stack vr): the rest of each of its rows ...
        base = 27u * v3 + 3u * vr, sa = 9u, sb = 1u;
        tbA = 27u * v3, tsA = 9u, ttA = 1u, oA0 = 3u * n1, oA1 = 3u * n2;
    }
    // ... and of each of its columns
    const uint32_t tbB = 3u * vr, oB0 = 27u * m1, oB1 = 27u * m2;
    const uint32_t m = a.list[0];
    for (;;) {
        uint32_t i = 0;
        if (t == 0) i = atomicAdd(a.next, 2u);
        i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
        if (i >= m) break;
        // entry i + half: a board of level 4, or the half idles
        bool work = i + half < m;
        uint32_t j = work ? a.list[1u + i + half] : 0u;
        work = work && j < a.n;
        j = work ? j : 0u;
        work = work && a.level[j] == 4u;
        const uint64_t wb = __ballot(work);
        const uint32_t valid = (wb & 0xFFFFFFFFull ? 1u : 0u) | (wb >> 32 ? 2u : 0u);
        if (valid == 0u) continue;
        __syncthreads();         // the round before: its last reads
        if (lane_unit) {
            const uint32_t c0 = 3u * hl;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t g = work ? a.in[(uint64_t)j * 81u + c0 + k] : 1u;
                c[c0 + k] = (g >= 1u && g <= 9u) ? 1u << (g - 1u) : kS4All;
            }
        }
        __syncthreads();
        const bool act = lane_unit && work;
        uint32_t prev[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        uint32_t done = ~valid & 3u, round = 0u;
        bool heavy = false;
        for (;;) {
            uint32_t r[9], p[9];
            bool diff = false;
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const uint32_t x = c[base + (q / 3) * sa + (q % 3) * sb];
                diff = diff || x != prev[q];
                prev[q] = x;
                r[q] = act ? x : kS4All;
            }
            const uint64_t db = __ballot(diff && act);
            const uint32_t chg = round == 0u ? 3u : (db & 0xFFFFFFFFull ? 1u : 0u) | (db >> 32 ? 2u : 0u);
            if (heavy) done |= ~chg & 3u;                // unchanged by a heavy round: F_4
            if (done == 3u || ++round >= kS4MaxRounds) break;
            heavy = (~done & ~chg & 3u) != 0u;           // the light rules are spent on some board
            __syncthreads();                             // every lane has read this round's snapshot
#pragma unroll
            for (int d = 0; d < 9; ++d) {
                uint32_t x = 0u;
#pragma unroll
                for (int q = 0; q < 9; ++q) x |= (r[q] >> d & 1u) << q;
                p[d] = x;
            }
            uint32_t rn[9], rh[9], T;
            s4_matrices(r, p, heavy, rn, rh, T);
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                uint32_t lose = rn[q];
#pragma unroll
                for (int d = 0; d < 9; ++d) lose |= (rh[d] >> q & 1u) << d;
                if (lose & r[q] & (act ? kS4All : 0u)) atomicAnd(&c[base + (q / 3) * sa + (q % 3) * sb], ~lose);
            }
            // locked candidates; a digit closed in the unit is N's, in the crossing unit's own lane
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const uint32_t conf = act ? s4_confined(p, 7u << (3 * s)) & ~T : 0u;
                if (conf) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        atomicAnd(&c[tbA + s * tsA + oA0 + k * ttA], ~conf);
                        atomicAnd(&c[tbA + s * tsA + oA1 + k * ttA], ~conf);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const uint32_t conf = (act && kind == 2u) ? s4_confined(p, 0x49u << s) & ~T : 0u;
                if (conf) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        atomicAnd(&c[tbB + s + oB0 + 9 * k], ~conf);
                        atomicAnd(&c[tbB + s + oB1 + 9 * k], ~conf);
                    }
                }
            }
            __syncthreads();                             // the removals are in before the next read
        }
        // the open cells of each half's final state
        uint32_t opn = 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t cell = hl + 32u * k;
            const bool o = cell < 81u && __popc(c[cell < 81u ? cell : 0u]) != 1;
            const uint64_t ob = __ballot(o);
            opn += (uint32_t)__popc((uint32_t)(half ? ob >> 32 : ob));
        }
        if (hl == 0u && work) a.open4[j] = (uint8_t)opn;
    }
}

}  // namespace sdk
