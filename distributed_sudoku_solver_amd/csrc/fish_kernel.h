// fish_kernel.h -- the fish stage: how many cells does a search-level board keep open once X-wings,
// swordfish and jellyfish join the subsets?  (sdk_fish_batch; include/sudoku_hip.h has the contract,
// DESIGN.md "Fish" the measurements)
//
// For a digit d, M_d is the 9 x 9 bit matrix whose row r holds the columns at which cell (r, c) still has
// candidate d, closed cells included.  A row fish of size k is k rows of M_d whose union has at most k
// columns: the other rows lose those columns.  A column fish is the same on the transpose.  That is the
// subsets stage's primitive (subsets_device.h) on a third kind of slice of the candidate cube.
// R5 = R4 + {row and column fish of sizes 2..4, every digit}; F_5 is its fixpoint.  A fish removes no digit
// of a completion (Hall's condition on the digit's places) and its premise survives further removals, so
// F_5 is one state whatever the order.  One stage gives both counts: open4, the open cells of F_4 exactly as
// subsets32_kernel reports them, and open5, the open cells of F_5.
//
// The layout is the subsets stage's: one board per 32-lane half, 81 candidate words per board in LDS,
// lanes 0..26 of a half own one unit each; a dequeue takes two list entries.  Rounds come in three tiers:
//   light  singles and locked candidates                                    (subsets_kernel.h, steps 1..4)
//   heavy  the light rules and the 246 subsets on every unit's two matrices (the same, with the table)
//   deep   fish only: lanes 0..8 of a half take one digit each, d = lane.  A lane reads the board's 81
//          words (the nine lanes of a half read one address at a time: a broadcast), forms M_d and its
//          transpose in registers, runs s4_matrices(..., heavy = true, ...) on the pair -- rows with one bit
//          are the k = 1 fish, a line's hidden single followed by N -- and clears bit d of the losing cells
//          by atomic AND.  Nothing is indexed dynamically, there are no private arrays.
// Every half has a tier of its own, the tier it needs next: a round that changed it sends it back to
// light; one that left it unchanged sends it one tier up -- light to heavy, heavy to deep (that state is
// F_4: open4 is counted and stored there, once), deep to finished (F_5).  The round's kind is one value per
// wave: deep if every unfinished half needs deep, else heavy if some unfinished half needs heavy, else
// light.  A heavy round serves a half that needs light (it applies every light rule), and an unchanged
// heavy round is F_4 for it too.  A half that needs deep while its wave-mate does not waits: the light and
// heavy rules run on it without effect, since it is a fixpoint of R4, and it keeps its tier.  So a deep
// round only ever runs when every unfinished half of the wave has stored open4: no fish removal touches a
// board before its open4 is taken, whatever its wave-mate is doing.  A finished or idle half keeps
// executing, without effect, until the other half ends.  Change is seen by the row lanes at the next
// round's read (every cell lies in a row), which every round does, deep ones included.
//
// Termination: a round that changes a board removes at least one of its 729 candidates and each unchanged
// tier escalates once: at most 3 * 729 + 3 rounds for a board alone.  In a wave, a round that changes
// neither half raises the round's kind (after light every unfinished half needs heavy or deep, after heavy
// deep, after deep none is left), so at most three such rounds follow a changing one, of which there are at
// most 2 * 729: 4 * 1458 + 3 rounds.  kF5MaxRounds is the guard above that; a board that reached it
// would report the open counts it has.  Bounds as in the subsets kernel: a wave that dequeues at or past the
// list's length exits, an entry past it idles its half, every list entry is checked against n, every LDS
// index is a cell 0..80 of the half's own words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fish_args.h"
#include "subsets_device.h"

namespace sdk {

constexpr uint32_t kF5MaxRounds = 6144;      // above 4 * 1458 + 3 (see above)
constexpr uint32_t kF5Light = 0u, kF5Heavy = 1u, kF5Deep = 2u;

// The open cells of each half's board (every lane of the wave calls it; a lane gets its own half's count).
__device__ __forceinline__ uint32_t f5_open_cells(const uint32_t* c, uint32_t hl, uint32_t half) {
    uint32_t opn = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t cell = hl + 32u * k;
        const bool o = cell < 81u && __popc(c[cell < 81u ? cell : 0u]) != 1;
        const uint64_t ob = __ballot(o);
        opn += (uint32_t)__popc((uint32_t)(half ? ob >> 32 : ob));
    }
    return opn;
}

__global__ __launch_bounds__(64) void fish32_kernel(Fish32Args a) {
    __shared__ uint32_t s_c[2][kS4LdsWords];
    const uint32_t t = threadIdx.x, hl = t & 31u, half = t >> 5;
    uint32_t* const c = s_c[half];
    // the lane's unit, as in subsets32_kernel: cell(q) = base + (q / 3) sa + (q % 3) sb; the cells that
    // lose what is confined to third s of the unit, by rows (A) and -- a box's columns -- by position in
    // the row (B): tb + s ts + o[i] + k tt, i < 2, k < 3
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
    const bool lane_digit = hl < 9u;             // a deep round: digit hl of the half's board
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
        // per half, one bit each: finished; needs heavy; needs deep; open4 stored
        uint32_t done = ~valid & 3u, t1 = 0u, t2 = 0u, rec = 0u, round = 0u;
        uint32_t mode = kF5Light;                        // the kind of the round before
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
            const uint32_t still = ~chg & ~done & 3u;    // unfinished halves the round before left as they were
            if (mode == kF5Deep) {
                done |= still;                           // unchanged by a deep round: F_5
            } else if (mode == kF5Heavy) {
                if (still & ~rec) {                      // unchanged by a heavy round: F_4, for the first time
                    const uint32_t opn = f5_open_cells(c, hl, half);
                    if (hl == 0u && work && ((still & ~rec) >> half & 1u)) a.open4[j] = (uint8_t)opn;
                }
                rec |= still;
                t2 |= still;
            } else {
                t1 |= still & ~t2;                       // the light rules are spent (a half that waits keeps its tier)
            }
            t1 &= ~(chg | t2);
            t2 &= ~chg;                                  // a changed half starts from the light rules again
            if (done == 3u || ++round >= kF5MaxRounds) break;
            const uint32_t live = ~done & 3u;
            mode = (t2 & live) == live ? kF5Deep : (t1 & live) ? kF5Heavy : kF5Light;
            __syncthreads();                             // every lane has read this round's snapshot
            if (mode == kF5Deep) {
                // every unfinished half is at F_4 with open4 stored; lane d < 9 of such a half takes digit d
                const bool fl = lane_digit && work && (live >> half & 1u);
                uint32_t mr[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, mc[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
                for (int y = 0; y < 9; ++y) {
#pragma unroll
                    for (int x = 0; x < 9; ++x) {
                        const uint32_t b = c[9 * y + x] >> hl & 1u;
                        mr[y] |= b << x;
                        mc[x] |= b << y;
                    }
                }
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    mr[q] = fl ? mr[q] : kS4All;
                    mc[q] = fl ? mc[q] : kS4All;
                }
                uint32_t fr[9], fc[9], T;
                s4_matrices(mr, mc, true, fr, fc, T);
#pragma unroll
                for (int y = 0; y < 9; ++y) {
                    uint32_t lose = fr[y];
#pragma unroll
                    for (int x = 0; x < 9; ++x) lose |= (fc[x] >> y & 1u) << x;
                    lose &= fl ? mr[y] : 0u;
                    if (lose) {
#pragma unroll
                        for (int x = 0; x < 9; ++x)
                            if (lose >> x & 1u) atomicAnd(&c[9 * y + x], ~(1u << hl));
                    }
                }
                __syncthreads();                         // the removals are in before the next read
                continue;
            }
            const bool heavy = mode == kF5Heavy;
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
        // the open cells of each half's final state; a board the guard stopped before F_4 reports it twice
        const uint32_t opn = f5_open_cells(c, hl, half);
        if (hl == 0u && work) {
            a.open5[j] = (uint8_t)opn;
            if (!(rec >> half & 1u)) a.open4[j] = (uint8_t)opn;
        }
    }
}

}  // namespace sdk
