// chains_kernel.h -- the chains stage: how many cells does a search-level board keep open once X-chains and
// XY-chains join the wings and simple colouring?  (sdk_chains_batch; include/sudoku_hip.h has the contract,
// DESIGN.md "Chains" the measurements)
//
// R7 = R6 + {X, Y} on the grader's candidate sets; F_7 is its fixpoint.
//   X (X-chains, one digit d at a time).  The places of d are the cells that hold candidate d, closed cells
//     included, as in M_d of the fish and the colouring's places.  A link is a unit with exactly two places.
//     For every open place s: ON starts as the other ends of the links through s; until ON stops growing, OFF
//     is the places that share a unit with a cell of ON, and every link with exactly one end in OFF puts its
//     other end into ON (s itself never).  For every t in ON either s or t holds d, so every open cell that
//     shares a unit with s and with t loses d.
//   Y (XY-chains).  For every bivalue cell s and each of its two digits z: a state (c, v) means "c is v", the
//     start state is (s, the other digit of s), and from (c, v) the chain goes to every bivalue cell c2 != s
//     that shares a unit with c and holds v, in the state (c2, the other digit of c2).  For every reached
//     state (c, z) with c != s either s or c holds z, so every open cell that shares a unit with s and with c
//     loses z.
// Both remove no digit of a completion.  A premise that further removals break becomes a single (a bivalue
// cell closes, a link's surviving end is a hidden single), so F_7 is one state whatever the order; the order
// here is an X + Y pass from F_6, then F_6 again, until a pass changes nothing (tests/chains_model.py, "f6").
// One stage gives four counts: open4, open5 and open6 exactly as wing32_kernel reports them, and open7.
//
// The frame is the wings stage's (wings_kernel.h), step for step: one board per 32-lane half, 81 candidate
// words per board in LDS and a snapshot copy of them, lanes 0..26 of a half own one unit each, a dequeue takes
// two list entries, one-wave workgroups, and the light, heavy, deep and wide tiers.  A fifth tier follows:
//   chain  X- and XY-chains, both from one snapshot, taken as a wide round takes it; all reads go to that
//          copy, all removals by atomic AND to the live words.
//          Masks: lane 9 b + v (< 27) of a half scans band b of the snapshot for the bivalue cells that have
//          digit v as their lower and as their higher digit, and stores the two 27-bit words in LDS
//          (kC7MaskWords per half).
//          X-chains: the same lane takes digit v and the start places of band b.  It reads the 81 snapshot
//          words (one address at a time across the wave: a broadcast) into the digit's places and the board's
//          open cells, three band words each; the 27 unit masks are constants of the unrolled code.
//          XY-chains: a task is (bivalue cell, one of its digits), strided over the half's 32 lanes.  The state
//          set is two cell sets, "set to its lower digit" and "set to its higher digit"; a step takes one
//          reached state, reads its digit's two masks from LDS and adds the peers they name.
//          Nothing in registers is indexed dynamically, there are no private arrays.
// A half that a wide round leaves unchanged is at F_6: open6 is counted and stored there, once, and the half
// needs chain.  The round's kind is one value per wave: chain if every unfinished half needs chain, else wide
// if every unfinished half needs wide or chain, else deep if every unfinished half needs deep, wide or chain,
// else heavy if some unfinished half needs heavy, else light.  A half that needs chain while its wave-mate
// does not waits, as halves wait at deep and at wide: the rounds that run meanwhile have no effect on it,
// since it is a fixpoint of R6, and it keeps its tier.  So a chain round only ever runs when every unfinished
// half of the wave has stored open4, open5 and open6: no chain removal touches a board before the three are
// taken, whatever its wave-mate is doing.  A half that a chain round leaves unchanged is finished (F_7); a
// changed half goes back to light.
// A finished or idle half keeps executing, without effect, until the other half ends: the light and heavy
// rounds apply their rules to every half with a board (`act`), finished ones included, and leave a finished
// half as it is because F_7 is a fixpoint of R5; the deep, the wide and the chain rounds skip it (`live`).
//
// Termination: a round that changes a board removes at least one of its 729 candidates, so a wave has at
// most 2 * 729 changing rounds.  A round that changes neither half raises the round's kind, so at most five
// such rounds follow a changing one: 6 * 1458 + 5 = 8753 rounds.  kF7MaxRounds is the guard above that; a
// board that reached it would report the open counts it has.  Inside a chain round, ON grows inside the
// digit's places and a sweep that adds nothing ends the closure; an XY state is followed once.  Bounds as in
// the wings kernel: a wave that dequeues at or past the list's length exits, an entry past it idles its half,
// every list entry is checked against n, and every LDS index is a cell 0..80 of the half's own words -- a peer
// of a cell below 81 (w6_peer), or a bit below 27 of a band word plus 27 times the band -- or a mask word
// below kC7MaskWords of the half's own masks (c7_mask clamps its digit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chains_args.h"
#include "chains_device.h"
#include "subsets_device.h"
#include "wings_device.h"

namespace sdk {

constexpr uint32_t kF7MaxRounds = 16384;     // above 6 * 1458 + 5 (see above)
constexpr uint32_t kC7Light = 0u, kC7Heavy = 1u, kC7Deep = 2u, kC7Wide = 3u, kC7Chain = 4u;

__global__ __launch_bounds__(64) void chain32_kernel(Chains32Args a) {
    __shared__ uint32_t s_c[2][kS4LdsWords];     // the candidate words
    __shared__ uint32_t s_s[2][kS4LdsWords];     // a wide or a chain round's snapshot of them
    __shared__ uint32_t s_m[2][kC7MaskWords];    // a chain round's bivalue masks
    const uint32_t t = threadIdx.x, hl = t & 31u, half = t >> 5;
    uint32_t* const c = s_c[half];
    uint32_t* const s = s_s[half];
    uint32_t* const bm = s_m[half];
    // the lane's unit and the cells its locked candidates clear, as in fish32_kernel
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
    const bool lane_digit = hl < 9u;             // a deep or a wide round: digit hl of the half's board
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
        // per half, one bit each: finished; needs heavy; needs deep; needs wide; needs chain; open4 stored;
        // open5 stored; open6 stored
        uint32_t done = ~valid & 3u, t1 = 0u, t2 = 0u, t3 = 0u, t4 = 0u, rec = 0u, rec5 = 0u, rec6 = 0u, round = 0u;
        uint32_t mode = kC7Light;                        // the kind of the round before
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
            if (mode == kC7Chain) {
                done |= still;                           // unchanged by a chain round: F_7
            } else if (mode == kC7Wide) {
                if (still & ~rec6) {                     // unchanged by a wide round: F_6, for the first time
                    const uint32_t opn = w6_open_cells(c, hl, half);
                    if (hl == 0u && work && ((still & ~rec6) >> half & 1u)) a.open6[j] = (uint8_t)opn;
                }
                rec6 |= still;
                t4 |= still;
            } else if (mode == kC7Deep) {
                if (still & ~rec5) {                     // unchanged by a deep round: F_5, for the first time
                    const uint32_t opn = w6_open_cells(c, hl, half);
                    if (hl == 0u && work && ((still & ~rec5) >> half & 1u)) a.open5[j] = (uint8_t)opn;
                }
                rec5 |= still;
                t3 |= still & ~t4;
            } else if (mode == kC7Heavy) {
                if (still & ~rec) {                      // unchanged by a heavy round: F_4, for the first time
                    const uint32_t opn = w6_open_cells(c, hl, half);
                    if (hl == 0u && work && ((still & ~rec) >> half & 1u)) a.open4[j] = (uint8_t)opn;
                }
                rec |= still;
                t2 |= still & ~(t3 | t4);
            } else {
                t1 |= still & ~(t2 | t3 | t4);           // the light rules are spent (a half that waits keeps its tier)
            }
            t1 &= ~(chg | t2 | t3 | t4);
            t2 &= ~(chg | t3 | t4);
            t3 &= ~(chg | t4);
            t4 &= ~chg;                                  // a changed half starts from the light rules again
            if (done == 3u || ++round >= kF7MaxRounds) break;
            const uint32_t live = ~done & 3u;
            mode = (t4 & live) == live                  ? kC7Chain
                   : ((t3 | t4) & live) == live        ? kC7Wide
                   : ((t2 | t3 | t4) & live) == live   ? kC7Deep
                   : (t1 & live)                       ? kC7Heavy
                                                       : kC7Light;
            __syncthreads();                             // every lane has read this round's snapshot
            if (mode == kC7Chain) {
                // every unfinished half is at F_6 with open4, open5 and open6 stored
                const bool wl = work && (live >> half & 1u);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t cell = hl + 32u * k;
                    if (cell < 81u) s[cell] = c[cell];
                }
                __syncthreads();
                // lane 9 b + d: digit d, band b.  The digit's places, the open cells, the band's bivalue masks
                // The lane index goes through a register the compiler cannot see into: without this everything
                // the round derives from it alone (d, part, their shifts and compares) is hoisted out of the
                // round loop and stays live across the light and heavy rounds, some 10 registers.
                uint32_t h2 = hl;
                asm volatile("" : "+v"(h2));
                const uint32_t d = h2 % 9u, part = h2 / 9u;
                W6Set places{0u, 0u, 0u}, open{0u, 0u, 0u};
                uint32_t blo = 0u, bhi = 0u;
#pragma unroll 9
                for (int x = 0; x < 27; ++x) {
                    const uint32_t w0 = s[x], w1 = s[27 + x], w2 = s[54 + x];
                    places.a |= (w0 >> d & 1u) << x;
                    places.b |= (w1 >> d & 1u) << x;
                    places.c |= (w2 >> d & 1u) << x;
                    open.a |= (__popc(w0) != 1 ? 1u : 0u) << x;
                    open.b |= (__popc(w1) != 1 ? 1u : 0u) << x;
                    open.c |= (__popc(w2) != 1 ? 1u : 0u) << x;
                    const uint32_t w = part == 0u ? w0 : part == 1u ? w1 : w2;
                    const bool biv = __popc(w) == 2 && (w >> d & 1u);
                    const bool low = (w & ((1u << d) - 1u)) == 0u;
                    blo |= (biv && low ? 1u : 0u) << x;
                    bhi |= (biv && !low ? 1u : 0u) << x;
                }
                if (lane_unit) {
                    bm[3u * (2u * d) + part] = blo;
                    bm[3u * (2u * d + 1u) + part] = bhi;
                }
                __syncthreads();
                if (!(lane_unit && wl)) places = W6Set{0u, 0u, 0u};
                const W6Set lose = c7_xchains(places, open, part);
                c7_clear(s, c, lose.a, 0u, 1u << d);
                c7_clear(s, c, lose.b, 27u, 1u << d);
                c7_clear(s, c, lose.c, 54u, 1u << d);
                c7_xychains(s, c, bm, h2, wl);
                __syncthreads();                         // the removals are in before the next read
                continue;
            }
            if (mode == kC7Wide) {
                // every unfinished half is at F_5 with open4 and open5 stored
                const bool wl = work && (live >> half & 1u);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t cell = hl + 32u * k;
                    if (cell < 81u) s[cell] = c[cell];
                }
                __syncthreads();
#pragma nounroll
                for (uint32_t k = 0; k < 3u; ++k) {
                    const uint32_t cell = hl + 32u * k;
                    c7_wings(s, c, cell < 81u ? cell : 0u, wl && cell < 81u);
                }
                const bool cl = lane_digit && wl;
                W6Set places{0u, 0u, 0u};
#pragma unroll 9
                for (int x = 0; x < 27; ++x) {
                    places.a |= (s[x] >> hl & 1u) << x;
                    places.b |= (s[27 + x] >> hl & 1u) << x;
                    places.c |= (s[54 + x] >> hl & 1u) << x;
                }
                if (!cl) places = W6Set{0u, 0u, 0u};
                const W6Set lose = w6_colour(places);
                c7_clear(s, c, lose.a, 0u, 1u << hl);
                c7_clear(s, c, lose.b, 27u, 1u << hl);
                c7_clear(s, c, lose.c, 54u, 1u << hl);
                __syncthreads();                         // the removals are in before the next read
                continue;
            }
            if (mode == kC7Deep) {
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
            const bool heavy = mode == kC7Heavy;
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
            for (int s3 = 0; s3 < 3; ++s3) {
                const uint32_t conf = act ? s4_confined(p, 7u << (3 * s3)) & ~T : 0u;
                if (conf) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        atomicAnd(&c[tbA + s3 * tsA + oA0 + k * ttA], ~conf);
                        atomicAnd(&c[tbA + s3 * tsA + oA1 + k * ttA], ~conf);
                    }
                }
            }
#pragma unroll
            for (int s3 = 0; s3 < 3; ++s3) {
                const uint32_t conf = (act && kind == 2u) ? s4_confined(p, 0x49u << s3) & ~T : 0u;
                if (conf) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        atomicAnd(&c[tbB + s3 + oB0 + 9 * k], ~conf);
                        atomicAnd(&c[tbB + s3 + oB1 + 9 * k], ~conf);
                    }
                }
            }
            __syncthreads();                             // the removals are in before the next read
        }
        // the open cells of each half's final state; a board the guard stopped before an earlier count reports it again
        const uint32_t opn = w6_open_cells(c, hl, half);
        if (hl == 0u && work) {
            a.open7[j] = (uint8_t)opn;
            if (!(rec6 >> half & 1u)) a.open6[j] = (uint8_t)opn;
            if (!(rec5 >> half & 1u)) a.open5[j] = (uint8_t)opn;
            if (!(rec >> half & 1u)) a.open4[j] = (uint8_t)opn;
        }
    }
}

}  // namespace sdk
