// wings_kernel.h -- the wings stage: how many cells does a search-level board keep open once XY-wings,
// XYZ-wings and simple colouring join the fish?  (sdk_wings_batch; include/sudoku_hip.h has the contract,
// DESIGN.md "Wings and colouring" the measurements)
//
// R6 = R5 + {W, C} on the grader's candidate sets; F_6 is its fixpoint.
//   W (wings).  The pivot p is an open cell with 2 or 3 candidates P.  The pincers q != r are bivalue cells,
//     each sharing a unit with p, with candidate sets Q != R and Q & R a single digit z.
//     XY-wing:  P == (Q | R) & ~z.  Every cell other than p, q, r that shares a unit with q and with r loses z.
//     XYZ-wing: P == Q | R.  Every cell other than p, q, r that shares a unit with p, q and r loses z.
//   C (simple colouring, one digit d at a time).  The places of d are the cells that hold candidate d, closed
//     cells included, as in M_d of the fish.  A link is a unit with exactly two places.  The links make a
//     graph on the places; each connected component with at least one link is two-coloured.
//     Wrap: if two places of one colour share a unit, every place of that colour loses d.
//     Trap: a place outside the component that shares a unit with a place of each colour loses d.
// Both remove no digit of a completion.  A premise that further removals break is taken over by singles
// (a pincer that closes, a link that loses an end), so F_6 is one state whatever the order; the order here
// is a W + C pass from F_5, then F_5 again, until a pass changes nothing (tests/wings_model.py, "f5").
// One stage gives three counts: open4 and open5 exactly as fish32_kernel reports them, and open6.
//
// The frame is the fish stage's (fish_kernel.h), step for step: one board per 32-lane half, 81 candidate
// words per board in LDS, lanes 0..26 of a half own one unit each, a dequeue takes two list entries, and
// the light, heavy and deep tiers.  A fourth tier follows them:
//   wide   wings and colouring, both from one snapshot: every lane copies its cells hl + 32 k into the
//          half's second 81 words, and after a barrier all reads go to that copy, all removals by atomic AND
//          to the live words.
//          Colouring: lanes 0..8 of a half take one digit each.  A lane reads the 81 snapshot words (the
//          nine lanes read one address at a time: a broadcast) into three 27-bit band words, the digit's
//          places; the 27 unit masks are constants of the unrolled code (wings_device.h).
//          Wings: a lane's cells hl + 32 k are pivots.  One with 2 or 3 candidates walks its 20 peers in the
//          snapshot (dynamic LDS indices), keeps the bivalue ones that can be its pincers as a 20-bit mask,
//          and tries the pairs; the targets come from arithmetic row, column and box masks.
//          Nothing in registers is indexed dynamically, there are no private arrays.
// A half that a deep round leaves unchanged is at F_5: open5 is counted and stored there, once, and the half
// needs wide.  The round's kind is one value per wave: wide if every unfinished half needs wide, else deep
// if every unfinished half needs deep or wide, else heavy if some unfinished half needs heavy, else light.
// A half that needs wide while its wave-mate does not waits, as halves wait at deep: the rounds that run
// meanwhile have no effect on it, since it is a fixpoint of R5, and it keeps its tier.  So a wide round only
// ever runs when every unfinished half of the wave has stored open4 and open5: no wing or colouring removal
// touches a board before both are taken, whatever its wave-mate is doing.  A half that a wide round leaves
// unchanged is finished (F_6); a changed half goes back to light.
// A finished or idle half keeps executing, without effect, until the other half ends: the light and heavy
// rounds apply their rules to every half with a board (`act`), finished ones included, and leave a finished
// half as it is because F_6 is a fixpoint of R5; the deep and the wide rounds skip it (`live`).
//
// Termination: a round that changes a board removes at least one of its 729 candidates, so a wave has at
// most 2 * 729 changing rounds.  A round that changes neither half raises the round's kind (after light
// every unfinished half needs heavy or more, after heavy deep or more, after deep wide, after wide none is
// left), so at most four such rounds follow a changing one: 5 * 1458 + 4 rounds.  kF6MaxRounds is the guard
// above that; a board that reached it would report the open counts it has.  Inside a wide round, a component
// takes at least its seed out of the linked places and a closure sweep that adds nothing ends its growth;
// the pair walk consumes a 20-bit mask.  Bounds as in the fish kernel: a wave that dequeues at or past the
// list's length exits, an entry past it idles its half, every list entry is checked against n, and every LDS
// index is a cell 0..80 of the half's own words -- a peer of a cell below 81 (w6_peer), or a bit below 27 of
// a band word plus 27 times the band.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "subsets_device.h"
#include "wings_args.h"
#include "wings_device.h"

namespace sdk {

constexpr uint32_t kF6MaxRounds = 8192;      // above 5 * 1458 + 4 (see above)
constexpr uint32_t kW6Light = 0u, kW6Heavy = 1u, kW6Deep = 2u, kW6Wide = 3u;

// Bit `bits` leaves the cells of band word `m` (cells base + bit) that hold some of it in the snapshot.
__device__ __forceinline__ void w6_clear(const uint32_t* s, uint32_t* c, uint32_t m, uint32_t base, uint32_t bits) {
    while (m) {
        const uint32_t t = base + (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (s[t] & bits) atomicAnd(&c[t], ~bits);
    }
}

// The wings of one pivot cell (p < 81) in the snapshot s; removals go to c.
__device__ __forceinline__ void w6_wings(const uint32_t* s, uint32_t* c, uint32_t p, bool on) {
    const uint32_t P = s[p], pc = (uint32_t)__popc(P), row = p / 9u, col = p % 9u;
    const bool xy = pc == 2u;
    uint32_t cand = 0u;
#pragma nounroll
    for (uint32_t i = 0; i < 20u; ++i) {
        const uint32_t Q = s[w6_peer(row, col, i)];
        // a pincer of an XY-wing shares one digit with the pivot, one of an XYZ-wing lies inside it
        const bool ok = __popc(Q) == 2 && (xy ? __popc(Q & P) == 1 : (Q & ~P) == 0u);
        cand |= ok ? 1u << i : 0u;
    }
    cand = (on && (pc == 2u || pc == 3u)) ? cand : 0u;
    while (cand) {
        const uint32_t q = w6_peer(row, col, (uint32_t)__ffs((int)cand) - 1u), Q = s[q];
        cand &= cand - 1u;
        uint32_t rest = cand;
        while (rest) {
            const uint32_t r = w6_peer(row, col, (uint32_t)__ffs((int)rest) - 1u), R = s[r], z = Q & R;
            rest &= rest - 1u;
            if (Q != R && __popc(z) == 1 && (xy ? P == ((Q | R) & ~z) : P == (Q | R))) {
                W6Set T = w6_and(w6_units_of(q), w6_units_of(r));
                if (!xy) T = w6_and(T, w6_units_of(p));
                T = w6_andnot(T, w6_or(w6_cell(p), w6_or(w6_cell(q), w6_cell(r))));
                w6_clear(s, c, T.a, 0u, z);
                w6_clear(s, c, T.b, 27u, z);
                w6_clear(s, c, T.c, 54u, z);
            }
        }
    }
}

__global__ __launch_bounds__(64) void wing32_kernel(Wings32Args a) {
    __shared__ uint32_t s_c[2][kS4LdsWords];     // the candidate words
    __shared__ uint32_t s_s[2][kS4LdsWords];     // a wide round's snapshot of them
    const uint32_t t = threadIdx.x, hl = t & 31u, half = t >> 5;
    uint32_t* const c = s_c[half];
    uint32_t* const s = s_s[half];
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
        // per half, one bit each: finished; needs heavy; needs deep; needs wide; open4 stored; open5 stored
        uint32_t done = ~valid & 3u, t1 = 0u, t2 = 0u, t3 = 0u, rec = 0u, rec5 = 0u, round = 0u;
        uint32_t mode = kW6Light;                        // the kind of the round before
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
            if (mode == kW6Wide) {
                done |= still;                           // unchanged by a wide round: F_6
            } else if (mode == kW6Deep) {
                if (still & ~rec5) {                     // unchanged by a deep round: F_5, for the first time
                    const uint32_t opn = w6_open_cells(c, hl, half);
                    if (hl == 0u && work && ((still & ~rec5) >> half & 1u)) a.open5[j] = (uint8_t)opn;
                }
                rec5 |= still;
                t3 |= still;
            } else if (mode == kW6Heavy) {
                if (still & ~rec) {                      // unchanged by a heavy round: F_4, for the first time
                    const uint32_t opn = w6_open_cells(c, hl, half);
                    if (hl == 0u && work && ((still & ~rec) >> half & 1u)) a.open4[j] = (uint8_t)opn;
                }
                rec |= still;
                t2 |= still & ~t3;
            } else {
                t1 |= still & ~(t2 | t3);                // the light rules are spent (a half that waits keeps its tier)
            }
            t1 &= ~(chg | t2 | t3);
            t2 &= ~(chg | t3);
            t3 &= ~chg;                                  // a changed half starts from the light rules again
            if (done == 3u || ++round >= kF6MaxRounds) break;
            const uint32_t live = ~done & 3u;
            mode = (t3 & live) == live          ? kW6Wide
                   : ((t2 | t3) & live) == live ? kW6Deep
                   : (t1 & live)                ? kW6Heavy
                                                : kW6Light;
            __syncthreads();                             // every lane has read this round's snapshot
            if (mode == kW6Wide) {
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
                    w6_wings(s, c, cell < 81u ? cell : 0u, wl && cell < 81u);
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
                w6_clear(s, c, lose.a, 0u, 1u << hl);
                w6_clear(s, c, lose.b, 27u, 1u << hl);
                w6_clear(s, c, lose.c, 54u, 1u << hl);
                __syncthreads();                         // the removals are in before the next read
                continue;
            }
            if (mode == kW6Deep) {
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
            const bool heavy = mode == kW6Heavy;
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
        // the open cells of each half's final state; a board the guard stopped before F_4 or F_5 reports it again
        const uint32_t opn = w6_open_cells(c, hl, half);
        if (hl == 0u && work) {
            a.open6[j] = (uint8_t)opn;
            if (!(rec5 >> half & 1u)) a.open5[j] = (uint8_t)opn;
            if (!(rec >> half & 1u)) a.open4[j] = (uint8_t)opn;
        }
    }
}

}  // namespace sdk
