// grade32_kernel.h -- the propagation pass run as a grader: which technique does a board need?
// (sdk_grade_batch; include/sudoku_hip.h has the contract, DESIGN.md "Grading" the measurements)
//
// Same layout, the same device functions and the same group driver as prop32_kernel.h (p32_group_begin,
// p32_run, p32_decide, p32_refute_handed, p32_group_end): bit b of a word is board b of the half's 32,
// lane hl < 27 owns row triad hl and unit hl.  Only the schedule of a step is this file's.  The fast pass
// runs naked singles (N), hidden singles (H) and locked candidates (L) together, on a schedule tuned
// for speed; here every board climbs R1 = {N}, R2 = {N, H}, R3 = {N, H, L} one set at a time and only
// from a fixpoint of the set it is in, so the set it holds when it is found solved is its level.
//
// Per-board technique masks.  Two board masks per group, `hid` and `lck` (64-bit scalars, bit 32 h + b
// as the pass's other masks; a lane uses its half's word), gate the rules bitwise -- one instruction
// stream, no divergence, boards of one word at different levels at the same time:
//   H  p32_cells<true, true>: the `anyh` word of a cell (boards in which the cell has a hidden
//      single) is ANDed with hid, so c &= H | ~anyh leaves the other boards' words alone;
//   L  p32_locked only removes from open cells (& ~s): the boards outside lck get their bits set in
//      the lane's three single words before the call (s is recomputed by the next p32_singles and
//      the pass reads nothing else of it), so it removes nothing from them.
// Escalation.  Every cells phase reports change bits.  A live board unchanged by a full step
//   without hid           gets hid;
//   with hid, without lck gets lck, and the group's next step is a locked pass;
//   with lck              -- the group's next step is a locked pass; unchanged by that too: stuck,
//                         at F_3, listed for the search (a board that just got lck was unchanged by
//                         the N + H step before the pass, so the same test holds for it).
// The locked pass also runs on the other lck boards of the group (still R3, and it can only remove).
// Only live boards escalate, so a decided board keeps the masks it was decided with: level =
// 1 + hid + lck for a solved board.
//
// The step limit is a termination guard only.  Count the unit/cells steps (`it`) a board can be live
// for: a step either removes at least one of its 729 candidates, or is one of its two escalations, or
// is an unchanged step under lck -- and that one is followed by a locked pass which removes a
// candidate (one of the same 729) or ends the board.  So no board sees more than 729 + 3 steps short
// of F_3; kG32MaxSteps is above that.  (The fast pass's 96 is a hand-off, not a bound.)
//
// Open cells.  For a stuck board the number of open cells of its final state: after the loop one
// p32_singles puts the 81 single words of each half into the cell records, and lane (half, b) --
// here a board, not a triad -- reads its half's 81 words (every lane of the half the same address: a
// broadcast, no bank conflict) and counts the clear bits at position b.  81 ds_read_b32 and as many
// bit extracts per group that has a stuck board, against ~120 LDS instructions per step: cheaper
// than a bit-sliced adder tree across lanes (seven planes through five DPP stages), and no state.
//
// Outputs.  status / out / the undecided list are the shared driver's (handover, the "digit closed
// twice" refutation of a handed grid included); level[] for every board: 1..3 solved, 4 stuck
// (provisional: g32_verdict_kernel clears it unless the search finds exactly one completion), 0
// refuted or inexact; open[] the count for stuck boards, else 0.
#pragma once
#include "prop32_kernel.h"

namespace sdk {

// SDK_GRADE32_STATS (profiling builds only): per group, histograms of the unit/cells steps it ran and
// of its locked passes (tools/bench_grade.py --stats reads them)
#ifndef SDK_GRADE32_STATS
#define SDK_GRADE32_STATS 0
#endif

#if SDK_GRADE32_STATS
__device__ unsigned long long g_g32_stats[2][128];
#define G32_STAT(k, v) atomicAdd(&g_g32_stats[k][min((uint32_t)(v), 127u)], 1ull)
#else
#define G32_STAT(k, v) ((void)0)
#endif

// The search's verdicts into the grades: a listed board keeps level 4 and its open count only where
// the search found exactly one completion (budget hits, several and none: both 0).
__global__ void g32_verdict_kernel(const uint32_t* list, const int8_t* sub_st, uint8_t* level, uint8_t* open) {
    const uint32_t m = list[0];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
        if (sub_st[i] != 1) {
            const uint32_t j = list[1 + i];
            level[j] = 0;
            open[j] = 0;
        }
}

// the lane's half of a 64-bit board mask
__device__ __forceinline__ uint32_t g32_word(const P32Lane& w, uint64_t m) {
    return w.half() ? (uint32_t)(m >> 32) : (uint32_t)m;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void grade32_kernel(Grade32Args ga) {
    const Prop32Args& a = ga.p;
    __shared__ __attribute__((aligned(16))) uint8_t s_lds[kP32Lds];
    p32_lds_t* const lds = (p32_lds_t*)s_lds;
    const P32Lane w = p32_wave_begin(lds);
    const uint32_t groups = (uint32_t)((a.n + 63) / 64);
    uint32_t seg = blockIdx.x % kP32Heads;
    for (;;) {
        const uint32_t g = p32_dequeue(a, groups, seg);
        if (g == ~0u) break;
        P32Cells x;
        P32Group G;
        p32_group_begin(a, w, g, x, G);
        uint64_t hid = 0ull, lck = 0ull;   // the boards' technique masks
        uint64_t fixl = 0ull;              // lck boards unchanged by the step before this locked pass
        bool lc = false;
        uint32_t it = 0;
#if SDK_GRADE32_STATS
        uint32_t st_lc = 0;
#endif
        p32_run(G, [&]() {
            uint32_t empty, alls;
            p32_singles(w, x, empty, alls);
            __builtin_amdgcn_wave_barrier();
            if (lc) {
#if SDK_GRADE32_STATS
                ++st_lc;
#endif
                const uint32_t off = ~g32_word(w, lck);    // boards without L: every cell reads as closed
#pragma unroll
                for (int k = 0; k < 3; ++k) x.s[k] |= off;
                const uint32_t lc_own = p32_locked(w, x);
                const uint64_t lchg = p32_mask64(p32_half_or(w.act ? lc_own : 0u));
                const uint64_t stuck = fixl & ~lchg & G.live;
                G.undec |= stuck;
                G.live &= ~stuck;
                fixl = 0ull;
                lc = false;
                __builtin_amdgcn_wave_barrier();
                return;
            }
            p32_decide(w, lds, it == 0, empty, alls, G);
            if (G.live != 0ull && ++it >= kG32MaxSteps) {   // (unreachable: see the header)
                G.undec |= G.live;
                G.live = 0ull;
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t chg_own = p32_cells<true, true>(w, x, g32_word(w, hid));
            const uint64_t unch = G.live & ~p32_mask64(p32_half_or(w.act ? chg_own : 0u));
            // at a fixpoint of its set: the next set, or the locked pass that tells whether it is F_3
            fixl = unch & hid;
            lck |= fixl;
            hid |= unch;
            lc = fixl != 0ull;
            __builtin_amdgcn_wave_barrier();
        });
#if SDK_GRADE32_STATS
        if (threadIdx.x == 0) {
            G32_STAT(0, it);
            G32_STAT(1, st_lc);
        }
#endif
        __builtin_amdgcn_wave_barrier();
        // the stuck boards (undecided, exact): their open cells, and with handover their grids
        uint64_t stuck = G.undec & ~G.inexact;
        uint64_t handed = a.handover ? stuck : 0ull;
        uint32_t nopen = 0u;
        if (stuck) {
            uint32_t empty, alls;
            p32_singles(w, x, empty, alls);   // for the refutation and for the count
            __builtin_amdgcn_wave_barrier();
            if (handed) stuck &= ~p32_refute_handed(w, lds, G, handed);
            // this lane as board (half, hl): the clear bits hl of its half's 81 single words
            const uint32_t bit = w.hl();
            const p32_lds_t* const reg = w.reg();
#pragma unroll 9
            for (uint32_t j = 0; j < 81u; ++j) {
                const uint32_t s =
                    *(const volatile __attribute__((address_space(3))) uint32_t*)(reg + kP32Rec * j + 36u);
                nopen += (~s >> bit) & 1u;
            }
            __builtin_amdgcn_wave_barrier();
        }
        // the grades; then the answers, the statuses and the list
        const uint32_t me = p32_tid();        // board me of the group (32 half + hl)
        if ((G.valid >> me) & 1ull) {
            const bool sv = (G.solved >> me) & 1ull, st = (stuck >> me) & 1ull;
            ga.level[G.base + me] =
                (uint8_t)(sv ? 1u + (uint32_t)((hid >> me) & 1ull) + (uint32_t)((lck >> me) & 1ull) : (st ? 4u : 0u));
            ga.open[G.base + me] = (uint8_t)(st ? nopen : 0u);
        }
        p32_group_end(a, w, x, lds, G, handed);
    }
}

}  // namespace sdk
