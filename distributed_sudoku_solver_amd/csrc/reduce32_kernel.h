// reduce32_kernel.h -- the propagation pass run as a minimiser: which clues can go while the technique
// set R_L (N; N + H; N + H + L, see grade32_kernel.h) still closes the board?  (sdk_minimize_level_batch;
// include/sudoku_hip.h has the contract, DESIGN.md "Level-minimal puzzles" the argument and the figures)
//
// A board R_L closes has exactly one completion, so no search is needed: the verdict of a trial is the
// pass restricted to R_L.  And removing a given only enlarges every candidate set the rules reach, so a
// removal that fails once fails at every later state: one pass over the board's cell order gives a
// puzzle in which no clue can go -- the whole 81-round loop of a group runs in one kernel, with no
// candidate boards in memory and no host in the loop.
//
// Same layout, the same device functions and the same group driver as prop32_kernel.h (p32_wave_begin,
// p32_load, p32_planes, p32_singles, p32_decide, p32_cells, p32_locked, p32_run, p32_mask64, p32_dequeue,
// p32_answers): one group is 64 consecutive boards, bit b of a word is board b of the half's 32, lane
// hl < 27 owns row triad hl and unit hl.  What this file adds is the state a group carries across its
// runs and how a run's boards are made from it:
//   state    per lane and cell the four binary planes of the givens (P[k][i]: bit b = bit i of the value
//            of cell 3 hl + k in board b; 0 = empty), twelve words, loaded and transposed once; the
//            boards with an inert given; `elig`.  Everything else is 64-bit masks in scalar registers.
//   run -1   eligibility: the candidate words are the minterms of the planes, the first step carries the
//            duplicate test, elig = solved (a board with an inert or duplicated given never is).
//   round q  board `me` of the group is lane `me`, which reads the board's order byte q: its trial cell.
//            The lanes that own the cells get, per cell k of their triad, the word T[k] of the boards
//            whose trial cell it is, through a table of 82 x 2 words in LDS (over the first cell
//            records, idle between two runs): zeroed, one ds_or_b32 of 1 << b per lane at (cell, half)
//            -- a byte >= 81 ORs nothing into the spare entry 81 -- and three reads per triad lane.
//            The trial's planes are P[k][i] & ~T[k]; its live boards are the eligible ones whose trial
//            cell is a given.  A round with no live board is skipped (a uniform branch).
//   steps    the grader's step with the technique masks preset and no escalation: hidden singles in
//            every board for L >= 2, else in none.  A live board unchanged by a full step is at a
//            fixpoint of N / N + H: for L < 3 the trial has failed; for L = 3 a locked pass follows, and
//            the trial fails if that removes nothing either (grade32_kernel's test for `stuck`).  A trial
//            holds the completion, so it is never refuted; kG32MaxSteps is the termination guard, and a
//            trial that reached it fails.
//   commit   P[k][i] &= ~(T[k] & solved).
//   end      the final planes' minterms through p32_singles / p32_answers as the pass's answers go; the
//            ineligible boards get their input bytes the way the pass's refuted boards do; status.
#pragma once
#include "prop32_kernel.h"
#include "reduce_args.h"

namespace sdk {

constexpr uint32_t kRd32Table = 82u * 8u;   // the trial table: (half 0, half 1) words of cells 0..80, a spare pair
static_assert(kRd32Table <= kP32Region, "the trial table lies in the first half's cell records");

// p32_minterms on gathered planes: a cell's nine candidate words from its four plane words
__device__ __forceinline__ void rd32_minterms(const uint32_t (&P)[4], uint32_t (&c)[9]) {
    const uint32_t e = ~(P[0] | P[1] | P[2] | P[3]);        // empty cells: every digit
    const uint32_t n3 = ~P[3];
    c[0] = (P[0] & ~P[1] & ~P[2] & n3) | e;
    c[1] = (~P[0] & P[1] & ~P[2] & n3) | e;
    c[2] = (P[0] & P[1] & ~P[2] & n3) | e;
    c[3] = (~P[0] & ~P[1] & P[2] & n3) | e;
    c[4] = (P[0] & ~P[1] & P[2] & n3) | e;
    c[5] = (~P[0] & P[1] & P[2] & n3) | e;
    c[6] = (P[0] & P[1] & P[2] & n3) | e;
    c[7] = (P[3] & ~P[0]) | e;
    c[8] = (P[3] & P[0]) | e;
}

// the lane's half of a 64-bit board mask
__device__ __forceinline__ uint32_t rd32_word(uint64_t m) { return (p32_tid() >> 5) ? (uint32_t)(m >> 32) : (uint32_t)m; }

// The trial words of one round.  cell: the trial cell of board `me` = this lane (>= 81: none).  Returns
// in T[k] the boards of the lane's half whose trial cell is cell 3 hl + k (spare lanes: triad 26's).
__device__ __forceinline__ void rd32_trial_words(p32_lds_t* lds, uint32_t cell, uint32_t (&T)[3]) {
    const uint32_t t = p32_tid(), hl = t & 31u, half = t >> 5;
    __builtin_amdgcn_wave_barrier();
    p32_st(lds, 8u * t, 0u, 0u);
    if (t < 82u - 64u) p32_st(lds, 8u * (t + 64u), 0u, 0u);
    __builtin_amdgcn_wave_barrier();
    {
        const uint32_t at = (uint32_t)(uintptr_t)lds + 8u * min(cell, 81u) + 4u * half;
        const uint32_t bit = cell < 81u ? 1u << hl : 0u;
        asm volatile("ds_or_b32 %0, %1" ::"v"(at), "v"(bit) : "memory");
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        T[k] = *(const volatile __attribute__((address_space(3))) uint32_t*)(lds + 8u * (3u * min(hl, 26u) + k) +
                                                                             4u * half);
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void reduce32_kernel(Reduce32Args ra) {
    const Prop32Args& a = ra.p;
    __shared__ __attribute__((aligned(16))) uint8_t s_lds[kP32Lds];
    p32_lds_t* const lds = (p32_lds_t*)s_lds;
    const P32Lane w = p32_wave_begin(lds);
    const uint32_t groups = (uint32_t)((a.n + 63) / 64);
    const uint32_t level = ra.level;
    const uint32_t hidw = level >= 2u ? ~0u : 0u;
    uint32_t seg = blockIdx.x % kP32Heads;
    for (;;) {
        const uint32_t g = p32_dequeue(a, groups, seg);
        if (g == ~0u) break;
        P32Group G;
        G.base = (uint64_t)g * 64;
        G.nb = (uint32_t)min<uint64_t>(64, a.n - G.base);
        G.valid = G.nb >= 64u ? ~0ull : ((1ull << G.nb) - 1ull);
        // the givens' planes, and the boards with an inert given
        uint32_t P[3][4];
        uint64_t inert64;
        {
            uint32_t d[32];
            p32_load(a.in + G.base * 81, G.nb, d);
            const uint32_t sh = (p32_tid() & 31u) == 26u ? 1u : 0u;
            uint32_t lo[3][4], hn[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                uint32_t l3[3];
                p32_planes(d + 8 * m, sh, l3, hn[m]);
#pragma unroll
                for (int k = 0; k < 3; ++k) lo[k][m] = l3[k];
            }
            uint32_t hi = p32_gather(hn, 0) | p32_gather(hn, 1) | p32_gather(hn, 2) | p32_gather(hn, 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int i = 0; i < 4; ++i) P[k][i] = p32_gather(lo[k], i);
                hi |= P[k][3] & (P[k][1] | P[k][2]);      // 10..15
            }
            inert64 = p32_mask64(p32_half_or(w.act ? hi : 0u));
        }
        const uint32_t me = p32_tid();        // board me of the group (32 half + hl)
        const uint8_t* const ord = ra.order + (G.base + min(me, G.nb - 1u)) * 81;
        uint64_t elig = 0ull;
        uint32_t cell = 0xFFu;                // board me's trial cell of this round
        P32Cells x;
        for (int q = -1; q < 81; ++q) {
            // the next round's order byte, on its way while this round runs
            uint32_t cell_next = 0xFFu;
            if (q < 80 && me < G.nb) cell_next = ord[q + 1];
            uint32_t T[3] = {0u, 0u, 0u};
            uint64_t live;
            if (q < 0) {
                live = G.valid & ~inert64;
            } else {
                rd32_trial_words(lds, cell, T);
                uint32_t any = 0u;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    T[k] &= P[k][0] | P[k][1] | P[k][2] | P[k][3];      // ... and it is a given there
                    any |= T[k];
                }
                live = elig & p32_mask64(p32_half_or(w.act ? any : 0u));
            }
            cell = cell_next;
            if (live == 0ull) {
                if (q < 0) break;      // no board to test: none eligible
                continue;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t Pt[4] = {P[k][0] & ~T[k], P[k][1] & ~T[k], P[k][2] & ~T[k], P[k][3] & ~T[k]};
                rd32_minterms(Pt, x.c[k]);
            }
            G.undec = 0ull;
            G.inexact = 0ull;
            G.live = live;
            G.solved = 0ull;
            G.contra = 0ull;
            uint64_t fixw = 0ull;              // live boards unchanged by the step before this locked pass
            bool lc = false;
            uint32_t it = 0;
            p32_run(G, [&]() {
                uint32_t empty, alls;
                p32_singles(w, x, empty, alls);
                __builtin_amdgcn_wave_barrier();
                if (lc) {
                    const uint32_t lc_own = p32_locked(w, x);
                    const uint64_t lchg = p32_mask64(p32_half_or(w.act ? lc_own : 0u));
                    G.live &= ~(fixw & ~lchg);      // at F_3 with open cells: the clue stays
                    fixw = 0ull;
                    lc = false;
                    __builtin_amdgcn_wave_barrier();
                    return;
                }
                p32_decide(w, lds, q < 0 && it == 0, empty, alls, G);
                if (G.live != 0ull && ++it >= kG32MaxSteps) G.live = 0ull;      // (a guard: see grade32_kernel.h)
                __builtin_amdgcn_wave_barrier();
                const uint32_t chg_own = p32_cells<true, true>(w, x, hidw);
                const uint64_t unch = G.live & ~p32_mask64(p32_half_or(w.act ? chg_own : 0u));
                if (level >= 3u) {
                    fixw = unch;
                    lc = unch != 0ull;
                } else {
                    G.live &= ~unch;                // at a fixpoint of N / N + H with open cells
                }
                __builtin_amdgcn_wave_barrier();
            });
            const uint64_t ok = G.solved & live;
            if (q < 0) {
                elig = ok;
                if (elig == 0ull) break;
            } else {
                const uint32_t okw = rd32_word(ok);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t keep = ~(T[k] & okw);
#pragma unroll
                    for (int i = 0; i < 4; ++i) P[k][i] &= keep;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // the results: the final planes as one-hot words (an empty cell's nine words leave its single
        // word clear: digit 0), the ineligible boards' inputs, the statuses
        {
#pragma unroll
            for (int k = 0; k < 3; ++k) rd32_minterms(P[k], x.c[k]);
            uint32_t empty, alls;
            p32_singles(w, x, empty, alls);
            __builtin_amdgcn_wave_barrier();
        }
        p32_answers(a, w, x, lds, G.base, G.nb, elig, G.valid & ~elig, 0ull);
        if (me < G.nb) ra.status[G.base + me] = (int8_t)((elig >> me) & 1ull);
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace sdk
