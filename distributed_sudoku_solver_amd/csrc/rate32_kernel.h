// rate32_kernel.h -- the propagation pass run as a rater: how many single-cell backdoors does a
// search-level board have?  (sdk_rate_batch; include/sudoku_hip.h has the contract, DESIGN.md
// "Rating" the measurements)
//
// A board of level SDK_GRADE_SEARCH has exactly one completion S, clean givens and an F_3 with open
// cells.  For an empty input cell c, child(c) is the board with S[c] written into c; c is a backdoor
// when every cell of F_3(child(c)) is closed.  The outputs are the number of backdoor cells and the
// lowest one (the key).
//
// One group is all the probes of one parent.  A uniquely solvable board has at least 17 clues, so at
// most 64 empty cells, and a group of the pass is 64 boards: probe slot r -- bit r % 32 of half r / 32
// -- is the child of the parent's r-th empty cell, in cell order.  Same layout, the same device
// functions and the same group driver as prop32_kernel.h (p32_wave_begin, p32_singles, p32_decide,
// p32_cells, p32_locked, p32_run, p32_mask64); only the begin and the end of a group are this file's:
//   begin  nothing is loaded bit-sliced and nothing converted: the children are synthesised.  Lane hl
//          reads the three bytes of its triad from the parent and from the completion (both halves
//          the same parent).  A given g is the word c[k][g - 1] = ~0 and eight zero words, in all 32
//          boards alike; an empty cell is nine words of ~0 -- except in the one probe board that owns
//          the cell, where only the word of S[c] keeps its bit.  The rank of an empty cell comes from
//          three wave ballots ("cell k of my triad is empty") and popcounts below the lane.  The
//          slots past the e empties hold the unprobed parent and are outside `valid`.
//   steps  the fast pass's: N + H cells, a locked-candidates pass after step lc_first and every
//          lc_every-th, a board stuck when unchanged by the step before a pass and by the pass -- a
//          fixpoint of all three rules, F_3, which does not depend on the schedule.  Nothing is
//          handed over: no tail, no max_steps; kG32MaxSteps is the termination guard (a probe that
//          reached it would count as not closed).  The children are never refuted (they hold S) and
//          never inexact (clean givens plus a digit of S), so the first step needs no duplicate test.
//   end    no staging, no board stores: backdoors = popcount(solved), key = the cell whose slot is
//          the lowest set bit of solved.  Each lane kept the slots of its three cells in one packed
//          word, so the lane that owns the key's cell writes both bytes (lane 0 when there is none).
#pragma once
#include "prop32_kernel.h"
#include "rate_args.h"

namespace sdk {

constexpr uint32_t kR32NoSlot = 0xFFu;    // a given cell's slot in the packed word
constexpr uint32_t kR32NoKey = 0xFEu;     // "no probe closed": matches no slot, no marker

// The group of parent j: the lane's candidate words, the group's masks and rk, the slots of the lane's
// three cells (byte k: the rank of cell 3 hl + k among the parent's empty cells, kR32NoSlot for a given).
__device__ __forceinline__ void r32_group_begin(const Rate32Args& a, const P32Lane& w, uint32_t j, P32Cells& x,
                                                P32Group& G, uint32_t& rk) {
    const uint32_t t = p32_tid(), hl = t & 31u, half = t >> 5;
    // spare lanes read triad 0 (inside the row; their results are masked out like all their others)
    const uint64_t off = (uint64_t)j * 81u + (hl < 27u ? 3u * hl : 0u);
    uint32_t g[3], sd[3], b[3];
    bool e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = a.in[off + k];
        sd[k] = a.sol[off + k];
        e[k] = w.act && g[k] == 0u;
        b[k] = (uint32_t)__ballot(e[k]);      // the first half's lanes: both halves hold the same parent
    }
    const uint32_t below = (1u << hl) - 1u;
    uint32_t rank = (uint32_t)(__popc(b[0] & below) + __popc(b[1] & below) + __popc(b[2] & below));
    const uint32_t ne = (uint32_t)(__popc(b[0]) + __popc(b[1]) + __popc(b[2]));
    rk = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // the probe board that owns this cell, if it lies in this half (rel wraps above 31 otherwise)
        const uint32_t rel = rank - 32u * half;
        const uint32_t keep = ~((e[k] && rel < 32u) ? 1u << rel : 0u);
        rk |= (e[k] ? min(rank, 0xFDu) : kR32NoSlot) << (8 * k);
#pragma unroll
        for (int d = 0; d < 9; ++d)
            x.c[k][d] = g[k] == 0u ? (sd[k] == (uint32_t)d + 1u ? ~0u : keep) : (g[k] == (uint32_t)d + 1u ? ~0u : 0u);
        rank += e[k] ? 1u : 0u;
    }
    G.base = j;
    G.nb = 64u;
    G.valid = ne >= 64u ? ~0ull : ((1ull << ne) - 1ull);
    G.undec = 0ull;
    G.inexact = 0ull;
    G.live = G.valid;
    G.solved = 0ull;
    G.contra = 0ull;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void rate32_kernel(Rate32Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_lds[kP32Lds];
    p32_lds_t* const lds = (p32_lds_t*)s_lds;
    const P32Lane w = p32_wave_begin(lds);
    const uint32_t m = a.list[0];
    for (;;) {
        uint32_t i = 0;
        if (p32_tid() == 0) i = atomicAdd(a.next, 1u);
        i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
        if (i >= m) break;
        const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.list[1 + i]);
        if (j >= a.n || a.level[j] != 4u) continue;      // only the level-4 boards are probed
        P32Cells x;
        P32Group G;
        uint32_t rk;
        r32_group_begin(a, w, j, x, G, rk);
        uint64_t fixw = 0ull;              // live boards unchanged by the step before this locked pass
        bool lc = false;
        uint32_t next_lc = a.lc_first;     // the step after which the next locked-candidates pass runs
        uint32_t it = 0;
        p32_run(G, [&]() {
            uint32_t empty, alls;
            p32_singles(w, x, empty, alls);
            __builtin_amdgcn_wave_barrier();
            if (lc) {
                const uint32_t lc_own = p32_locked(w, x);
                const uint64_t lchg = p32_mask64(p32_half_or(w.act ? lc_own : 0u));
                G.live &= ~(fixw & ~lchg);      // stuck: at F_3 with open cells, not a backdoor
                fixw = 0ull;
                lc = false;
                __builtin_amdgcn_wave_barrier();
                return;
            }
            p32_decide(w, lds, false, empty, alls, G);
            if (G.live != 0ull && ++it >= kG32MaxSteps) G.live = 0ull;      // (a guard: see grade32_kernel.h)
            __builtin_amdgcn_wave_barrier();
            lc = G.live != 0ull && it == next_lc;
            if (lc) next_lc += a.lc_every;
            if (lc) {
                const uint32_t chg_own = p32_cells<true>(w, x);
                fixw = G.live & ~p32_mask64(p32_half_or(w.act ? chg_own : 0u));
            } else {
                (void)p32_cells<false>(w, x);
            }
            __builtin_amdgcn_wave_barrier();
        });
        __builtin_amdgcn_wave_barrier();
        // the rating: two one-byte stores from the lane of the first half that owns the key's cell
        const uint64_t sv = G.solved & G.valid;
        const uint32_t low = sv ? (uint32_t)__builtin_ctzll(sv) : kR32NoKey;
        const uint32_t t = p32_tid();
        uint32_t cell = 0xFFu;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (((rk >> (8 * k)) & 0xFFu) == low) cell = 3u * t + (uint32_t)k;
        if (sv ? (t < 27u && cell != 0xFFu) : t == 0u) {
            a.backdoors[j] = (uint8_t)__builtin_popcountll(sv);
            if (a.key) a.key[j] = (uint8_t)(sv ? cell : 0xFFu);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace sdk
