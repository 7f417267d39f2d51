// solve2_launch.hip -- separate translation unit for solve2_kernel (two boards per
// wave), compiled with -mllvm -simplifycfg-sink-common=false (see Makefile): with
// common-store sinking the three per-lane cell states are stored through a phi
// of their addresses and demoted to scratch memory.
#include "launch.h"
#include "solve2_kernel.h"

namespace sdk {

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void solve2_kernel(SolveArgs args) {
    __shared__ uint32_t s_cell[2 * 96];
    __shared__ uint32_t s_unit[2 * 32];
    __shared__ uint32_t s_br[2][kMaxDepth];
    __shared__ uint2 s_stk[kLdsLevels][64];
    Lane2 w;
    init_lane2(w, s_cell, s_unit);
    uint2* g_stk = reinterpret_cast<uint2*>(args.stack) + (size_t)blockIdx.x * (kMaxDepth * 64);
    Args2 a;
    a.in = args.in;
    a.in_first = args.in_first;
    a.in_step = args.in_step;
    a.mask = args.mask;
    a.next = args.next;
    a.chunk = args.chunk;
    a.n = args.n;
    a.order = args.order;
    a.out = args.out;
    a.status = args.status;
    a.work = args.work;
    a.work_rounds = args.work_rounds;
    a.budget = args.budget;

    Board2 b;
    b.bidx = 0xFFFFFFFFu;   // ++ -> 0 >= bend = 0: first dequeue
    b.bend = 0;
    b.in0 = b.in1 = b.in2 = 0;
    b.depth = 0;
    b.count = 0;
    next_board(w, a, b);

    for (;;) {
        if (!__any((int)b.active)) break;
        bool bad, chg;
        round2(w, b.s0, b.s1, b.s2, bad, chg);
        ++b.rounds;
        const bool ev = b.active && (bad || !chg);
        if (!__any((int)ev)) continue;
        if (!ev) continue;
        ++b.nodes;
        int r = bad ? P_CONTRA
                    : (half_any(w, open_count2(b.s0) >= 2 || open_count2(b.s1) >= 2 || open_count2(b.s2) >= 2) ? P_OPEN
                                                                                                          : P_SOLVED);
        if (a.budget && b.nodes > a.budget) {
            finish_board(w, a, b, -2);
            continue;
        }
        if (r == P_SOLVED) {
            ++b.count;
            if (b.count == 1 && w.act) {
                uint8_t* dst = a.out + (uint64_t)b.bidx * 81;
                dst[w.c0] = (uint8_t)out_byte(b.in0, b.s0, true);
                dst[w.c1] = (uint8_t)out_byte(b.in1, b.s1, true);
                dst[w.c2] = (uint8_t)out_byte(b.in2, b.s2, true);
            }
            if (b.count >= b.lim) {
                if (b.order == ORDER_MRV) {      // >= 2 completions: lex re-search
                    b.order = ORDER_LEX;
                    b.lim = 1;
                    start_board(w, a, b, false);
                } else {
                    finish_board(w, a, b, 1);
                }
                continue;
            }
            r = P_CONTRA;
        }
        if (r == P_OPEN) {
            uint32_t key = ~0u;
            if (w.act)
                key = min(branch_key(b.s0, w.c0, b.order), min(branch_key(b.s1, w.c1, b.order),
                                                               branch_key(b.s2, w.c2, b.order)));
            key = half_min(key);
            const int cell = (int)((key >> 9) & 0x7Fu);
            const uint32_t m = key & kCands;
            const uint32_t d = m & (0u - m);
            const uint2 snap = make_uint2(pack2(b.s0) | (pack2(b.s1) << 16), pack2(b.s2));
            if (b.depth < kLdsLevels) s_stk[b.depth][w.lane] = snap;
            else g_stk[b.depth * 64 + w.lane] = snap;
            if (w.hl == 0) s_br[w.half][b.depth] = (uint32_t)cell | ((m ^ d) << 16);
            ++b.depth;
            b.maxd = max(b.maxd, (uint32_t)b.depth);
            set_cell2(w, b.s0, b.s1, b.s2, cell, d);
            continue;
        }
        // contradiction: resume the deepest level with untried digits
        if (b.depth == 0) {
            finish_board(w, a, b, b.count > 0 ? 1 : 0);
            continue;
        }
        const uint32_t br = s_br[w.half][b.depth - 1];
        const int cell = (int)(br & 0xFFu);
        uint32_t rest = br >> 16;
        const uint32_t d = rest & (0u - rest);
        rest ^= d;
        const uint2 snap = b.depth - 1 < kLdsLevels ? s_stk[b.depth - 1][w.lane] : g_stk[(b.depth - 1) * 64 + w.lane];
        b.s0 = unpack2(snap.x & 0xFFFFu);
        b.s1 = unpack2(snap.x >> 16);
        b.s2 = unpack2(snap.y);
        if (rest == 0) --b.depth;
        else if (w.hl == 0) s_br[w.half][b.depth - 1] = (uint32_t)cell | (rest << 16);
        set_cell2(w, b.s0, b.s1, b.s2, cell, d);
    }
}

hipError_t launch_solve2(const SolveArgs& a, unsigned grid, hipStream_t stream) {
    solve2_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
