// solve_launch.hip -- translation unit of solve_kernel, the one-board-per-wave solver (its propagation,
// branching and stack helpers are solve_kernel.h's, which every other solver shares)
#include "launch.h"
#include "solve_kernel.h"

namespace sdk {

__global__ __launch_bounds__(64, 8) void solve_kernel(SolveArgs a) {
    __shared__ uint32_t s_cell[96];
    __shared__ uint32_t s_unit[32];
    __shared__ uint32_t s_br[kMaxDepth];
    Wave w;
    init_wave(w, s_cell, s_unit, s_br);
    w.stk = a.stack + (size_t)blockIdx.x * kStackWordsPerBlock;
    const int lane = w.lane;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(a.next, a.chunk);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if ((uint64_t)base >= a.n) break;
        const uint64_t end = min((uint64_t)base + a.chunk, a.n);
        for (uint64_t i = base; i < end; ++i) {
            const uint8_t* src = a.in + (a.in_first + i * a.in_step) * 81;
            const uint32_t inA = src[lane];
            const uint32_t inB = w.hasB ? (uint32_t)src[64 + lane] : 0u;
            uint32_t sa = cell_init(inA);
            uint32_t sb = w.hasB ? cell_init(inB) : kInert;
            // TASK `range` restricts the lowest-index empty input cell only (DHT_Node.py:474,522,531)
            const uint32_t fm = a.mask ? (((uint32_t)a.mask[i] >> 1) & kCands) : kCands;
            const unsigned long long za = __ballot(inA == 0);
            const unsigned long long zb = __ballot(w.hasB && inB == 0);
            if (za) {
                if (lane == (int)__builtin_ctzll(za)) sa &= fm | ~kCands;
            } else if (zb) {
                if (lane == (int)__builtin_ctzll(zb)) sb &= fm | ~kCands;
            }
            uint8_t* dst = a.out ? a.out + i * 81 : nullptr;
            uint64_t nodes = 0, rounds = 0, maxd = 0;
            int8_t st;
            // count mode: whole-subtree count (order-independent, so MRV); the
            // batch stops early once the running total reaches the limit.
            // solve mode: MRV search for <= 2 completions, or LEX for the first.
            bool skip = false;
            if (a.count_mode && a.limit) {
                unsigned long long tot = 0;
                if (lane == 0) tot = __hip_atomic_load(a.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                tot = __shfl(tot, 0);
                skip = tot >= a.limit;
            }
            const int order0 = (a.count_mode || a.order != ORDER_LEX) ? ORDER_MRV : ORDER_LEX;
            const uint64_t lim0 = a.count_mode ? a.limit : (order0 == ORDER_LEX ? 1u : 2u);
            int64_t c = 0;
            if (!skip) c = search(w, order0, sa, sb, lim0, a.budget, nodes, rounds, maxd, dst, inA, inB);
            if (!a.count_mode && order0 == ORDER_MRV && c >= 2)
                c = search(w, ORDER_LEX, sa, sb, 1, a.budget, nodes, rounds, maxd, dst, inA, inB);
            if (a.count_mode && lane == 0) {
                if (c > 0) atomicAdd(a.count, (unsigned long long)c);
                if (a.counts) a.counts[i] = (unsigned long long)(c < 0 ? 0 : c);
            }
            st = c < 0 ? (int8_t)-2 : (c > 0 ? (int8_t)1 : (int8_t)0);
            if (dst && c <= 0) write_board(w, dst, inA, inB, sa, sb, false);
            if (lane == 0) {
                if (a.status) a.status[i] = st;
                if (a.work) a.work[i] = a.work_rounds == 1 ? rounds : (a.work_rounds == 2 ? maxd : nodes);
            }
        }
    }
}

hipError_t launch_solve1(const SolveArgs& a, unsigned grid, hipStream_t stream) {
    solve_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
