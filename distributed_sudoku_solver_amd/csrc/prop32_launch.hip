// prop32_launch.hip -- translation unit of prop32_kernel (bit-sliced root propagation, 32 boards
// per half-wave; see prop32_kernel.h)
#include "launch.h"
#include "prop32_kernel.h"

namespace sdk {

// The fallback's answers back into the batch: listed board i is board list[1 + i]; a board the search
// did not solve gets its own input back (DHT_Node.py:535), not the propagated grid it was searched from.
// One thread per 4 bytes of the dense answers (one dword load; 32-bit index math: the list holds at most
// 2^24 boards), grid-stride over the whole list.
__global__ void p32_scatter_kernel(const uint32_t* list, const uint8_t* sub_out, const int8_t* sub_st,
                                   const uint8_t* in, uint8_t* out, int8_t* status) {
    const uint32_t total = list[0] * 81u;
    for (uint32_t e0 = 4u * (blockIdx.x * blockDim.x + threadIdx.x); e0 < total; e0 += 4u * gridDim.x * blockDim.x) {
        uint32_t word;
        if (e0 + 4u <= total) {
            word = *reinterpret_cast<const uint32_t*>(sub_out + e0);
        } else {
            word = 0u;
            for (uint32_t b = 0; e0 + b < total; ++b) word |= (uint32_t)sub_out[e0 + b] << (8 * b);
        }
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t e = e0 + b;
            if (e >= total) break;
            const uint32_t i = e / 81u, c = e - 81u * i;
            const uint32_t j = list[1 + i];
            const int8_t st = sub_st[i];
            const uint64_t o = (uint64_t)j * 81u + c;
            out[o] = st == 1 ? (uint8_t)(word >> (8 * b)) : in[o];
            if (c == 0) status[j] = st;
        }
    }
}

#ifndef SDK_PROP32_WAVES_PER_EU
#define SDK_PROP32_WAVES_PER_EU 5
#endif
// The kernel body; kStamp (prop32_clock_kernel, a diagnostic twin: the timed kernel runs no stamp)
// writes s_memtime (shader clock) and s_memrealtime (100 MHz) at a workgroup's entry and exit to
// stamps[4 blockIdx.x ..], a buffer nothing else reads: the in-kernel clock of a launch is
// their ratio (MI355X_MICROARCH.md, "DVFS give-back" item 6), the clock the VALU roofline prices
template <bool kStamp>
__device__ __forceinline__ void prop32_body(Prop32Args a, uint64_t* stamps) {
    // (kStamp: eight bytes more, where the workgroup's stamp address waits for the exit -- held in
    // scalar registers through the loop it is the pair that no longer fits, and a scalar register
    // spilled costs the kernel a vector register, which costs it the fifth wave)
    __shared__ __attribute__((aligned(16))) uint8_t s_lds[kP32Lds + (kStamp ? 8u : 0u)];
    p32_lds_t* const lds = (p32_lds_t*)s_lds;
    if (kStamp && threadIdx.x == 0) {    // (stored at once: no register holds them through the loop)
        uint64_t* o = stamps + 4u * blockIdx.x;
        o[0] = __builtin_amdgcn_s_memtime();
        o[1] = __builtin_amdgcn_s_memrealtime();
        *(volatile __attribute__((address_space(3))) uint64_t*)(lds + kP32Lds) = (uint64_t)(uintptr_t)o;
    }
    const P32Lane w = p32_wave_begin(lds);
    const uint32_t groups = (uint32_t)((a.n + 63) / 64);
    uint32_t seg = blockIdx.x % kP32Heads;
    for (;;) {
        const uint32_t g = p32_dequeue(a, groups, seg);
        if (g == ~0u) break;
        P32Cells x;
        P32Group G;
        p32_group_begin(a, w, g, x, G);
        uint64_t fixw = 0ull;              // live boards unchanged by the step before this locked pass
        bool lc = false;
        uint32_t next_lc = a.lc_first;     // the step after which the next locked-candidates pass runs
#if SDK_PROP32_STATS
        uint32_t st_lc = 0, st_t4 = ~0u, st_t1 = ~0u;
#endif
        uint32_t it = 0;
        p32_run(G, [&]() {
            uint32_t empty, alls;
            p32_singles(w, x, empty, alls);
            __builtin_amdgcn_wave_barrier();
            if (lc) {
#if SDK_PROP32_STATS
                ++st_lc;
#endif
                const uint32_t lc_own = p32_locked(w, x);
                const uint64_t lchg = p32_mask64(p32_half_or(w.act ? lc_own : 0u));
                const uint64_t stuck = fixw & ~lchg & G.live;
                G.undec |= stuck;
                G.live &= ~stuck;
                fixw = 0ull;
                lc = false;
                __builtin_amdgcn_wave_barrier();
                return;
            }
            p32_decide(w, lds, it == 0, empty, alls, G);
#if SDK_PROP32_STATS
            if (st_t4 == ~0u && __builtin_popcountll(G.live) <= 4) st_t4 = it;
            if (st_t1 == ~0u && __builtin_popcountll(G.live) <= 1) st_t1 = it;
#endif
            // the verdicts emptied the group: no cells phase, nothing reads its update (p32_run)
            if (G.live == 0ull) {
                __builtin_amdgcn_wave_barrier();
                return;
            }
            // a group ended by one of these hand-offs is not at a fixpoint: it runs the cells phase
            // below, and its boards are handed over with this step's update
            if (a.tail_live && it >= a.tail_step && (uint32_t)__builtin_popcountll(G.live) <= a.tail_live) {
                G.undec |= G.live;   // the last few boards go to the search with their propagated grids
                G.live = 0ull;
            } else if (++it >= a.max_steps) {
                G.undec |= G.live;
                G.live = 0ull;
            }
            __builtin_amdgcn_wave_barrier();
            // step lc_first and every lc_every-th after it are followed by a locked-candidates pass;
            // that step also reports which boards it left unchanged (a board unchanged by it and by
            // the pass is stuck)
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
#if SDK_PROP32_STATS
        if (threadIdx.x == 0) {
            P32_STAT(0, it);
            P32_STAT(1, st_t4);
            P32_STAT(2, st_t1);
            P32_STAT(3, st_lc);
        }
#endif
        __builtin_amdgcn_wave_barrier();
        uint64_t handed = a.handover ? G.undec & ~G.inexact : 0ull;   // listed with their grids
        if (handed) {
            uint32_t empty, alls;
            p32_singles(w, x, empty, alls);
            __builtin_amdgcn_wave_barrier();
            (void)p32_refute_handed(w, lds, G, handed);
            __builtin_amdgcn_wave_barrier();
        }
        p32_group_end(a, w, x, lds, G, handed);
    }
    if (kStamp) {
        const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (p32_tid() == 0) {
            uint64_t* o = (uint64_t*)(uintptr_t)(*(volatile __attribute__((address_space(3))) uint64_t*)(lds + kP32Lds));
            o[2] = t1;
            o[3] = r1;
        }
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SDK_PROP32_WAVES_PER_EU))) void prop32_kernel(
    Prop32Args a) {
    prop32_body<false>(a, nullptr);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SDK_PROP32_WAVES_PER_EU))) void prop32_clock_kernel(
    Prop32Args a, uint64_t* stamps) {
    prop32_body<true>(a, stamps);
}

// stamps non-null: the diagnostic twin that records the in-kernel clock (prop32_body)
hipError_t launch_prop32(const Prop32Args& a, unsigned grid, hipStream_t stream, uint64_t* stamps) {
    if (stamps)
        prop32_clock_kernel<<<grid, 64, 0, stream>>>(a, stamps);
    else
        prop32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_p32_scatter(const uint32_t* list, const uint8_t* sub_out, const int8_t* sub_st, const uint8_t* in,
                              uint8_t* out, int8_t* status, unsigned grid, hipStream_t stream) {
    p32_scatter_kernel<<<grid, 256, 0, stream>>>(list, sub_out, sub_st, in, out, status);
    return hipGetLastError();
}

}  // namespace sdk

#if SDK_PROP32_STATS
// profiling build only: the g_p32_stats histograms (see prop32_kernel.h), zeroed after the read
extern "C" int sdk_debug_p32_stats(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sdk::g_p32_stats), sizeof(sdk::g_p32_stats)) != hipSuccess) return -1;
    static const unsigned long long zero[4][128] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(sdk::g_p32_stats), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif
