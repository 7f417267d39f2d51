// grade32_launch.hip -- translation unit of grade32_kernel (the propagation pass as a grader, one
// technique set at a time; see grade32_kernel.h)
#include "launch.h"
#include "grade32_kernel.h"

namespace sdk {

hipError_t launch_grade32(const Grade32Args& a, unsigned grid, hipStream_t stream) {
    grade32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_g32_verdict(const uint32_t* list, const int8_t* sub_st, uint8_t* level, uint8_t* open,
                              unsigned grid, hipStream_t stream) {
    g32_verdict_kernel<<<grid, 256, 0, stream>>>(list, sub_st, level, open);
    return hipGetLastError();
}

}  // namespace sdk

#if SDK_GRADE32_STATS
// profiling build only: the g_g32_stats histograms (see grade32_kernel.h), zeroed after the read
extern "C" int sdk_debug_g32_stats(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sdk::g_g32_stats), sizeof(sdk::g_g32_stats)) != hipSuccess) return -1;
    static const unsigned long long zero[2][128] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(sdk::g_g32_stats), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif
