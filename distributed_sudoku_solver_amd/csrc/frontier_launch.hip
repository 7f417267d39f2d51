// frontier_launch.hip -- translation unit of the frontier kernels (frontier_kernel.h): the level loop's
// begin / expand / scan / emit / end, the gather of a refinement's share, and the result kernels of the
// first-solution scan and the count.  The one-workgroup kernels take no grid.
#include "launch.h"
#include "frontier_kernel.h"

namespace sdk {

hipError_t launch_frontier_begin(FrontierCtl* ctl, uint64_t target, int force, hipStream_t stream) {
    frontier_begin_kernel<<<1, 1, 0, stream>>>(ctl, target, force);
    return hipGetLastError();
}

hipError_t launch_frontier_end(FrontierCtl* ctl, int first, hipStream_t stream) {
    frontier_end_kernel<<<1, 1, 0, stream>>>(ctl, first);
    return hipGetLastError();
}

hipError_t launch_expand(const ExpandArgs& a, unsigned grid, hipStream_t stream) {
    expand_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_scan_tiles(const uint32_t* cnt, uint64_t* off, const FrontierCtl* ctl, uint64_t* tsum, unsigned grid,
                             hipStream_t stream) {
    scan_tiles_kernel<<<grid, 1024, 0, stream>>>(cnt, off, ctl, tsum);
    return hipGetLastError();
}

hipError_t launch_scan_top(uint64_t* tsum, FrontierCtl* ctl, uint64_t cap, hipStream_t stream) {
    scan_top_kernel<<<1, 1024, 0, stream>>>(tsum, ctl, cap);
    return hipGetLastError();
}

hipError_t launch_emit(const uint8_t* prop, const uint8_t* bcell, const uint16_t* bmask, const uint64_t* off,
                       const uint64_t* tsum, const FrontierCtl* ctl, uint8_t* out, unsigned grid, hipStream_t stream) {
    emit_kernel<<<grid, 64, 0, stream>>>(prop, bcell, bmask, off, tsum, ctl, out);
    return hipGetLastError();
}

hipError_t launch_gather_boards(const uint8_t* in, uint64_t first, uint64_t step, uint64_t n, uint8_t* out,
                                unsigned grid, hipStream_t stream) {
    gather_boards_kernel<<<grid, 256, 0, stream>>>(in, first, step, n, out);
    return hipGetLastError();
}

hipError_t launch_first_init(long long* found, hipStream_t stream) {
    first_init_kernel<<<1, 1, 0, stream>>>(found);
    return hipGetLastError();
}

hipError_t launch_first_hit(const int8_t* status, const uint8_t* out, uint64_t n, uint64_t lo, long long* found,
                            uint8_t* best, hipStream_t stream) {
    first_hit_kernel<<<1, 256, 0, stream>>>(status, out, n, lo, found, best);
    return hipGetLastError();
}

hipError_t launch_count_result(const int8_t* status, uint64_t n, const unsigned long long* count,
                               unsigned long long* result, hipStream_t stream) {
    count_result_kernel<<<1, 256, 0, stream>>>(status, n, count, result);
    return hipGetLastError();
}

}  // namespace sdk
