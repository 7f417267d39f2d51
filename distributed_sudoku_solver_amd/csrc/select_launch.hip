// select_launch.hip -- translation unit of the selection kernels of sdk_generate_graded (flag, scan,
// scatter; see select_kernel.h).  The flag and scatter grids are one wave per tile, whatever `grid`
// policy the host has elsewhere: a tile is the unit of the compaction.
#include "launch.h"
#include "select_kernel.h"

namespace sdk {

hipError_t launch_select_flag(const SelFlagArgs& a, uint32_t tiles, hipStream_t stream) {
    select_flag_kernel<<<tiles, kSelTileRows, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_select_scan(const SelScanArgs& a, hipStream_t stream) {
    select_scan_kernel<<<1, kSelScanThreads, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_select_scatter(const SelScatterArgs& a, uint32_t tiles, hipStream_t stream) {
    select_scatter_kernel<<<tiles, kSelTileRows, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
