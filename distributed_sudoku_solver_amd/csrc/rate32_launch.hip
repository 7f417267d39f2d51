// rate32_launch.hip -- translation unit of rate32_kernel (the propagation pass as a rater: all the
// single-cell probes of one level-4 board in one group; see rate32_kernel.h)
#include "launch.h"
#include "rate32_kernel.h"

namespace sdk {

hipError_t launch_rate32(const Rate32Args& a, unsigned grid, hipStream_t stream) {
    rate32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
