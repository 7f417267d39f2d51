// reduce32_launch.hip -- translation unit of reduce32_kernel (the propagation pass as a minimiser: a
// group's 81 removal rounds under one technique set in one kernel; see reduce32_kernel.h)
#include "launch.h"
#include "reduce32_kernel.h"

namespace sdk {

hipError_t launch_reduce32(const Reduce32Args& a, unsigned grid, hipStream_t stream) {
    reduce32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
