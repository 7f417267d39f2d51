// generate_launch.hip -- translation unit of generate_kernel (generate_kernel.h)
#include "launch.h"
#include "generate_kernel.h"

namespace sdk {

hipError_t launch_generate_grids(const GenArgs& a, unsigned grid, hipStream_t stream) {
    generate_kernel<<<grid, kGenThreads, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
