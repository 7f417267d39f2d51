// chains_launch.hip -- translation unit of chain32_kernel (subsets, basic fish, wings, simple colouring,
// X-chains and XY-chains on the level-4 boards of the grade pass's list, one board per half-wave; see
// chains_kernel.h)
#include "launch.h"
#include "chains_kernel.h"

namespace sdk {

hipError_t launch_chains32(const Chains32Args& a, unsigned grid, hipStream_t stream) {
    chain32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
