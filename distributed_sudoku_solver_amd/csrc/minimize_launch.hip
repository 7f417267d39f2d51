// minimize_launch.hip -- translation unit of minimize_round_kernel (minimize_kernel.h)
#include "launch.h"
#include "minimize_kernel.h"

namespace sdk {

hipError_t launch_minimize_round(const MinRoundArgs& a, unsigned grid, hipStream_t stream) {
    minimize_round_kernel<<<grid, kMinThreads, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
