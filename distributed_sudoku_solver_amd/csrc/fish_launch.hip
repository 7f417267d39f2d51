// fish_launch.hip -- translation unit of fish32_kernel (subsets and basic fish on the level-4 boards of the
// grade pass's list, one board per half-wave; see fish_kernel.h)
#include "launch.h"
#include "fish_kernel.h"

namespace sdk {

hipError_t launch_fish32(const Fish32Args& a, unsigned grid, hipStream_t stream) {
    fish32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
