// wings_launch.hip -- translation unit of wing32_kernel (subsets, basic fish, wings and simple colouring on
// the level-4 boards of the grade pass's list, one board per half-wave; see wings_kernel.h)
#include "launch.h"
#include "wings_kernel.h"

namespace sdk {

hipError_t launch_wings32(const Wings32Args& a, unsigned grid, hipStream_t stream) {
    wing32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
