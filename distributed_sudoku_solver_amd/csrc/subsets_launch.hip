// subsets_launch.hip -- translation unit of subsets32_kernel (naked and hidden subsets on the level-4
// boards of the grade pass's list, one board per half-wave; see subsets_kernel.h)
#include "launch.h"
#include "subsets_kernel.h"

namespace sdk {

hipError_t launch_subsets32(const Subsets32Args& a, unsigned grid, hipStream_t stream) {
    subsets32_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
