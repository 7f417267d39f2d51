// canon_launch.hip -- translation unit of canon_kernel (the canonical form of a board under the Sudoku
// symmetries, one board per wave; see canon_kernel.h)
#include "launch.h"
#include "canon_kernel.h"

namespace sdk {

hipError_t launch_canon(const CanonArgs& a, unsigned grid, hipStream_t stream) {
    canon_kernel<<<grid, 64, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
