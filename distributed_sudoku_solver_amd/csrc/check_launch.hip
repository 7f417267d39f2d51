// check_launch.hip -- translation unit of the check kernels (check_kernel.h): the seven uint8 pipelines
// behind one switch over SDK_CHECK_*, and the int64 form.  Which pipeline a batch gets is the host's choice
// (SDK_OPT_CHECK_VARIANT and its fall-back rule); an unknown variant runs the default pipeline.
#include "../../include/sudoku_hip.h"
#include "launch.h"
#include "check_kernel.h"

namespace sdk {

hipError_t launch_check(int variant, const uint8_t* in, uint8_t* out, uint64_t n, unsigned grid, hipStream_t stream) {
    switch (variant) {
        case SDK_CHECK_REG2: check_kernel_rr2<<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
        case SDK_CHECK_GLDS2: check_kernel_glds<2><<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
        case SDK_CHECK_GLDS3: check_kernel_glds<3><<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
        case SDK_CHECK_GLDS4: check_kernel_glds<4><<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
        case SDK_CHECK_WAVE1: check_kernel_wave<1><<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
        case SDK_CHECK_WAVE2: check_kernel_wave<2><<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
        default: check_kernel<<<grid, kCheckThreads, 0, stream>>>(in, out, n); break;
    }
    return hipGetLastError();
}

hipError_t launch_check_i64(const int64_t* in, uint8_t* out, uint64_t n, unsigned grid, hipStream_t stream) {
    check_kernel_i64<<<grid, kCheckI64Threads, 0, stream>>>(in, out, n);
    return hipGetLastError();
}

}  // namespace sdk
