// lane_launch.hip -- translation unit of solve_lane_kernel, the one-board-per-lane solver (SDK_SOLVER_LANE;
// solve_lane_kernel.h).  A unit of its own, not a second kernel in solve_launch.hip: the two kernels share
// solve_kernel.h's device functions, and each keeps the inlining it gets when it is their only caller.
#include "launch.h"
#include "solve_lane_kernel.h"

namespace sdk {

hipError_t launch_solve_lane(const SolveArgs& a, unsigned grid, hipStream_t stream) {
    solve_lane_kernel<<<grid, kLaneThreads, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace sdk
