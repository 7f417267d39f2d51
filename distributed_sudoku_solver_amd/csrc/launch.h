// launch.h -- the kernels that live in translation units of their own (*_launch.hip), behind launch
// functions.  A launch function enqueues on `stream` with the grid it is given (grid policy is the
// host's) and the kernel's own workgroup size, and returns hipGetLastError().  With the *_args.h headers
// this is all the host (sudoku_hip.hip) sees of those kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "donate_args.h"
#include "frontier_args.h"
#include "prop32_args.h"
#include "rate_args.h"
#include "reduce_args.h"
#include "select_args.h"
#include "solve_args.h"
#include "subsets_args.h"

namespace sdk {

// solve_launch.hip, solve2_launch.hip, solve4_launch.hip
hipError_t launch_solve1(const SolveArgs& a, unsigned grid, hipStream_t stream);
hipError_t launch_solve2(const SolveArgs& a, unsigned grid, hipStream_t stream);
hipError_t launch_solve4(const SolveArgs& a, unsigned grid, hipStream_t stream);
int solve4_dn_blocks_per_cu();   // resident workgroups per CU of solve4_kernel<true>
hipError_t launch_expand4(const ExpandArgs& a, unsigned grid, hipStream_t stream);   // expand4_kernel.h

// prop32_launch.hip, grade32_launch.hip
hipError_t launch_prop32(const Prop32Args& a, unsigned grid, hipStream_t stream, uint64_t* stamps);
hipError_t launch_p32_scatter(const uint32_t* list, const uint8_t* sub_out, const int8_t* sub_st, const uint8_t* in,
                              uint8_t* out, int8_t* status, unsigned grid, hipStream_t stream);
hipError_t launch_grade32(const Grade32Args& a, unsigned grid, hipStream_t stream);
hipError_t launch_g32_verdict(const uint32_t* list, const int8_t* sub_st, uint8_t* level, uint8_t* open,
                              unsigned grid, hipStream_t stream);

// rate32_launch.hip: one wave per level-4 board of the grade pass's list (its length is on the device)
hipError_t launch_rate32(const Rate32Args& a, unsigned grid, hipStream_t stream);

// reduce32_launch.hip: one wave per group of 64 boards (a.p.heads zeroed), all 81 rounds inside
hipError_t launch_reduce32(const Reduce32Args& a, unsigned grid, hipStream_t stream);

// subsets_launch.hip: one half-wave per level-4 board of the grade pass's list (its length is on the device)
hipError_t launch_subsets32(const Subsets32Args& a, unsigned grid, hipStream_t stream);

// select_launch.hip: one wave per tile of 64 rows (flag, scatter), one workgroup (scan)
hipError_t launch_select_flag(const SelFlagArgs& a, uint32_t tiles, hipStream_t stream);
hipError_t launch_select_scan(const SelScanArgs& a, hipStream_t stream);
hipError_t launch_select_scatter(const SelScatterArgs& a, uint32_t tiles, hipStream_t stream);

}  // namespace sdk
