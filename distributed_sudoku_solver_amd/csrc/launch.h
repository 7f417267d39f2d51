// launch.h -- every kernel lives in a translation unit of its own family (*_launch.hip), behind launch
// functions.  A launch function enqueues on `stream` with the grid it is given (grid policy is the
// host's) and the kernel's own workgroup size, and returns hipGetLastError().  With the *_args.h headers
// this is all the host (sudoku_hip.hip) sees of the kernels.  Plain C++.
#pragma once
#include <hip/hip_runtime.h>

#include "canon_args.h"
#include "chains_args.h"
#include "check_args.h"
#include "donate_args.h"
#include "fish_args.h"
#include "frontier_args.h"
#include "generate_args.h"
#include "minimize_args.h"
#include "prop32_args.h"
#include "rate_args.h"
#include "reduce_args.h"
#include "select_args.h"
#include "solve_args.h"
#include "subsets_args.h"
#include "wings_args.h"

namespace sdk {

// check_launch.hip: a tile of kCheckThreads boards per workgroup pass; `variant` is an SDK_CHECK_* (any
// other value: SDK_CHECK_REG1's pipeline).  The int64 form: kCheckI64Threads boards per workgroup pass.
hipError_t launch_check(int variant, const uint8_t* in, uint8_t* out, uint64_t n, unsigned grid, hipStream_t stream);
hipError_t launch_check_i64(const int64_t* in, uint8_t* out, uint64_t n, unsigned grid, hipStream_t stream);

// lane_launch.hip: kLaneThreads boards per workgroup at a time (persistent)
hipError_t launch_solve_lane(const SolveArgs& a, unsigned grid, hipStream_t stream);

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

// fish_launch.hip: the same work items and layout, with the fish rounds and both counts
hipError_t launch_fish32(const Fish32Args& a, unsigned grid, hipStream_t stream);

// wings_launch.hip: the same again, with the wide rounds (wings and simple colouring) and three counts
hipError_t launch_wings32(const Wings32Args& a, unsigned grid, hipStream_t stream);

// chains_launch.hip: the same again, with the chain rounds (X-chains and XY-chains) and four counts
hipError_t launch_chains32(const Chains32Args& a, unsigned grid, hipStream_t stream);

// canon_launch.hip: one wave per board (grid-stride over the slice)
hipError_t launch_canon(const CanonArgs& a, unsigned grid, hipStream_t stream);

// select_launch.hip: one wave per tile of 64 rows (flag, scatter), one workgroup (scan)
hipError_t launch_select_flag(const SelFlagArgs& a, uint32_t tiles, hipStream_t stream);
hipError_t launch_select_scan(const SelScanArgs& a, hipStream_t stream);
hipError_t launch_select_scatter(const SelScatterArgs& a, uint32_t tiles, hipStream_t stream);

// donate_launch.hip: the phased solve's list kernels.  collect: one thread per board of the batch, 256 per
// workgroup; seed: one wave per resumed board; scatter: one workgroup per listed board; prep: one workgroup.
hipError_t launch_dn_collect(const int8_t* status, uint64_t n, const uint32_t* n_dev, int8_t code, uint32_t* list,
                             uint32_t* total, const uint8_t* in, const uint16_t* mask, uint64_t in_first,
                             uint64_t in_step, uint8_t* out, uint16_t* out_mask, const DnResume& rs, unsigned grid,
                             hipStream_t stream);
hipError_t launch_dn_prep(const DnPrep& p, hipStream_t stream);
hipError_t launch_dn_seed(const uint32_t* seeds, const SplitSave* save, uint32_t* list, uint32_t* total,
                          const uint8_t* in, const uint16_t* mask, uint64_t in_first, uint64_t in_step, uint8_t* out,
                          uint16_t* out_mask, DnCtl* ctl, unsigned grid, hipStream_t stream);
hipError_t launch_dn_scatter(const uint32_t* list, const uint8_t* sub_out, const int8_t* sub_st,
                             const uint64_t* sub_work, bool depth, uint8_t* out, int8_t* status, uint64_t* work,
                             unsigned grid, hipStream_t stream);

// frontier_launch.hip: expand, one wave per board (kChunk boards per dequeue); scan_tiles, a tile of kScanTile
// entries per workgroup pass; emit, one wave per parent; gather, four boards per workgroup pass; begin, end,
// scan_top, first_init, first_hit and count_result are one workgroup each
hipError_t launch_frontier_begin(FrontierCtl* ctl, uint64_t target, int force, hipStream_t stream);
hipError_t launch_frontier_end(FrontierCtl* ctl, int first, hipStream_t stream);
hipError_t launch_expand(const ExpandArgs& a, unsigned grid, hipStream_t stream);
hipError_t launch_scan_tiles(const uint32_t* cnt, uint64_t* off, const FrontierCtl* ctl, uint64_t* tsum, unsigned grid,
                             hipStream_t stream);
hipError_t launch_scan_top(uint64_t* tsum, FrontierCtl* ctl, uint64_t cap, hipStream_t stream);
hipError_t launch_emit(const uint8_t* prop, const uint8_t* bcell, const uint16_t* bmask, const uint64_t* off,
                       const uint64_t* tsum, const FrontierCtl* ctl, uint8_t* out, unsigned grid, hipStream_t stream);
hipError_t launch_gather_boards(const uint8_t* in, uint64_t first, uint64_t step, uint64_t n, uint8_t* out,
                                unsigned grid, hipStream_t stream);
hipError_t launch_first_init(long long* found, hipStream_t stream);
hipError_t launch_first_hit(const int8_t* status, const uint8_t* out, uint64_t n, uint64_t lo, long long* found,
                            uint8_t* best, hipStream_t stream);
hipError_t launch_count_result(const int8_t* status, uint64_t n, const unsigned long long* count,
                               unsigned long long* result, hipStream_t stream);

// minimize_launch.hip: kMinBlockBytes bytes of the batch per workgroup pass
hipError_t launch_minimize_round(const MinRoundArgs& a, unsigned grid, hipStream_t stream);

// generate_launch.hip: one wave per workgroup (persistent)
hipError_t launch_generate_grids(const GenArgs& a, unsigned grid, hipStream_t stream);

}  // namespace sdk
