// check_args.h -- what the host and the check kernels (check_kernel.h) share: the tile a workgroup owns,
// which is what the host sizes a check grid by.  Plain C++.
#pragma once

namespace sdk {

constexpr int kCheckThreads = 256;       // boards per tile = threads per workgroup of the seven uint8 pipelines
constexpr int kCheckI64Threads = 256;    // check_kernel_i64: one board per thread

}  // namespace sdk
