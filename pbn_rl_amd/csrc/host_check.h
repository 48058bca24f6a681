// host_check.h -- the argument checks and host-side constants that the entry points of several
// sources share (library-internal; not part of the C-ABI).  Each message is spelled here once.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace pbn {

// p is a multiple of a (a power of two); a null pointer is aligned
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (uintptr_t)(a - 1u)) == 0; }

// the next multiple of 16 (elements of a flat buffer's segments)
__host__ __device__ inline int64_t al16(int64_t x) { return (x + 15) & ~int64_t(15); }

// EXPLORE law (DESIGN.md "Step semantics" 6): explore iff word 0 < floor(epsilon 2^32), so
// epsilon = 1 always explores and 0 never does
__host__ __device__ inline uint64_t explore_threshold(float epsilon) {
  return (uint64_t)floor((double)epsilon * 4294967296.0);
}

// The scalars an acting kernel reads from device memory when it runs (graph replays): the step
// index and epsilon, both optional unless need_step.  The message of the first failure, or null.
inline const char* dev_scalars_error(const void* d_step, const void* d_epsilon, bool need_step = false) {
  if (need_step && !d_step) return "null d_step";
  if (!aligned(d_step, 8)) return "d_step must be 8-byte aligned";
  if (!aligned(d_epsilon, 4)) return "d_epsilon misaligned";
  return nullptr;
}

// epsilon (NaN fails), then the device scalars: the group as the acting entry points check it
inline const char* explore_args_error(float epsilon, const void* d_step = nullptr, const void* d_epsilon = nullptr) {
  if (!(epsilon >= 0.f && epsilon <= 1.f)) return "epsilon must be in [0, 1]";
  return dev_scalars_error(d_step, d_epsilon);
}

}  // namespace pbn
