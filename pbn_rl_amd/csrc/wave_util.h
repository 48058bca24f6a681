// wave_util.h -- the few wave-level helpers that the step kernels (step_parts.h), the DQN forward
// (dqn_forward.h) and the BDQ kernels (pbn_qnet.hip; learn_fwd.h, learn_bwd.h, learn_apply.h) share:
// one definition each.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Block barrier ordering LDS only.  __syncthreads() is a workgroup fence on every address
// space, so each wave would first wait (s_waitcnt vmcnt(0)) for its global stores (on CDNA they
// count in vmcnt with the loads) and for what it requested ahead: the step loops' per-step obs /
// reward / flags / flip-mask stores, the weight fragments of learn_fwd / learn_bwd.  The waves
// that use it communicate through LDS alone and never read back what they store to HBM in the
// loop.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

}  // namespace
