// pbn_settle.hip -- the settle-law kernel instances (include/pbn_env.h "Step law"): the wave
// step kernel's variants 3 and 4 (pbn_step; the rollout of networks with gates) and the
// pipelined settle rollout pbn_rollout_settle, and the policy rollout's settle instance
// (pbn_step_wave<W, B, 4, PolicyArgs>), compiled beside pbn_env.hip so that the kernel
// instances build in parallel.
#include "rollout_settle.h"
#include "step_small.h"
#include "step_wave.h"

namespace {

template <int V>
StepFn pick_settle(int W, int B) {
  return step_kernel_for(W, B, [](auto w, auto b) -> StepFn {
    return pbn_step_wave<decltype(w)::value, decltype(b)::value, V>;
  });
}

}  // namespace

namespace pbn {

void* settle_pipe_kernel(int W, int B) {
  return reinterpret_cast<void*>(step_kernel_for(W, B, [](auto w, auto b) -> StepFn {
    return pbn_rollout_settle<decltype(w)::value, decltype(b)::value>;
  }));
}

void* settle_kernel(int W, int B, int lean) {
  return reinterpret_cast<void*>(lean ? pick_settle<4>(W, B) : pick_settle<3>(W, B));
}

void* settle_dqn_kernel(int W, int B) {
  return reinterpret_cast<void*>(step_kernel_for(W, B, [](auto w, auto b) -> PolicyFn {
    return pbn_step_wave<decltype(w)::value, decltype(b)::value, 4, PolicyArgs>;
  }));
}

}  // namespace pbn
