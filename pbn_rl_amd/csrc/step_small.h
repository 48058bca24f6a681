// step_small.h -- the small kernels (state histogram, reset) and the (W, B) dispatcher of the
// step kernels' template instances.
#pragma once
#include "step_args.h"
#include "step_debug.h"

namespace {

// ------------------------------------------------------------- state histogram
// Visits per state for the steady-state distribution.  States of a steady-state chain
// concentrate on a few attractor basins, so a wave first merges equal values (a few
// ballot rounds: the leader adds the count of its value) before per-lane atomics.
__global__ void __launch_bounds__(256) pbn_hist_kernel(const uint32_t* __restrict__ states, int64_t n_rows,
                                                       int64_t n_cols, int64_t row_stride, uint32_t mask,
                                                       uint32_t* __restrict__ hist) {
  const int64_t total = n_rows * n_cols;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool have = i < total;
    uint32_t v = 0;
    if (have) {
      const int64_t r = i / n_cols, c = i - r * n_cols;
      v = states[r * row_stride + c] & mask;
    }
    bool pending = have;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
      const uint64_t act = __ballot(pending);
      if (act == 0) break;
      const int leader = __builtin_ctzll(act);
      const uint32_t lv = __shfl(v, leader);
      const uint64_t same = __ballot(pending && v == lv);
      if ((threadIdx.x & 63) == leader) atomicAdd(&hist[lv], (uint32_t)__popcll(same));
      if (pending && v == lv) pending = false;
    }
    if (pending) atomicAdd(&hist[v], 1u);
  }
}

// ---------------------------------------------------------------- reset kernel
template <int W>
__global__ void __launch_bounds__(256) pbn_reset_kernel(const int32_t* __restrict__ att_start,
                                                        const uint32_t* __restrict__ att_states,
                                                        int n_attr, int n_states, int N, uint32_t am1_magic,
                                                        uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n,
                                                        uint32_t* state, uint8_t* target, uint8_t* t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t ge = env_offset + (uint64_t)i;
  uint32_t ns[W];
  uint32_t nt;
  if (n_attr >= 1) {
    // the pair and the start state from the 64-bit value (word 1 : word 0) of RESET call 0
    const Word4 r0 = pbn::draw(seed, ge, step, pbn::kStreamReset, 0);
    uint32_t hi = r0.y, lo = r0.x, as;
    uint64_t xr = 0;   // (nothing is drawn after the start state)
    pbn::pair_draw(hi, lo, (uint32_t)n_attr, am1_magic, as, nt);
    const uint32_t row = pbn::start_pick(hi, lo, as, false,
                                         [&](uint32_t j) { return att_start[CK(j, n_attr + 1, 20)]; }, xr);
#pragma unroll
    for (int w = 0; w < W; ++w) ns[w] = att_states[CK((size_t)row * W + w, (size_t)n_states * W, 22)];
  } else {
    nt = pbn::random_reset_state<W>((uint32_t)ge, (uint32_t)step,
                                    (uint32_t)((ge >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16),
                                    (uint32_t)seed, (uint32_t)(seed >> 32), N, ns);
  }
#pragma unroll
  for (int w = 0; w < W; ++w) state[(size_t)w * n + i] = ns[w];
  target[i] = (uint8_t)nt;
  t[i] = 0;
}

// The (W, B) dispatcher: the step kernels are instantiated for 1..4 state words and 4, 8, 12 or
// 16 probability bits.  make(w, b) receives the pair as std::integral_constant values and
// returns the host stub of its instance; nullptr for any other pair.  (for_state_words and
// for_prob_bits are its halves, for a caller that chooses something between the two.)
// (The policy rollout's instances take a second argument, PolicyFn: the dispatchers return what
// make returns.)
using StepFn = void (*)(StepArgs);
using PolicyFn = void (*)(StepArgs, PolicyArgs);

template <typename F>
auto for_state_words(int W, F f) -> decltype(f(std::integral_constant<int, 1>{})) {
  switch (W) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
  }
  return nullptr;
}

template <typename F>
auto for_prob_bits(int B, F f) -> decltype(f(std::integral_constant<int, 4>{})) {
  switch (B) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
  }
  return nullptr;
}

template <typename Make>
auto step_kernel_for(int W, int B, Make make)
    -> decltype(make(std::integral_constant<int, 1>{}, std::integral_constant<int, 4>{})) {
  return for_state_words(W, [&](auto w) { return for_prob_bits(B, [&](auto b) { return make(w, b); }); });
}

}  // namespace
