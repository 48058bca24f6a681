// pbn_eval.hip -- bookkeeping of the batched control evaluation (model_tester.py:587-658).
//
// The reference steers one env at a time from a source attractor towards a target attractor and
// counts env.step calls until the state lies in the target (:616), failing past 100 (:628,
// recorded as 101, :635).  Batched (pbn_rl_amd/evaluate.py) every (pair, run) is one env of a
// VectorPBNEnv and a protocol step is act -> pbn_step_dev -> pbn_eval_track on one stream:
//
//   pbn_eval_track   per env: first hit (count, hit state), the failure rule, the recorded
//                    actions, and the number of envs still open after the step (the survival
//                    curve the host polls instead of synchronising every step)
//   pbn_eval_reduce  per (source, target) pair: sum of the counts and failures, and the length
//                    histogram of all runs
//
// Both are one pass over a few bytes per env; closed envs keep stepping (no compaction, so env
// ids and with them the RNG coordinates never move) and are skipped here.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "../../include/pbn_env.h"
#include "host_check.h"
#include "net_view.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxSteps = 254;       // the step kernels' t is uint8
constexpr int kMaxBranches = 64;
constexpr int kBins = 256;           // >= kMaxSteps + 2

// One thread per env.  k = *d_step - step0 + 1 is the 1-based protocol step; a k outside
// 1..max_steps (a replay past the end) touches nothing.
__global__ void __launch_bounds__(kThreads) eval_track_kernel(
    int64_t n_alloc, int64_t n_real, int W, int K, int max_steps, const int64_t* __restrict__ d_step, int64_t step0,
    const uint8_t* __restrict__ flags, const int32_t* __restrict__ actions, const uint32_t* __restrict__ state,
    int32_t* __restrict__ count, uint8_t* __restrict__ open, uint32_t* __restrict__ hit_state,
    int16_t* __restrict__ strategy, int32_t* __restrict__ open_after) {
  const int64_t k64 = *d_step - step0 + 1;
  if (k64 < 1 || k64 > max_steps) return;      // uniform over the grid
  const int k = (int)k64;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  bool still = false;
  if (i < n_real && open[i] != 0) {
    if (strategy != nullptr) {
      int16_t* row = strategy + ((size_t)(k - 1) * (size_t)n_alloc + (size_t)i) * (size_t)K;
      const int32_t* act = actions + (size_t)i * (size_t)K;
      for (int b = 0; b < K; ++b) row[b] = (int16_t)act[b];
    }
    if (flags[i] & PBN_FLAG_TERMINATED) {
      count[i] = k;
      open[i] = 0;
      if (hit_state != nullptr)
        for (int w = 0; w < W; ++w) hit_state[(size_t)w * n_alloc + i] = state[(size_t)w * n_alloc + i];
    } else if (k == max_steps) {
      count[i] = max_steps + 1;
      open[i] = 0;
    } else {
      still = true;
    }
  }
  // one add per wave: every lane of the wave reaches the ballot (no early exits above)
  const unsigned long long mask = __ballot(still);
  if ((threadIdx.x & (kWave - 1)) == 0 && mask != 0ull) atomicAdd(&open_after[k], (int)__popcll(mask));
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

// One block per pair at a time (grid-stride over the pairs).  The block's histogram lives in LDS
// for all of its pairs and is merged once, one atomic per non-empty bin.
__global__ void __launch_bounds__(kThreads) eval_reduce_kernel(const int32_t* __restrict__ count, int64_t n_pairs,
                                                               int64_t runs, int max_steps,
                                                               int64_t* __restrict__ pair_sum,
                                                               int32_t* __restrict__ pair_fail,
                                                               unsigned long long* __restrict__ hist) {
  __shared__ unsigned int s_hist[kBins];
  __shared__ long long s_sum[kThreads / kWave];
  __shared__ long long s_fail[kThreads / kWave];
  const int tid = threadIdx.x;
  const int fail_bin = max_steps + 1;
  s_hist[tid] = 0u;                      // kBins == kThreads
  __syncthreads();
  for (int64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const int32_t* row = count + (size_t)p * (size_t)runs;
    long long sum = 0, fail = 0;
    for (int64_t r = tid; r < runs; r += kThreads) {
      int c = row[r];
      c = c < 0 ? 0 : (c > fail_bin ? fail_bin : c);      // keeps the bin inside s_hist
      atomicAdd(&s_hist[c], 1u);
      sum += c;
      fail += c == fail_bin;
    }
    sum = wave_sum(sum);
    fail = wave_sum(fail);
    if ((tid & (kWave - 1)) == 0) {
      s_sum[tid / kWave] = sum;
      s_fail[tid / kWave] = fail;
    }
    __syncthreads();
    if (tid == 0) {
      long long s = 0, f = 0;
      for (int w = 0; w < kThreads / kWave; ++w) {
        s += s_sum[w];
        f += s_fail[w];
      }
      pair_sum[p] = s;
      pair_fail[p] = (int32_t)f;
    }
    __syncthreads();
  }
  if (tid <= fail_bin && s_hist[tid] != 0u) atomicAdd(&hist[tid], (unsigned long long)s_hist[tid]);
}

static_assert(kBins == kThreads, "eval_reduce_kernel zeroes and merges one bin per thread");
static_assert(kMaxSteps + 2 <= kBins, "the histogram has max_steps + 2 bins");

using pbn::aligned;

}  // namespace

extern "C" {

int pbn_eval_track(int64_t n_alloc, int64_t n_real, int32_t words, int32_t n_branches, int32_t max_steps,
                   const int64_t* d_step, int64_t step0, const uint8_t* d_flags, const int32_t* d_actions,
                   const uint32_t* d_state, int32_t* d_count, uint8_t* d_open, uint32_t* d_hit_state,
                   int16_t* d_strategy, int32_t* d_open_after, void* stream) {
  if (n_alloc < 32 || (n_alloc & 31) || n_alloc >= ((int64_t)1 << 31))
    return pbn::set_error(PBN_EINVAL, "n_alloc must be a positive multiple of 32 below 2^31");
  if (n_real < 0 || n_real > n_alloc) return pbn::set_error(PBN_EINVAL, "n_real must be in 0..n_alloc");
  if (words < 1 || words > PBN_MAX_NODES / 32) return pbn::set_error(PBN_EINVAL, "words must be 1..4");
  if (n_branches < 1 || n_branches > kMaxBranches) return pbn::set_error(PBN_EINVAL, "n_branches must be 1..64");
  if (max_steps < 1 || max_steps > kMaxSteps) return pbn::set_error(PBN_EINVAL, "max_steps must be 1..254");
  if (!d_step || !d_flags || !d_state || !d_count || !d_open || !d_open_after)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  if (d_strategy && !d_actions) return pbn::set_error(PBN_EINVAL, "d_strategy needs d_actions");
  if (!aligned(d_step, 8)) return pbn::set_error(PBN_EINVAL, "d_step must be 8-byte aligned");
  if (!aligned(d_actions, 4) || !aligned(d_state, 4) || !aligned(d_count, 4) || !aligned(d_hit_state, 4) ||
      !aligned(d_open_after, 4))
    return pbn::set_error(PBN_EINVAL, "d_actions, d_state, d_count, d_hit_state and d_open_after must be 4-byte aligned");
  if (!aligned(d_strategy, 2)) return pbn::set_error(PBN_EINVAL, "d_strategy must be 2-byte aligned");
  const unsigned blocks = (unsigned)((n_alloc + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(eval_track_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, n_alloc, n_real,
                     (int)words, (int)n_branches, (int)max_steps, d_step, step0, d_flags, d_actions, d_state, d_count,
                     d_open, d_hit_state, d_strategy, d_open_after);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}

int pbn_eval_reduce(const int32_t* d_count, int64_t n_pairs, int64_t runs, int32_t max_steps, int64_t* d_pair_sum,
                    int32_t* d_pair_fail, int64_t* d_hist, void* stream) {
  if (n_pairs < 1 || runs < 1 || runs >= ((int64_t)1 << 31) || n_pairs > (((int64_t)1 << 40) / runs))
    return pbn::set_error(PBN_EINVAL, "n_pairs >= 1, 1 <= runs < 2^31, n_pairs * runs <= 2^40");
  if (max_steps < 1 || max_steps > kMaxSteps) return pbn::set_error(PBN_EINVAL, "max_steps must be 1..254");
  if (!d_count || !d_pair_sum || !d_pair_fail || !d_hist) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!aligned(d_count, 4) || !aligned(d_pair_fail, 4))
    return pbn::set_error(PBN_EINVAL, "d_count and d_pair_fail must be 4-byte aligned");
  if (!aligned(d_pair_sum, 8) || !aligned(d_hist, 8))
    return pbn::set_error(PBN_EINVAL, "d_pair_sum and d_hist must be 8-byte aligned");
  const unsigned blocks = (unsigned)std::min<int64_t>(n_pairs, 2048);
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, d_count, n_pairs, runs,
                     (int)max_steps, d_pair_sum, d_pair_fail, reinterpret_cast<unsigned long long*>(d_hist));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}

}  // extern "C"
