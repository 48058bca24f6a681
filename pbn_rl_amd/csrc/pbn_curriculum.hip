// pbn_curriculum.hip -- curriculum resets on the device: the reference's env.rework_probas(ep_len)
// (bdq_model/__init__.py:203), which biases the next restarts towards the (start attractor, target
// attractor) pairs whose episodes run long, as two stages of a learning frame that a captured frame
// holds like any other launch.  The law is curriculum_law.h's (DESIGN.md "Curriculum resets").
//
//   pbn_curriculum_redraw   after the step and the ring store, before pbn_episode_track: every env
//                           whose step reset it restarts from a weighted draw instead of the step
//                           law's uniform one; the step kernels and their law are untouched
//   pbn_curriculum_refresh  after pbn_episode_track: every refresh_every frames one block rebuilds
//                           the table of prefix sums from the pair statistics
//
// Redraw: one thread per env.  A wave without a resetting lane returns after its flag loads: no
// Philox call, no table read.  A resetting lane runs the law's two binary searches (8 steps each at
// most) on the table in global memory, which a few hundred waves read at once and the caches hold.
// Copying rowcdf, or rowcdf and the rows, into a per-wave slice of LDS first was measured and bought
// nothing (DESIGN.md "Curriculum resets": the kernel sits at the cost of a launch either way), so
// there is no LDS, no barrier, no fence, flag or spin: no lane waits for another.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/pbn_env.h"
#include "curriculum_law.h"
#include "host_check.h"
#include "net_view.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kRefreshThreads = 1024;    // one block: 16 waves, a row each at a time

struct RedrawArgs {
  const int32_t* att_start;
  const uint32_t* att_states;
  uint64_t seed, step;
  const uint64_t* d_step;
  uint64_t env_offset;
  int64_t n_alloc, n_real;
  const uint8_t* flags;
  uint32_t* state;
  uint8_t* target;
  uint8_t* target_copy;
  const uint64_t* rowcdf;
  const uint32_t* cdf;
  const uint64_t* total;
  int A;
};

template <int W>
__global__ void __launch_bounds__(kThreads) curriculum_redraw_kernel(RedrawArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool reset = i < a.n_real && (a.flags[i] & PBN_FLAG_RESET) != 0;
  if (!reset) return;
  const int A = a.A;
  const uint64_t step = a.d_step ? *a.d_step : a.step;
  const pbn::Word4 x = pbn::draw(a.seed, a.env_offset + (uint64_t)i, step, pbn::kStreamCurriculum, 0u);
  const pbn::CurriculumDraw d = pbn::curriculum_draw(
      x, A, *a.total, [&](int s) { return a.rowcdf[s]; },
      [&](int s, int t) { return a.cdf[(size_t)s * (size_t)A + (size_t)t]; }, [&](int s) { return a.att_start[s]; });
  uint32_t words[W];
#pragma unroll
  for (int w = 0; w < W; ++w) words[w] = a.att_states[(size_t)d.row * W + w];
#pragma unroll
  for (int w = 0; w < W; ++w) a.state[(size_t)w * (size_t)a.n_alloc + (size_t)i] = words[w];
  a.target[i] = (uint8_t)d.t;
  if (a.target_copy) a.target_copy[i] = (uint8_t)d.t;
}

// inclusive prefix sum over the wave's lanes
template <typename T>
__device__ __forceinline__ T wave_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T up = __shfl_up(v, off);
    if (lane >= off) v += up;
  }
  return v;
}

// One block.  Wave j builds rows j, j + 16, ...: 64 weights at a time, a wave scan, the carry of the
// chunks before; then wave 0 scans the rows' totals.  Integer sums in a fixed association: the table
// is curriculum_build's whatever the schedule.
__global__ void __launch_bounds__(kRefreshThreads) curriculum_refresh_kernel(
    const int64_t* __restrict__ totals, const int64_t* __restrict__ pairs, int A, uint32_t H, int64_t refresh_every,
    uint64_t* __restrict__ rowcdf, uint32_t* __restrict__ cdf, uint64_t* __restrict__ total,
    uint64_t* __restrict__ refreshes) {
  __shared__ uint32_t row_total[256];
  if (refresh_every > 0 && totals[0] % refresh_every != 0) return;    // uniform over the block
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int s = wave; s < A; s += kRefreshThreads / kWave) {
    uint32_t carry = 0;
    for (int t0 = 0; t0 < A; t0 += kWave) {
      const int t = t0 + lane;
      const uint32_t w = t < A ? pbn::curriculum_weight_of(H, pairs, A, s, t) : 0u;
      const uint32_t c = wave_scan(w, lane) + carry;
      if (t < A) cdf[(size_t)s * (size_t)A + (size_t)t] = c;
      carry = __shfl(c, kWave - 1);
    }
    if (lane == 0) row_total[s] = carry;
  }
  __syncthreads();
  if (wave != 0) return;
  unsigned long long carry = 0;
  for (int s0 = 0; s0 < A; s0 += kWave) {
    const int s = s0 + lane;
    const unsigned long long c = wave_scan<unsigned long long>(s < A ? row_total[s] : 0u, lane) + carry;
    if (s < A) rowcdf[s] = c;
    carry = __shfl(c, kWave - 1);
  }
  if (lane == 0) {
    *total = carry;
    *refreshes += 1;
  }
}

using RedrawFn = void (*)(RedrawArgs);

RedrawFn pick_redraw(int W) {
  switch (W) {
    case 1: return curriculum_redraw_kernel<1>;
    case 2: return curriculum_redraw_kernel<2>;
    case 3: return curriculum_redraw_kernel<3>;
    case 4: return curriculum_redraw_kernel<4>;
  }
  return nullptr;
}

using pbn::aligned;

constexpr const char* kNullBuffer = "null buffer";
constexpr const char* kAttrRange = "n_attr must be in 2..254";

int launched() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}

struct Table {
  uint64_t* rowcdf;
  uint32_t* cdf;
  uint64_t* total;
  uint64_t* refreshes;
};
Table table_of(void* d_table, int A) {
  char* p = static_cast<char*>(d_table);
  return Table{reinterpret_cast<uint64_t*>(p), reinterpret_cast<uint32_t*>(p + pbn::curriculum_cdf_offset(A)),
               reinterpret_cast<uint64_t*>(p + pbn::curriculum_total_offset(A)),
               reinterpret_cast<uint64_t*>(p + pbn::curriculum_refreshes_offset(A))};
}

}  // namespace

extern "C" {

int pbn_curriculum_table_bytes(int32_t n_attr) {
  if (n_attr < pbn::kCurriculumMinAttr || n_attr > pbn::kCurriculumMaxAttr) return pbn::set_error(PBN_EINVAL, kAttrRange);
  return (int)pbn::curriculum_table_bytes(n_attr);
}

int pbn_curriculum_redraw(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step, uint64_t env_offset,
                          int64_t n_alloc, int64_t n_real, const uint8_t* d_flags, uint32_t* d_state, uint8_t* d_target,
                          uint8_t* d_target_copy, const void* d_table, void* stream) {
  pbn::NetView v;
  if (int rc = pbn::check_device(net)) return rc;
  if (int rc = pbn::net_view(net, &v)) return rc;
  if (v.W < 1 || v.W > PBN_MAX_NODES / 32) return pbn::set_error(PBN_EINVAL, "the net's state words must be 1..4");
  if (v.n_attr < pbn::kCurriculumMinAttr)
    return pbn::set_error(PBN_EINVAL, "the curriculum needs a net with at least two attractors");
  if (n_alloc < 32 || (n_alloc & 31) || n_alloc >= ((int64_t)1 << 31))
    return pbn::set_error(PBN_EINVAL, "n_alloc must be a positive multiple of 32 below 2^31");
  if (n_real < 1 || n_real > n_alloc) return pbn::set_error(PBN_EINVAL, "n_real must be in 1..n_alloc");
  if (!d_flags || !d_state || !d_target || !d_table) return pbn::set_error(PBN_EINVAL, kNullBuffer);
  if (!aligned(d_state, 4)) return pbn::set_error(PBN_EINVAL, "d_state must be 4-byte aligned");
  if (!aligned(d_table, 8)) return pbn::set_error(PBN_EINVAL, "d_table must be 8-byte aligned");
  if (const char* msg = pbn::dev_scalars_error(d_step, nullptr)) return pbn::set_error(PBN_EINVAL, msg);
  const int A = v.n_attr;
  const Table t = table_of(const_cast<void*>(d_table), A);
  const unsigned blocks = (unsigned)((n_real + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(pick_redraw(v.W), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream,
                     RedrawArgs{v.att_start, v.att_states, seed, step, d_step, env_offset, n_alloc, n_real, d_flags,
                                d_state, d_target, d_target_copy, t.rowcdf, t.cdf, t.total, A});
  return launched();
}

int pbn_curriculum_refresh(const int64_t* d_totals, const int64_t* d_pairs, int32_t n_attr, int32_t horizon,
                           int64_t refresh_every, void* d_table, void* stream) {
  if (n_attr < pbn::kCurriculumMinAttr || n_attr > pbn::kCurriculumMaxAttr) return pbn::set_error(PBN_EINVAL, kAttrRange);
  if (horizon < 1 || horizon > 65535) return pbn::set_error(PBN_EINVAL, "horizon must be in 1..65535");
  if (refresh_every < -1) return pbn::set_error(PBN_EINVAL, "refresh_every must be >= -1");
  if (!d_pairs || !d_table) return pbn::set_error(PBN_EINVAL, kNullBuffer);
  if (!d_totals && refresh_every > 0)
    return pbn::set_error(PBN_EINVAL, "d_totals may be null only when refresh_every is -1 or 0");
  if (!aligned(d_totals, 8) || !aligned(d_pairs, 8) || !aligned(d_table, 8))
    return pbn::set_error(PBN_EINVAL, "d_totals, d_pairs and d_table must be 8-byte aligned");
  if (refresh_every == 0) return PBN_OK;      // never due: no launch
  const Table t = table_of(d_table, n_attr);
  hipLaunchKernelGGL(curriculum_refresh_kernel, dim3(1), dim3(kRefreshThreads), 0, (hipStream_t)stream, d_totals, d_pairs,
                     (int)n_attr, (uint32_t)horizon, refresh_every, t.rowcdf, t.cdf, t.total, t.refreshes);
  return launched();
}

}  // extern "C"
