// pbn_episode.hip -- episode statistics kept on the device, one call per frame, so that a captured
// learning frame (and k of them replayed back to back) records what the reference logs on the host:
// RecordEpisodeStatistics' ep_rew_mean / ep_len_mean (ddqn_per/__init__.py:67,357-377) and the BDQ
// loop's ep_len, ep_reward and missed[(state_attractor_id, target_attractor_id)]
// (bdq_model/__init__.py:179-236).
//
//   pbn_episode_begin  opens an episode for every env from its current state and target
//   pbn_episode_track  one frame: every env's return and length move on; the envs whose step was
//                      done close their episode into the aggregates and open the next one.  A second,
//                      single-wave launch then counts the frame and, every log_every frames, copies the
//                      totals into the series ring: after the frame's adds, at a kernel boundary.
//
// The aggregates are int64 and only integer atomics write them, so they do not depend on the order
// of the adds; a return enters them once, at its close, as a fixed-point value (2^-20 units).  Inside
// a wave the closers with equal (source, target) are merged by ballot rounds and the leader of each
// key issues its atomics (pbn_table_insert's merge); the totals take one set of atomics per wave and a
// wave without a closer issues none.  No lane waits for another: there is no fence, flag or spin.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/pbn_env.h"
#include "host_check.h"
#include "net_view.h"
#include "step_parts.h"   // attractor_lookup: the hash function and the probe, stated once

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMergeRounds = 4;      // keys left after these issue their own atomics
constexpr int kTotals = 8;           // frames, episodes, successes, missed, len_sum, ret_sum, last_reward_sum, unpaired
constexpr int kPairFields = 4;       // episodes, missed, len_sum, ret_sum
constexpr int kHistBins = 256;       // bin 255: every length >= 255
constexpr double kFixedOne = 1048576.0;   // 2^20: the unit of the float sums

// what the lookup reads of the net (NetView's hash fields)
struct HashView {
  const uint32_t* tab;
  int bits, probes;
  uint32_t mult[4];
};

struct EnvBuffers {      // the per-env episode state, SoA [n_alloc]
  float* ret;
  uint32_t* len;
  uint8_t* src;
  uint8_t* tgt;
};

using i64 = long long;

__device__ __forceinline__ i64 to_fixed(float v) { return __double2ll_rn((double)v * kFixedOne); }

__device__ __forceinline__ void add64(int64_t* p, i64 v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);   // (two's complement: signed sums)
}

// the sum over the wave, in every lane
__device__ __forceinline__ i64 wave_sum(i64 v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)((unsigned long long)v >> 32), off);
    v += (i64)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

// attractor id of env i's state, or PBN_NO_TARGET: EnvSpec.attractor_id through the step kernels' hash
template <int W>
__device__ __forceinline__ uint32_t source_of(const HashView& h, const uint32_t* __restrict__ state, int64_t n_alloc,
                                              int64_t i) {
  StepArgs a;             // (attractor_lookup reads these four fields only)
  a.hash_bits = h.bits;
  a.hash_probes = h.probes;
#pragma unroll
  for (int w = 0; w < 4; ++w) a.hash_mult[w] = h.mult[w];
  uint32_t sp[W];
#pragma unroll
  for (int w = 0; w < W; ++w) sp[w] = state[(size_t)w * (size_t)n_alloc + (size_t)i];
  const int att = attractor_lookup<W>(a, h.tab, sp);
  return att < 0 ? (uint32_t)PBN_NO_TARGET : (uint32_t)att;
}

template <int W>
__device__ __forceinline__ void open_episode(const HashView& h, const uint32_t* __restrict__ state,
                                             const uint8_t* __restrict__ target, int64_t n_alloc, int64_t i,
                                             const EnvBuffers& e) {
  e.ret[i] = 0.f;
  e.len[i] = 0u;
  e.tgt[i] = target[i];
  e.src[i] = (uint8_t)source_of<W>(h, state, n_alloc, i);
}

template <int W>
__global__ void __launch_bounds__(kThreads) episode_begin_kernel(HashView h, int64_t n_alloc, int64_t n_real,
                                                                 const uint32_t* __restrict__ state,
                                                                 const uint8_t* __restrict__ target, EnvBuffers e) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_real) open_episode<W>(h, state, target, n_alloc, i, e);
}

// Merges the wave's pending lanes of equal key: after kMergeRounds rounds (one distinct key each) the
// leader of every merged key holds its equals' number in count, how many of them are flagged in
// flagged and their sums in v[0..NS); the lanes merged into it drop out; lanes whose key no round
// reached keep their own (1, flag, v).  The numbers are popcounts of ballots; the sums go through
// the lanes only when a key has more than one lane (uniform: the ballot is).  Returns whether this
// lane issues.  Every lane of the wave must call it (ballots).
template <int NS>
__device__ __forceinline__ bool merge_equal(bool pending, uint32_t key, bool flag, i64& count, i64& flagged, i64* v) {
  const int lane = threadIdx.x & (kWave - 1);
  bool issue = pending;
  count = 1;
  flagged = flag ? 1 : 0;
#pragma unroll 1
  for (int round = 0; round < kMergeRounds; ++round) {
    const uint64_t act = __ballot(pending);
    if (act == 0) break;                      // uniform over the wave
    const int leader = __builtin_ctzll(act);
    const uint32_t lk = __shfl(key, leader);
    const bool eq = pending && key == lk;
    const uint64_t same = __ballot(eq);
    const uint64_t same_flagged = __ballot(eq && flag);
    if (same & (same - 1)) {                  // more than one lane holds this key
      i64 s[NS > 0 ? NS : 1];
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] = wave_sum(eq ? v[j] : 0);
      if (lane == leader) {
        count = __popcll(same);
        flagged = __popcll(same_flagged);
#pragma unroll
        for (int j = 0; j < NS; ++j) v[j] = s[j];
      } else if (eq) {
        issue = false;
      }
    }
    if (eq) pending = false;
  }
  return issue;
}

// One thread per env; the grid covers n_alloc, so every lane of every wave reaches the ballots.
template <int W>
__global__ void __launch_bounds__(kThreads) episode_track_kernel(
    HashView h, int n_attr, int64_t n_alloc, int64_t n_real, uint32_t done_mask, const float* __restrict__ reward,
    const uint8_t* __restrict__ flags, const uint32_t* __restrict__ state, const uint8_t* __restrict__ target,
    EnvBuffers e, int64_t* __restrict__ totals, int64_t* __restrict__ pairs, int64_t* __restrict__ hist) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  bool close = false, paired = false;
  uint32_t fl = 0, src = PBN_NO_TARGET, tgt = PBN_NO_TARGET, len = 0;
  float ret = 0.f, last = 0.f;
  if (i < n_real) {
    last = reward[i];
    ret = e.ret[i] + last;
    len = e.len[i] + 1u;
    fl = flags[i];
    close = (fl & done_mask) != 0;
    if (close) {
      src = e.src[i];
      tgt = e.tgt[i];
      paired = src < (uint32_t)n_attr && tgt < (uint32_t)n_attr;
      open_episode<W>(h, state, target, n_alloc, i, e);
    } else {
      e.ret[i] = ret;
      e.len[i] = len;
    }
  }
  const uint64_t closers = __ballot(close);
  if (closers == 0) return;                   // uniform over the wave: it issues no atomic
  const bool success = close && (fl & PBN_FLAG_TERMINATED) != 0;
  const bool miss = close && !success && (fl & PBN_FLAG_TRUNCATED) != 0;
  const i64 c_len = close ? (i64)len : 0, c_ret = close ? to_fixed(ret) : 0, c_last = close ? to_fixed(last) : 0;
  // the totals: lane j adds total 1 + j (total 0, the frames, is the second launch's)
  {
    const i64 t_len = wave_sum(c_len), t_ret = wave_sum(c_ret), t_last = wave_sum(c_last);
    const i64 t_eps = __popcll(closers), t_suc = __popcll(__ballot(success)), t_mis = __popcll(__ballot(miss));
    const i64 t_unp = __popcll(__ballot(close && !paired));
    const i64 mine = lane == 0 ? t_eps : lane == 1 ? t_suc : lane == 2 ? t_mis : lane == 3 ? t_len
                   : lane == 4 ? t_ret : lane == 5 ? t_last : t_unp;
    if (lane < kTotals - 1 && mine != 0) add64(totals + 1 + lane, mine);
  }
  // the length histogram: equal bins merged, one atomic per merged bin
  {
    i64 count, unused;
    const uint32_t bin = len < (uint32_t)(kHistBins - 1) ? len : (uint32_t)(kHistBins - 1);
    if (merge_equal<0>(close, bin, false, count, unused, nullptr)) add64(hist + bin, count);
  }
  // the pairs: equal (source, target) merged, the key's leader issues its four atomics
  if (__ballot(paired) != 0) {
    i64 episodes, missed, sums[2] = {c_len, c_ret};
    if (merge_equal<2>(paired, (src << 8) | tgt, miss, episodes, missed, sums)) {
      int64_t* p = pairs + ((size_t)src * (size_t)n_attr + (size_t)tgt) * kPairFields;
      add64(p + 0, episodes);
      if (missed != 0) add64(p + 1, missed);
      add64(p + 2, sums[0]);
      if (sums[1] != 0) add64(p + 3, sums[1]);
    }
  }
}

// The frame is over (a kernel boundary after the adds): count it, and every log_every frames copy
// the eight totals into the series ring.  One wave; lane j moves total j.
__global__ void __launch_bounds__(kWave) episode_series_kernel(int64_t* __restrict__ totals, int64_t log_every,
                                                               int64_t series_rows, int64_t* __restrict__ series) {
  const int lane = threadIdx.x;
  i64 v = lane < kTotals ? (i64)totals[lane] : 0;
  if (lane == 0) {
    v += 1;
    totals[0] = v;
  }
  const uint32_t lo = __shfl((uint32_t)v, 0), hi = __shfl((uint32_t)((unsigned long long)v >> 32), 0);
  const i64 frames = (i64)(((unsigned long long)hi << 32) | lo);
  if (log_every > 0 && frames % log_every == 0 && lane < kTotals) {
    const i64 row = (frames / log_every - 1) % series_rows;
    series[row * kTotals + lane] = v;
  }
}

using BeginFn = void (*)(HashView, int64_t, int64_t, const uint32_t*, const uint8_t*, EnvBuffers);
using TrackFn = void (*)(HashView, int, int64_t, int64_t, uint32_t, const float*, const uint8_t*, const uint32_t*,
                         const uint8_t*, EnvBuffers, int64_t*, int64_t*, int64_t*);

BeginFn pick_begin(int W) {
  switch (W) {
    case 1: return episode_begin_kernel<1>;
    case 2: return episode_begin_kernel<2>;
    case 3: return episode_begin_kernel<3>;
    case 4: return episode_begin_kernel<4>;
  }
  return nullptr;
}

TrackFn pick_track(int W) {
  switch (W) {
    case 1: return episode_track_kernel<1>;
    case 2: return episode_track_kernel<2>;
    case 3: return episode_track_kernel<3>;
    case 4: return episode_track_kernel<4>;
  }
  return nullptr;
}

using pbn::aligned;

constexpr const char* kNullBuffer = "null buffer";

// what both entry points check of the envs and their episode state; the message, or null
const char* envs_error(int64_t n_alloc, int64_t n_real, const void* d_state, const void* d_target, const void* d_ret,
                       const void* d_len, const void* d_src, const void* d_tgt) {
  if (n_alloc < 32 || (n_alloc & 31) || n_alloc >= ((int64_t)1 << 31))
    return "n_alloc must be a positive multiple of 32 below 2^31";
  if (n_real < 1 || n_real > n_alloc) return "n_real must be in 1..n_alloc";
  if (!d_state || !d_target || !d_ret || !d_len || !d_src || !d_tgt) return kNullBuffer;
  if (!aligned(d_state, 4) || !aligned(d_ret, 4) || !aligned(d_len, 4))
    return "d_state, d_ret and d_len must be 4-byte aligned";
  return nullptr;
}

int view_of(const pbn_net* net, pbn::NetView* v, HashView* h) {
  if (int rc = pbn::check_device(net)) return rc;
  if (int rc = pbn::net_view(net, v)) return rc;
  if (v->W < 1 || v->W > PBN_MAX_NODES / 32) return pbn::set_error(PBN_EINVAL, "the net's state words must be 1..4");
  h->tab = v->att_hash;
  h->bits = v->n_attr ? v->hash_bits : 0;
  h->probes = v->hash_probes;
  for (int w = 0; w < 4; ++w) h->mult[w] = v->hash_mult[w];
  return PBN_OK;
}

int launched() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pbn::set_error(PBN_EDEVICE, hipGetErrorString(e));
  return PBN_OK;
}

}  // namespace

extern "C" {

int pbn_episode_begin(const pbn_net* net, int64_t n_alloc, int64_t n_real, const uint32_t* d_state,
                      const uint8_t* d_target, float* d_ret, uint32_t* d_len, uint8_t* d_src, uint8_t* d_tgt,
                      void* stream) {
  pbn::NetView v;
  HashView h;
  if (int rc = view_of(net, &v, &h)) return rc;
  if (const char* msg = envs_error(n_alloc, n_real, d_state, d_target, d_ret, d_len, d_src, d_tgt))
    return pbn::set_error(PBN_EINVAL, msg);
  const unsigned blocks = (unsigned)((n_real + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(pick_begin(v.W), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, h, n_alloc, n_real,
                     d_state, d_target, EnvBuffers{d_ret, d_len, d_src, d_tgt});
  return launched();
}

int pbn_episode_track(const pbn_net* net, int64_t n_alloc, int64_t n_real, uint32_t done_mask, const float* d_reward,
                      const uint8_t* d_flags, const uint32_t* d_state, const uint8_t* d_target, float* d_ret,
                      uint32_t* d_len, uint8_t* d_src, uint8_t* d_tgt, int64_t* d_totals, int64_t* d_pairs,
                      int64_t* d_hist, int64_t log_every, int64_t series_rows, int64_t* d_series, void* stream) {
  pbn::NetView v;
  HashView h;
  if (int rc = view_of(net, &v, &h)) return rc;
  if (const char* msg = envs_error(n_alloc, n_real, d_state, d_target, d_ret, d_len, d_src, d_tgt))
    return pbn::set_error(PBN_EINVAL, msg);
  if (done_mask == 0 || (done_mask & ~(PBN_FLAG_TERMINATED | PBN_FLAG_TRUNCATED)) != 0)
    return pbn::set_error(PBN_EINVAL, "done_mask must be a non-zero subset of TERMINATED | TRUNCATED");
  if (!d_reward || !d_flags || !d_totals || !d_hist) return pbn::set_error(PBN_EINVAL, kNullBuffer);
  if (!d_pairs && v.n_attr != 0)
    return pbn::set_error(PBN_EINVAL, "d_pairs may be null only when the net has no attractors");
  if (!aligned(d_reward, 4)) return pbn::set_error(PBN_EINVAL, "d_reward must be 4-byte aligned");
  if (!aligned(d_totals, 8) || !aligned(d_pairs, 8) || !aligned(d_hist, 8) || !aligned(d_series, 8))
    return pbn::set_error(PBN_EINVAL, "d_totals, d_pairs, d_hist and d_series must be 8-byte aligned");
  if (log_every < 0) return pbn::set_error(PBN_EINVAL, "log_every must be >= 0");
  if (log_every > 0 && series_rows < 1) return pbn::set_error(PBN_EINVAL, "series_rows must be >= 1 when log_every > 0");
  if (log_every > 0 && !d_series) return pbn::set_error(PBN_EINVAL, "d_series may be null only when log_every is 0");
  const unsigned blocks = (unsigned)(n_alloc / kThreads + (n_alloc % kThreads != 0));
  hipLaunchKernelGGL(pick_track(v.W), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, h, v.n_attr, n_alloc,
                     n_real, done_mask, d_reward, d_flags, d_state, d_target, EnvBuffers{d_ret, d_len, d_src, d_tgt},
                     d_totals, d_pairs, d_hist);
  if (int rc = launched()) return rc;
  hipLaunchKernelGGL(episode_series_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, d_totals, log_every,
                     series_rows, d_series);
  return launched();
}

}  // extern "C"
