// curriculum_law.h -- the curriculum reset law (DESIGN.md "Curriculum resets"), stated once for the
// kernels of pbn_curriculum.hip and for a host program (tests/curriculum_law_check.cpp): the weight
// of a (source, target) pair from its episode statistics, the table's layout, and the draw of a
// restart (start attractor, target, start state) from one CURRICULUM Philox call.  Integer
// arithmetic only; what touches memory is handed in as functors, as step_law.h's start_pick does.
//
// The table (one caller-owned buffer, pbn_curriculum_table_bytes(A) bytes, 8-byte aligned):
//   uint64 rowcdf[A]     inclusive prefix sums of the rows' totals
//   uint32 cdf[A][A]     row s: inclusive prefix sums of w[s][.]   (padded to a multiple of 8 bytes)
//   uint64 total         rowcdf[A - 1], below 2^40
//   uint64 refreshes     how often pbn_curriculum_refresh rebuilt the table
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace pbn {

constexpr int kCurriculumMinAttr = 2, kCurriculumMaxAttr = 254;
constexpr uint32_t kCurriculumWeightCap = (1u << 24) - 1u;   // 254 * 2^24 < 2^32: a row's sum fits uint32
constexpr int kCurriculumShift = 8;                          // weights count 2^-8 steps
constexpr int kStatPairFields = 4;                               // pairs[s][t]: episodes, missed, len_sum, ret_sum

// byte offsets into the table
__host__ __device__ inline int64_t curriculum_cdf_offset(int A) { return 8 * (int64_t)A; }
__host__ __device__ inline int64_t curriculum_total_offset(int A) {
  return curriculum_cdf_offset(A) + ((4 * (int64_t)A * A + 7) & ~(int64_t)7);
}
__host__ __device__ inline int64_t curriculum_refreshes_offset(int A) { return curriculum_total_offset(A) + 8; }
__host__ __device__ inline int64_t curriculum_table_bytes(int A) { return curriculum_refreshes_offset(A) + 8; }

// floor(a * b / 2^64)
__host__ __device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The facade's rule (env.py PBNEnv.pair_weights), (horizon + sum of lengths) / (1 + episodes), in
// units of 2^-8 and capped: H = the spec's horizon or 20, L = pairs[s][t].len_sum, E = .episodes.
// Every episode has a step and H >= 1, so an off-diagonal weight is >= 256.
__host__ __device__ __forceinline__ uint32_t curriculum_weight(uint32_t H, uint64_t L, uint64_t E, bool diagonal) {
  if (diagonal) return 0u;
  const uint64_t q = (((uint64_t)H + L) << kCurriculumShift) / (1u + E);
  return q < kCurriculumWeightCap ? (uint32_t)q : kCurriculumWeightCap;
}
__host__ __device__ __forceinline__ uint32_t curriculum_weight_of(uint32_t H, const int64_t* pairs, int A, int s, int t) {
  const int64_t* p = pairs + ((size_t)s * (size_t)A + (size_t)t) * kStatPairFields;
  return curriculum_weight(H, (uint64_t)p[2], (uint64_t)p[0], s == t);
}

// min{i in [0, n) : at(i) > v}, for a non-decreasing at with at(n - 1) > v: a binary search of
// ceil(log2 n) steps, 8 for n <= 254 (at(n - 1) is never read)
template <typename T, typename At>
__host__ __device__ __forceinline__ int first_above(int n, T v, At at) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (at(mid) > v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The restart of one env from x = draw(seed, env id, step, CURRICULUM, 0): the start attractor s
// with probability (row s's total) / total, the target t != s with probability w[s][t] / (row s's
// total) -- a diagonal entry repeats its left neighbour's prefix sum (or is 0), so no search stops
// on it -- and the row of the attractor-state table, uniform within attractor s as step_law.h's
// start_pick is.  rowcdf(i), cdf(s, j): the table; first(a): the attractor-state table's att_start.
struct CurriculumDraw {
  uint32_t s, t, row;
};
template <typename RowCdf, typename Cdf, typename First>
__host__ __device__ __forceinline__ CurriculumDraw curriculum_draw(const Word4& x, int A, uint64_t total, RowCdf rowcdf,
                                                                   Cdf cdf, First first) {
  CurriculumDraw d;
  const uint64_t v = mulhi64(((uint64_t)x.y << 32) | x.x, total);
  const int s = first_above<uint64_t>(A, v, rowcdf);
  const uint32_t vs = (uint32_t)(v - (s > 0 ? (uint64_t)rowcdf(s - 1) : 0u));   // below row s's total < 2^32
  const int t = first_above<uint32_t>(A, vs, [&](int j) { return cdf(s, j); });
  const uint32_t st0 = (uint32_t)first(s), size = (uint32_t)first(s + 1) - st0;
  d.s = (uint32_t)s;
  d.t = (uint32_t)t;
  d.row = st0 + (uint32_t)mulhi64(((uint64_t)x.w << 32) | x.z, size);
  return d;
}

// The whole table from pairs [A][A][4], in order (the host's statement; pbn_curriculum_refresh
// computes the same integers with wave scans).  Returns total.
inline uint64_t curriculum_build(int A, uint32_t H, const int64_t* pairs, uint64_t* rowcdf, uint32_t* cdf) {
  uint64_t total = 0;
  for (int s = 0; s < A; ++s) {
    uint32_t row = 0;
    for (int t = 0; t < A; ++t) cdf[(size_t)s * A + t] = row += curriculum_weight_of(H, pairs, A, s, t);
    rowcdf[s] = total += row;
  }
  return total;
}

}  // namespace pbn
