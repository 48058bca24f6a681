// step_law.h -- the per-env half of the transition law (DESIGN.md "Step semantics"), stated once
// for every step kernel of step_kernels.h: the bounded draws from the ENV call's 64-bit uniform,
// the random reset state, the perturbation mask from the geometric gaps and their rare tail, the
// step's outcome.  Integer arithmetic only, no StepArgs, LDS or threadIdx: what touches memory
// stays in the kernels, and a host program compiles and calls every function here
// (tests/step_law_check.cpp).  Restated from oracle/pbn_oracle.c: ext64 (ext64), reset_draw
// (pair_draw + start_pick), gap_of (gap_tail's gap functor), the step's epilogue (step_outcome).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pbn_env.h"
#include "philox.h"

namespace pbn {

// floor(a * b / 2^32): one v_mul_hi_u32
__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

__host__ __device__ __forceinline__ uint32_t valid_word_mask(int n, int w) {
  const int bits = n - 32 * w;
  return bits >= 32 ? 0xFFFFFFFFu : (bits <= 0 ? 0u : ((1u << bits) - 1u));
}

// One bounded draw from the 64-bit uniform X = (hi:lo), keeping the rest of X: v =
// floor(X * K / 2^64) in [0, K), X <- X * K mod 2^64 (two v_mad_u64_u32; bias <= K / 2^64;
// oracle/pbn_oracle.c ext64).
__host__ __device__ __forceinline__ uint32_t ext64(uint32_t& hi, uint32_t& lo, uint32_t K) {
  const uint64_t x = (uint64_t)lo * K;
  const uint64_t y = (uint64_t)hi * K + (x >> 32);
  lo = (uint32_t)x;
  hi = (uint32_t)y;
  return (uint32_t)(y >> 32);
}

template <int W>
__host__ __device__ __forceinline__ void set_bit(uint32_t (&g)[W], int pos, int N) {
#pragma unroll
  for (int w = 0; w < W; ++w)
    if ((unsigned)pos < (unsigned)N && (pos >> 5) == w) g[w] |= 1u << (pos & 31);
}

// Three actions uniform on [0, N]: the base-(N+1) digits of c, one draw over (N+1)^3.
// Division by N+1 is a multiply-high by magic = ceil(2^32 / (N+1)), exact for c * (N+1) < 2^32
// (c < (N+1)^3 <= 129^3).  Two divisions: the second quotient is below N+1 (c < (N+1)^3), so it is
// the third digit itself, which the compiler cannot know (a third divide would always return 0).
template <int W>
__host__ __device__ __forceinline__ void actions_from_draw(uint32_t c, int N, uint32_t magic, uint32_t (&m)[W]) {
  const uint32_t n1 = (uint32_t)(N + 1);
  const uint32_t q1 = mulhi32(c, magic), q2 = mulhi32(q1, magic);
  const uint32_t acts[3] = {c - q1 * n1, q1 - q2 * n1, q2};
#pragma unroll
  for (int q = 0; q < 3; ++q) {   // action a in [0, N]: 0 = no-op, else flip node a-1
    const int act = (int)acts[q];
#pragma unroll
    for (int w = 0; w < W; ++w)
      if (act > 0 && ((act - 1) >> 5) == w) m[w] |= 1u << ((act - 1) & 31);
  }
}

// actions_from_draw for one word with N <= 31: action a sets bit a - 1 as 1 << (a - 1), where
// a = 0 shifts by 31 (the shift count's low five bits) onto a bit past the network that `vmask`
// (valid_word_mask(N, 0)) clears once for all three: no per-action guard
__host__ __device__ __forceinline__ uint32_t actions_mask31(uint32_t c, uint32_t n1, uint32_t magic, uint32_t vmask) {
  const uint32_t q1 = mulhi32(c, magic), q2 = mulhi32(q1, magic);   // (two divisions, as above)
  return ((1u << ((c - q1 * n1 - 1u) & 31u)) | (1u << ((q1 - q2 * n1 - 1u) & 31u)) | (1u << ((q2 - 1u) & 31u))) & vmask;
}

// ---- the autoreset pair (reset_draw, first half): one draw c over the A(A-1) ordered (start,
// target != start) pairs, c = as * (A - 1) + rt', rt = rt' + (rt' >= as).  The divide is a
// multiply-high by am1_magic = ceil(2^32 / (A - 1)) (net_image.h; 0: A - 1 == 1).  Two halves, so
// that a loop can place the start attractor (it feeds a table read) ahead of the target.
__host__ __device__ __forceinline__ uint32_t pair_start(uint32_t c, uint32_t am1_magic) {
  return am1_magic ? mulhi32(c, am1_magic) : c;   // c / (A - 1)
}
__host__ __device__ __forceinline__ uint32_t pair_target(uint32_t c, uint32_t as, uint32_t A) {
  uint32_t rt = c - as * (A - 1);
  return rt += (rt >= as) ? 1u : 0u;
}
// (as, rt) drawn from X = (hi:lo); A <= 1: (0, 0) and no draw
__host__ __device__ __forceinline__ void pair_draw(uint32_t& hi, uint32_t& lo, uint32_t A, uint32_t am1_magic,
                                                   uint32_t& as, uint32_t& rt) {
  as = rt = 0;
  if (A >= 2) {
    const uint32_t c = ext64(hi, lo, A * (A - 1));
    as = pair_start(c, am1_magic);
    rt = pair_target(c, as, A);
  }
}

// ---- the start state (reset_draw, second half): the row of the attractor-state table, uniform
// within attractor `as` = [first(as), first(as + 1)).  att_single (every attractor is one state):
// the draw over one state is 0 and leaves X as it is, and state a is attractor a's: no table read.
// xr (X * x_mult mod 2^64, where a caller takes gap 2's uniform off the draws' chain) takes the
// same factor.
template <typename First>
__host__ __device__ __forceinline__ uint32_t start_pick(uint32_t& hi, uint32_t& lo, uint32_t as, bool att_single,
                                                        First first, uint64_t& xr) {
  const int st0 = att_single ? (int)as : (int)first(as);
  uint32_t idx = 0;
  if (!att_single) {
    const uint32_t size = (uint32_t)((int)first(as + 1) - st0);
    idx = ext64(hi, lo, size);
    xr *= size;
  }
  return (uint32_t)st0 + idx;
}

// ---- no attractors: the reset state is RESET call 1 of the env's step, masked to the network's
// nodes (counter words c0, c1, c3 as philox.h's counter map); returns the target, PBN_NO_TARGET
template <int W>
__host__ __device__ __forceinline__ uint32_t random_reset_state(uint32_t c0, uint32_t c1, uint32_t c3, uint32_t k0,
                                                                uint32_t k1, int N, uint32_t (&s)[W]) {
  const Word4 rr = philox(c0, c1, (kStreamReset << 28) | 1u, c3, k0, k1);
  const uint32_t rw4[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
  for (int w = 0; w < W; ++w) s[w] = rw4[w] & valid_word_mask(N, w);
  return PBN_NO_TARGET;
}

// ---- perturbation: flip positions are the prefix sums of geometric gaps from -1, until one passes
// the last node.  The first three gaps' bits; returns p2
template <int W>
__host__ __device__ __forceinline__ int first_gaps_mask(int g0, int g1, int g2, int N, uint32_t (&gam)[W]) {
  const int p0 = g0 - 1, p1 = p0 + g1, p2 = p1 + g2;
  set_bit<W>(gam, p0, N);
  set_bit<W>(gam, p1, N);
  set_bit<W>(gam, p2, N);
  return p2;
}
// one word, N <= 31: a position past the network lands on bits N..31, which vmask (the word mask) clears
__host__ __device__ __forceinline__ int first_gaps_mask31(int g0, int g1, int g2, uint32_t vmask, uint32_t& gam) {
  const int p0 = g0 - 1, p1 = p0 + g1, p2 = p1 + g2;
  gam = ((1u << min((uint32_t)p0, 31u)) | (1u << min((uint32_t)p1, 31u)) | (1u << min((uint32_t)p2, 31u))) & vmask;
  return p2;
}

// The stream word of gap j of update k.  Update 0 (the ENV call's words 0, 1 and u2 are gaps 0-2):
// gap j >= 3 is word jj = j - 3 of the PERT stream.  Update k >= 1: gap j is word jj = j of the
// SETTLE_ENV stream of update k.  Word jj of a stream is word jj & 3 of its call jj >> 2, whose
// counter word 2 is PERT: stream | jj >> 2; SETTLE_ENV: stream | (k-1) << 8 | jj >> 2.
__host__ __device__ __forceinline__ uint32_t gap_call_c2(uint32_t k, int jj) {
  return k == 0 ? ((kStreamPert << 28) | (uint32_t)(jj >> 2))
                : ((kStreamSettleEnv << 28) | ((k - 1) << 8) | (uint32_t)(jj >> 2));
}

// The further gaps of update k, from gap j at position pos (after the three first gaps j = 3,
// pos = p2, P = the update's first call; the whole update j = 0, pos = -1).  call(jj) returns the
// words of the call of stream word jj (counter word 2: gap_call_c2), gap(u) the gap of u (gap_of).
template <int W, typename Call, typename Gap>
__host__ __device__ __forceinline__ void gap_tail(uint32_t k, int j, int pos, int N, Word4 P, Call call, Gap gap,
                                                  uint32_t (&gam)[W]) {
  for (; pos < N - 1; ++j) {
    const int jj = k == 0 ? j - 3 : j;   // gap j's word of its stream
    if ((jj & 3) == 0) P = call(jj);
    const int j4 = jj & 3;
    const uint32_t u = j4 == 0 ? P.x : (j4 == 1 ? P.y : (j4 == 2 ? P.z : P.w));
    pos += gap(u);
    set_bit<W>(gam, pos, N);
  }
}

// gap_tail(0, 3, p2, ...) for a loop that rarely gets there (callers test p2 < N - 1): the fourth
// gap, word 0 of PERT call 0 (P0, which the caller has drawn), in line; gaps 4 and up, about 1e-5
// per env-step at p = 0.01, as gap_tail's rolled loop behind a second unlikely branch.  past(u):
// a cheap sufficient test that gap(u) > N (no position is left for it, whatever p2: no flip, and
// the tail ends) which spares the gap's table read; the bucket table's sentinel bucket (gap_lut),
// or never
template <int W, typename Call, typename Gap, typename Past>
__host__ __device__ __forceinline__ void gap_tail_split(int p2, int N, Word4 P0, Call call, Gap gap, Past past,
                                                        uint32_t (&gam)[W]) {
  if (past(P0.x)) return;
  const int pos = p2 + gap(P0.x);
  set_bit<W>(gam, pos, N);
  if (__builtin_expect(pos < N - 1, 0)) gap_tail<W>(0u, 4, pos, N, P0, call, gap, gam);
}

// ---- the step's outcome from the attractor id of s' (-1: none), the env's target and t; horizon
// 0: none; open: the settle law's last update left s' outside every attractor.  flags: the
// PBN_FLAG_* byte; t saturates at 255 and is 0 after an autoreset.

struct StepOutcome {
  bool term, wrong, trunc, reset;
  uint32_t t, flags;
};
__host__ __device__ __forceinline__ StepOutcome step_outcome(int att, uint32_t target, uint32_t t, int horizon,
                                                             bool autoreset, bool pert, bool open) {
  StepOutcome o;
  const bool in_attr = att >= 0;
  o.term = in_attr && (uint32_t)att == target;
  o.wrong = in_attr && !o.term;
  int tt = (int)t + 1;
  tt = tt > 255 ? 255 : tt;
  o.trunc = horizon > 0 && tt >= horizon;
  o.reset = autoreset && (o.term || o.trunc);
  o.flags = (uint32_t)o.term | ((uint32_t)o.trunc << 1) | ((uint32_t)in_attr << 2) | ((uint32_t)pert << 3) |
            ((uint32_t)o.reset << 4) | ((uint32_t)open << 5);
  o.t = o.reset ? 0u : (uint32_t)tt;
  return o;
}
// the step's reward within the {none, wrong, term, -} row of its action count
__host__ __device__ __forceinline__ int reward_slot(const StepOutcome& o) { return 2 * (int)o.term + (int)o.wrong; }

}  // namespace pbn
