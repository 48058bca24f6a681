// philox.h -- Philox4x32-R (Salmon et al., SC'11 / Random123) for gfx950.  Every stream draws
// Philox4x32-7 (kPhiloxRounds, DESIGN.md "RNG"): seven rounds is the smallest round count of
// Philox4x32 with no TestU01 BigCrush failure in the paper (Random123 defaults to 10 for a
// three-round safety margin).  The round function is pinned at 10 rounds by rocRAND's engine and
// at 7 and 10 by Random123's published known-answer vectors (tests/test_philox.py).
//
// One round: two 32x32->64 products (v_mad_u64_u32), two 3-input xors
// (v_xor3_b32); the key schedule is wave-uniform and lives in SGPRs.
// Counter map (DESIGN.md "RNG stream map"):
//   ctr = (lo32(id), lo32(step), stream << 28 | idx, hi16(id) | hi16(step) << 16)
//   key = (lo32(seed), hi32(seed))
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbn {

// EXPLORE = 4: epsilon-greedy draws of pbn_q_to_flipmask (per env; word 0 = explore test,
// word k + 1 = branch k's random action, by multiply-high); SETTLE_SEL = 5 (per env: node i's
// selection uniform of update k is 16-bit field i & 7 of call (k << 8) | (i >> 3)) and
// SETTLE_ENV = 6 (per env): updates k >= 1 of a step under the settle law (settle_updates);
// REPLAY = 7: the learner's replay rows (pbn_replay_advance: id = row of the batch, step = draw);
// CURRICULUM = 8: the weighted restart of an env that the step reset (curriculum_law.h: call 0 of
// the env at the step's index).  The stream field has four bits.
enum : uint32_t {
  kStreamSel = 0, kStreamEnv = 1, kStreamPert = 2, kStreamReset = 3, kStreamExplore = 4,
  kStreamSettleSel = 5, kStreamSettleEnv = 6, kStreamReplay = 7, kStreamCurriculum = 8
};

struct Word4 {
  uint32_t x, y, z, w;
};

// a ^ b ^ c in one v_bitop3_b32 (gfx950; LUT 0x96 = 3-input xor)
__host__ __device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}

constexpr int kPhiloxRounds = 7;

// ctr = (c0, c1, c2, c3), key = (k0, k1); one round: two 32x32->64 products, two 3-input xors,
// the Weyl key bump (SALU: the key is wave-uniform).  XM (default 0) is xor-ed into output words
// 0 and 2 for free, through the last round's keys (the settle law's packed compares bias them).
template <int R = kPhiloxRounds, uint32_t XM = 0u>
__host__ __device__ __forceinline__ Word4 philox(uint32_t c0, uint32_t c1, uint32_t c2,
                                                  uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, r == R - 1 ? (k0 ^ XM) : k0);
    const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, r == R - 1 ? (k1 ^ XM) : k1);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Word4{c0, c1, c2, c3};
}

// The key schedule of philox<R> on its own: rk0[r], rk1[r] = the keys of round r (k + r * Weyl
// constant, modulo 2^32).  It depends on the seed alone, so a loop that draws every step builds it
// once in front of the loop instead of once per call (pbn_rollout_pipe's RNG waves).
template <int R = kPhiloxRounds>
__host__ __device__ __forceinline__ void philox_round_keys(uint32_t k0, uint32_t k1, uint32_t (&rk0)[R],
                                                            uint32_t (&rk1)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    rk0[r] = k0;
    rk1[r] = k1;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// philox<R, XM> with the round keys of philox_round_keys given: the same round function, no key
// bump inside
template <int R = kPhiloxRounds, uint32_t XM = 0u>
__host__ __device__ __forceinline__ Word4 philox_rk(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                     const uint32_t (&rk0)[R], const uint32_t (&rk1)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, r == R - 1 ? (rk0[r] ^ XM) : rk0[r]);
    const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, r == R - 1 ? (rk1[r] ^ XM) : rk1[r]);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  return Word4{c0, c1, c2, c3};
}

// The part of philox_rk's first three rounds that does not depend on counter word 1.  A loop that
// calls with (c0, c2, c3) and the key fixed and only c1 (the step's low word) moving builds it once
// in front of the loop (pbn_rollout_pipe's RNG waves).  With one round written as
//   n0 = hi(M1 * c2) ^ c1 ^ k0,  n2 = hi(M0 * c0) ^ c3 ^ k1,  c1' = lo(M1 * c2),  c3' = lo(M0 * c0)
// and (a, b, d) the counters after rounds 1, 2, 3:
//   round 1: both products are fixed; a0 = A ^ c1, and a1, a2, a3 are fixed;
//   round 2: M1 * a2 is fixed, so b0 and b1 are; b2 = hi(M0 * a0) ^ B, b3 = lo(M0 * a0);
//   round 3: M0 * b0 is fixed, so d3 is; d0 = hi(M1 * b2) ^ D, d1 = lo(M1 * b2), d2 = b3 ^ E.
// B and D depend on (c0, c3) and the key only: calls that differ in c2 alone share them.
struct PhiloxPrefix {
  uint32_t A, B, D, E, d3;
};

template <int R = kPhiloxRounds>
__host__ __device__ __forceinline__ PhiloxPrefix philox_prefix(uint32_t c0, uint32_t c2, uint32_t c3,
                                                                const uint32_t (&rk0)[R], const uint32_t (&rk1)[R]) {
  static_assert(R >= 4, "the prefix covers rounds 1-3; the last round's XM belongs to the tail");
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t a1 = (uint32_t)p1, a3 = (uint32_t)p0;
  const uint32_t a2 = xor3((uint32_t)(p0 >> 32), c3, rk1[0]);
  const uint64_t q1 = (uint64_t)0xCD9E8D57u * a2;
  const uint32_t b0 = xor3((uint32_t)(q1 >> 32), a1, rk0[1]);
  const uint64_t s0 = (uint64_t)0xD2511F53u * b0;
  PhiloxPrefix pre;
  pre.A = (uint32_t)(p1 >> 32) ^ rk0[0];
  pre.B = a3 ^ rk1[1];
  pre.D = (uint32_t)q1 ^ rk0[2];
  pre.E = (uint32_t)(s0 >> 32) ^ rk1[2];
  pre.d3 = (uint32_t)s0;
  return pre;
}

// The prefix of the call that differs from `of`'s in counter word 2 alone: its own A, E and d3
// beside `of`'s B and D, so a loop that pins both prefixes holds three more values, not five
// (the env-draw wave's PERT call 0 beside its ENV call; sel_fast holds its CPN calls the same way)
template <int R = kPhiloxRounds>
__host__ __device__ __forceinline__ PhiloxPrefix philox_prefix_sibling(const PhiloxPrefix& of, uint32_t c0, uint32_t c2,
                                                                        uint32_t c3, const uint32_t (&rk0)[R],
                                                                        const uint32_t (&rk1)[R]) {
  const PhiloxPrefix own = philox_prefix(c0, c2, c3, rk0, rk1);
  return PhiloxPrefix{own.A, of.B, of.D, own.E, own.d3};
}

// philox_rk<R, XM>(c0, c1, c2, c3, rk0, rk1) from the prefix of (c0, c2, c3): one xor, one product
// and one xor, one product and two xors, then rounds 4..R as they are
template <int R = kPhiloxRounds, uint32_t XM = 0u>
__host__ __device__ __forceinline__ Word4 philox_tail(const PhiloxPrefix& pre, uint32_t c1,
                                                       const uint32_t (&rk0)[R], const uint32_t (&rk1)[R]) {
  static_assert(R >= 4, "the prefix covers rounds 1-3; the last round's XM belongs to the tail");
  const uint64_t p = (uint64_t)0xD2511F53u * (pre.A ^ c1);
  const uint64_t q = (uint64_t)0xCD9E8D57u * ((uint32_t)(p >> 32) ^ pre.B);
  uint32_t c0 = (uint32_t)(q >> 32) ^ pre.D;
  c1 = (uint32_t)q;
  uint32_t c2 = (uint32_t)p ^ pre.E;
  uint32_t c3 = pre.d3;
#pragma unroll
  for (int r = 3; r < R; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, r == R - 1 ? (rk0[r] ^ XM) : rk0[r]);
    const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, r == R - 1 ? (rk1[r] ^ XM) : rk1[r]);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  return Word4{c0, c1, c2, c3};
}

__host__ __device__ __forceinline__ Word4 draw(uint64_t seed, uint64_t id, uint64_t step,
                                                uint32_t stream, uint32_t idx) {
  return philox((uint32_t)id, (uint32_t)step, (stream << 28) | (idx & 0x0FFFFFFFu),
                       (uint32_t)((id >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16),
                       (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace pbn
