// step_parts.h -- what more than one step kernel uses: the table image's copy, the attractor
// hash, the perturbation gaps, the bit-sliced compare, the 32x32 bit transposes, the function
// evaluation from compact records and leaf selectors, the padded node chain, the settle law's
// per-env selection words and compare.  A helper with one user lives with that user.
#pragma once
#include "step_args.h"
#include "step_debug.h"
#include "wave_util.h"

namespace {

constexpr int kStatePrio = 2;      // s_setprio of the pipelined rollout's state wave

// The LDS table image from global memory, all of a thread's loads issued before its stores
// (four loads in flight per thread, where a load-store loop waits once per element)
__device__ __forceinline__ void copy_image(uint32_t* L, const StepArgs& a) {
  // LDS-DMA (global_load_lds_dwordx4): every wave issues its share of the image at once, with no
  // VGPR round trip; the destination of a wave-instruction is base + 16 B x lane, so wave w
  // moves uint4s [base, base + 64) of each blockDim-wide stripe.  The caller's barrier waits for it.
  const int n4 = a.tab_words >> 2, lane = (int)threadIdx.x & 63;
  const uint4* src = reinterpret_cast<const uint4*>(a.tab);
  for (int base = (int)threadIdx.x - lane; base < n4; base += (int)blockDim.x) {
    if (base + lane < n4)
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src + base + lane),
                                       (__attribute__((address_space(3))) void*)(L + 4 * base), 16, 0, 0);
  }
}

// LDS hash of the attractor states, slot-major: slot s holds its key words at [s * HS, s * HS +
// W) and the attractor id (0xFFFFFFFF: empty) at s * HS + W, HS = W + 1 rounded up to a power
// of two, so that one probe is one ds_read_b64 (W = 1) or ds_read_b128 (W = 2, 3)
template <int W>
struct HashStride {
  static constexpr int value = hash_stride(W);
};

// attractor id of the state sp at slot s, or -1
template <int W>
__device__ __forceinline__ int hash_probe(const uint32_t* __restrict__ htab, uint32_t s, const uint32_t (&sp)[W]) {
  constexpr int HS = HashStride<W>::value;
  const uint32_t* e = htab + (size_t)s * HS;
  uint32_t ent[HS];
  if constexpr (HS == 2) {
    const uint2 v = *reinterpret_cast<const uint2*>(e);
    ent[0] = v.x; ent[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < HS / 4; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(e)[q];
      ent[4 * q] = v.x; ent[4 * q + 1] = v.y; ent[4 * q + 2] = v.z; ent[4 * q + 3] = v.w;
    }
  }
  bool eq = ent[W] != 0xFFFFFFFFu;
#pragma unroll
  for (int w = 0; w < W; ++w) eq = eq && ent[w] == sp[w];
  return eq ? (int)ent[W] : -1;
}

// gap(u) = min{m in 1..N : u < C[m-1]} (N+1 or more if none); C padded with 0xFFFFFFFF.
__device__ __forceinline__ int gap_of(const uint32_t* __restrict__ cdf, int len, uint32_t u) {
  int cnt = 0;
  for (int s = len >> 1; s >= 1; s >>= 1)
    if (cdf[cnt + s - 1] <= u) cnt += s;
  if (cdf[cnt] <= u) cnt += 1;
  return cnt + 1;
}

// lanes-of-32-envs bit mask of (u < c), u = digits dig[0..B) MSB first (B = prob_bits).
// From the least significant digit up: lt' = c_d ? (u_d ? lt : 1) : (u_d ? 0 : lt),
// one v_bitop3_b32 per digit over (u_d, lt, C_d) with LUT 0x8E.
__device__ __forceinline__ uint32_t less_than(const uint32_t (&dig)[16], uint32_t c, int B) {
  uint32_t lt = 0;
#pragma unroll
  for (int d = 15; d >= 0; --d) {
    if (d < B) {
      const uint32_t C = (uint32_t)__builtin_amdgcn_sbfe((int)c, B - 1 - d, 1);
      lt = __builtin_amdgcn_bitop3_b32(dig[d], lt, C, 0x8E);
    }
  }
  return lt;
}

// y = a of lane ^ J (J in 1, 2, 4, 8, 16), within 32-lane halves, without LDS
// ~0 on lanes with bit J of the lane index set, else 0 (a VGPR value: selecting with it
// needs no exec mask or SGPR pair, which the step loops cannot spare)
template <int J>
__device__ __forceinline__ uint32_t lane_bit_mask(int lane) {
  return 0u - (uint32_t)((lane & J) != 0);
}

// (every lane's DPP source is inside its row for these controls, so each lane is written and
// the "old" operand is never used: mov_dpp leaves it undefined, which saves the v_mov that
// update_dpp(0, ...) spends initialising the destination)
template <int J>
__device__ __forceinline__ uint32_t xor_lane(uint32_t a, int lane) {
  if constexpr (J == 1) {
    return __builtin_amdgcn_mov_dpp(a, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
  } else if constexpr (J == 2) {
    return __builtin_amdgcn_mov_dpp(a, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
  } else if constexpr (J == 4) {
    const uint32_t r4 = __builtin_amdgcn_mov_dpp(a, 0x124, 0xF, 0xF, true);   // row_ror:4
    const uint32_t r12 = __builtin_amdgcn_mov_dpp(a, 0x12C, 0xF, 0xF, true);  // row_ror:12
    return pbn::bfi3(lane_bit_mask<4>(lane), r4, r12);
  } else if constexpr (J == 8) {
    return __builtin_amdgcn_mov_dpp(a, 0x128, 0xF, 0xF, true);  // row_ror:8
  } else {
    const auto r = __builtin_amdgcn_permlane16_swap(a, a, false, false);
    return pbn::bfi3(lane_bit_mask<16>(lane), r[0], r[1]);
  }
}

// one butterfly stage: lanes without bit J keep their M bits and take the partner's M bits
// shifted up by J; lanes with bit J take the partner's ~M bits shifted down.  Branch-free: the
// shift is a per-lane rotate (v_alignbit_b32; wrapped bits land outside the kept field) and
// the field a per-lane mask.
template <int J>
__device__ __forceinline__ uint32_t transpose_step(uint32_t a, int lane) {
  constexpr uint32_t M = J == 16 ? 0x0000FFFFu : (J == 8 ? 0x00FF00FFu : (J == 4 ? 0x0F0F0F0Fu : (J == 2 ? 0x33333333u : 0x55555555u)));
  const uint32_t y = xor_lane<J>(a, lane);
  const uint32_t up = lane_bit_mask<J>(lane);
  const uint32_t rot = __builtin_amdgcn_alignbit(y, y, (32u - J) ^ (up & ((32u - J) ^ (uint32_t)J)));
  return pbn::bfi3(M ^ ~up, rot, a);
}

// the partner value of lane ^ J within 32-lane halves through the LDS crossbar (ds_swizzle,
// bit mode: and 0x1F, xor J): no VALU issue slot, where DPP cannot cross rows of 16 lanes
template <int J>
__device__ __forceinline__ uint32_t swizzle_xor(uint32_t a) {
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)a, (J << 10) | 0x1F);
}

// byte-granular stages (J = 16, 8) as one v_perm_b32 with a per-lane selector: the shift and
// the field select of transpose_step in one instruction.  perm(y, a, sel): bytes 0-3 are a's,
// 4-7 the partner's.
//   J = 16: low lanes [a0 a1 y0 y1], high lanes [y2 y3 a2 a3]
//   J = 8:  low lanes [a0 y0 a2 y2], high lanes [y1 a1 y3 a3]
template <int J>
__device__ __forceinline__ uint32_t perm_sel(int lane) {
  if constexpr (J == 16) return (lane & 16) ? 0x03020706u : 0x05040100u;
  else return (lane & 8) ? 0x03070105u : 0x06020400u;
}

// lane k holds row k of a 32x32 bit matrix (per 32-lane half); afterwards lane c holds column c.
// 11 VALU (J = 16: swizzle + perm; 8: DPP + perm; 4: swizzle + alignbit + bitop3; 2, 1: DPP +
// alignbit + bitop3) where five transpose_step spend 20.
__device__ __forceinline__ uint32_t lane_transpose32(uint32_t a, int lane) {
  a = __builtin_amdgcn_perm(swizzle_xor<16>(a), a, perm_sel<16>(lane));
  a = __builtin_amdgcn_perm(xor_lane<8>(a, lane), a, perm_sel<8>(lane));
  {
    const uint32_t y = swizzle_xor<4>(a);
    const uint32_t up = lane_bit_mask<4>(lane);
    const uint32_t rot = __builtin_amdgcn_alignbit(y, y, 28u ^ (up & (28u ^ 4u)));
    a = pbn::bfi3(0x0F0F0F0Fu ^ ~up, rot, a);
  }
  a = transpose_step<2>(a, lane);
  a = transpose_step<1>(a, lane);
  return a;
}

// eval of a lane-varying function from its compact record: 4 input planes, 16-bit
// truth table T; leaf masks are sign-extended table bits (v_bfe_i32).
__device__ __forceinline__ uint32_t eval_compact(uint32_t ins, uint32_t T, const uint32_t* __restrict__ S) {
  const uint32_t x0 = S[ins & 0xFFu], x1 = S[(ins >> 8) & 0xFFu], x2 = S[(ins >> 16) & 0xFFu], x3 = S[ins >> 24];
  uint32_t v[8];
#pragma unroll
  for (int mm = 0; mm < 8; ++mm) {
    const uint32_t l0 = (uint32_t)__builtin_amdgcn_sbfe((int)T, 2 * mm, 1);
    const uint32_t l1 = (uint32_t)__builtin_amdgcn_sbfe((int)T, 2 * mm + 1, 1);
    v[mm] = bfi(x0, l1, l0);
  }
  const uint32_t w0 = bfi(x1, v[1], v[0]), w1 = bfi(x1, v[3], v[2]), w2 = bfi(x1, v[5], v[4]), w3 = bfi(x1, v[7], v[6]);
  return bfi(x3, bfi(x2, w3, w2), bfi(x2, w1, w0));
}

// eval from per-lane leaf selectors: leaf m = (T bit 2m, T bit 2m+1) = (value at x0 = 0,
// value at x0 = 1) is one of {0, x0, ~x0, ~0}, i.e. per byte one v_perm_b32 of {~x0 : x0}
// with selector byte j, 4 + j, 12 (0x00) or 13 (0xFF); the selectors are built on the host.
__device__ __forceinline__ uint32_t eval_sel(uint32_t ins, uint4 sa, uint4 sb, const uint32_t* __restrict__ S) {
  const uint32_t x0 = S[ins & 0xFFu], x1 = S[(ins >> 8) & 0xFFu], x2 = S[(ins >> 16) & 0xFFu], x3 = S[ins >> 24];
  const uint32_t nx0 = ~x0;
  const uint32_t v0 = __builtin_amdgcn_perm(nx0, x0, sa.x), v1 = __builtin_amdgcn_perm(nx0, x0, sa.y);
  const uint32_t v2 = __builtin_amdgcn_perm(nx0, x0, sa.z), v3 = __builtin_amdgcn_perm(nx0, x0, sa.w);
  const uint32_t v4 = __builtin_amdgcn_perm(nx0, x0, sb.x), v5 = __builtin_amdgcn_perm(nx0, x0, sb.y);
  const uint32_t v6 = __builtin_amdgcn_perm(nx0, x0, sb.z), v7 = __builtin_amdgcn_perm(nx0, x0, sb.w);
  const uint32_t w0 = bfi(x1, v1, v0), w1 = bfi(x1, v3, v2), w2 = bfi(x1, v5, v4), w3 = bfi(x1, v7, v6);
  return bfi(x3, bfi(x2, w3, w2), bfi(x2, w1, w0));
}

// eval_sel with the four input planes already read
__device__ __forceinline__ uint32_t eval_sel_in(const uint32_t (&x)[4], uint4 sa, uint4 sb) {
  const uint32_t x0 = x[0], nx0 = ~x0;
  const uint32_t v0 = __builtin_amdgcn_perm(nx0, x0, sa.x), v1 = __builtin_amdgcn_perm(nx0, x0, sa.y);
  const uint32_t v2 = __builtin_amdgcn_perm(nx0, x0, sa.z), v3 = __builtin_amdgcn_perm(nx0, x0, sa.w);
  const uint32_t v4 = __builtin_amdgcn_perm(nx0, x0, sb.x), v5 = __builtin_amdgcn_perm(nx0, x0, sb.y);
  const uint32_t v6 = __builtin_amdgcn_perm(nx0, x0, sb.z), v7 = __builtin_amdgcn_perm(nx0, x0, sb.w);
  const uint32_t w0 = bfi(x[1], v1, v0), w1 = bfi(x[1], v3, v2), w2 = bfi(x[1], v5, v4), w3 = bfi(x[1], v7, v6);
  return bfi(x[3], bfi(x[2], w3, w2), bfi(x[2], w1, w0));
}

// gap(u) = min{m : u < C[m-1]} from a float estimate of log(1-x)/log(1-p) corrected
// exactly (+-1) against the integer CDF in LDS; C padded with 0xFFFFFFFF.
__device__ __forceinline__ int gap_est(const uint32_t* __restrict__ cdf, int len, float inv_log2q, uint32_t u) {
  const float x = (float)u * 2.3283064365386963e-10f;   // u / 2^32
  const float l2 = __builtin_amdgcn_logf(1.0f - x);     // v_log_f32: log2
  float est = floorf(l2 * inv_log2q) + 1.0f;
  est = fminf(fmaxf(est, 1.0f), (float)len);
  int g = (int)est;
  // C[g-2] and C[g-1] as one pair of adjacent reads (no branch: g == 1 reads C[0], C[1])
  const int base = g >= 2 ? g - 2 : 0;
  const uint32_t c0 = cdf[base], c1 = cdf[base + 1];
  const uint32_t hi = g >= 2 ? c1 : c0;                 // C[g-1]
  const uint32_t lo = g >= 2 ? c0 : 0u;                 // C[g-2]
  g += (u >= hi) ? 1 : 0;
  g -= (g >= 2 && u < lo) ? 1 : 0;
  return g;
}

// gap(u) from the bucket table: within a bucket of u (its top bits) the gap takes at most two
// values, lo and lo + 1, split at threshold C[lo-1]; buckets from C[N-1] on share one sentinel
// entry (gap N+1, no flip).  One LDS read and two VALU ops, where gap_est spends ~22.
__device__ __forceinline__ int gap_lut(const uint2* __restrict__ lut, int shift, int nb, uint32_t u) {
  const uint32_t b = min(u >> shift, (uint32_t)nb);
  const uint2 e = lut[b];
  return (int)e.y + (u >= e.x ? 1 : 0);
}

// one gap by the net's method (mode: 0 estimate, 1 binary search, 2 bucket table)
__device__ __forceinline__ int gap_any(int mode, const uint32_t* __restrict__ L, const StepArgs& a, uint32_t u) {
  if (mode == 2) return gap_lut(reinterpret_cast<const uint2*>(L + a.gap_lut_off), a.gap_shift, a.gap_nb, u);
  return mode ? gap_of(L, a.cdf_len, u) : gap_est(L, a.cdf_len, a.inv_log2q, u);
}

// an update's first three gaps, which are independent: computed side by side by one method
__device__ __forceinline__ void first_gaps(int mode, const uint32_t* __restrict__ L, const StepArgs& a, uint32_t u0,
                                           uint32_t u1, uint32_t u2, int& g0, int& g1, int& g2) {
  if (mode == 2) {
    g0 = gap_any(2, L, a, u0); g1 = gap_any(2, L, a, u1); g2 = gap_any(2, L, a, u2);
  } else if (mode) {
    g0 = gap_of(L, a.cdf_len, u0); g1 = gap_of(L, a.cdf_len, u1); g2 = gap_of(L, a.cdf_len, u2);
  } else {
    g0 = gap_est(L, a.cdf_len, a.inv_log2q, u0);
    g1 = gap_est(L, a.cdf_len, a.inv_log2q, u1);
    g2 = gap_est(L, a.cdf_len, a.inv_log2q, u2);
  }
}

// attractor id of the per-env state sp (open-addressing LDS hash; keys are unique, so the probe
// order does not matter: the first four probes are read side by side), or -1
template <int W>
__device__ __forceinline__ int attractor_lookup(const StepArgs& a, const uint32_t* __restrict__ htab,
                                                const uint32_t (&sp)[W]) {
  int att = -1;
  if (a.hash_bits > 0) {
    PBN_ISA_ARM("hash");
    const uint32_t hmask = (1u << a.hash_bits) - 1u;
    uint32_t h = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) h += sp[w] * a.hash_mult[w];
    h >>= (32 - a.hash_bits);
    // the first probe always (h < 2^bits needs no mask); the table is usually collision free
    // (hash_probes = 1: every bundled network), so the others sit behind a uniform branch
    att = hash_probe<W>(htab, h, sp);
    if (a.hash_probes > 1) {
      PBN_ISA_ARM("hash_more_probes");
      for (int pr = 1; pr < a.hash_probes; ++pr) {
        const int id = hash_probe<W>(htab, (h + pr) & hmask, sp);
        if (id >= 0) att = id;
      }
    }
  }
  return att;
}

// The settle law's per-env selection (oracle/pbn_oracle.c env_uniforms): the 16 words of env
// ge's SETTLE_SEL calls 4r .. 4r+3 for update k; node 32r + b's 16-bit field is b & 1 of
// U[b >> 1].  Calls past the network's last node are not made (U = 0).
// XM: xor-ed into words 0 and 2 of every call (philox's last-round keys; settle_lt_word_pk's bias)
template <uint32_t XM = 0u>
__device__ __forceinline__ void settle_sel_words(uint32_t ge_lo, uint32_t ge_hi, uint32_t st_lo, uint32_t k, int r,
                                                 int N, uint32_t k0, uint32_t k1, uint32_t (&U)[16]) {
  const uint32_t c2 = (pbn::kStreamSettleSel << 28) | (k << 8) | (uint32_t)(4 * r);
  if (32 * r + 24 < N) {   // every call (a word of more than 24 nodes): in one block, interleaved
    PBN_ISA_ARM("sel_all_calls");
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const Word4 P = pbn::philox<pbn::kPhiloxRounds, XM>(ge_lo, st_lo, c2 | (uint32_t)c, ge_hi, k0, k1);
      U[4 * c + 0] = P.x; U[4 * c + 1] = P.y; U[4 * c + 2] = P.z; U[4 * c + 3] = P.w;
    }
  } else {
    PBN_ISA_ARM("sel_some_calls");
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      Word4 P = {0u, 0u, 0u, 0u};
      if (32 * r + 8 * c < N) P = pbn::philox<pbn::kPhiloxRounds, XM>(ge_lo, st_lo, c2 | (uint32_t)c, ge_hi, k0, k1);
      U[4 * c + 0] = P.x; U[4 * c + 1] = P.y; U[4 * c + 2] = P.z; U[4 * c + 3] = P.w;
    }
  }
}

// env-major selection word of one threshold: bit b = (field of node 32r + b < C[b]), C = the
// thresholds scaled to 16 bits (c << (16 - B); 65536 past a node's last function: sthr), most
// significant node first.  Per node one subtract (the field selected by SDWA) whose sign is the
// compare (both operands <= 2^16) and one v_alignbit_b32 that shifts it in: (lt:d) >> 31.  C is
// read through the constant address space, so the 32 thresholds of a row are scalar loads.
using ConstU32 = const __attribute__((address_space(4))) uint32_t;
__device__ __forceinline__ uint32_t settle_lt_word(const uint32_t (&U)[16], const uint32_t* C_) {
  ConstU32* C = (ConstU32*)C_;
  uint32_t lt = 0;
#pragma unroll
  for (int b = 31; b >= 0; --b) {
    const uint32_t u = (b & 1) ? (U[b >> 1] >> 16) : (U[b >> 1] & 0xFFFFu);
    lt = __builtin_amdgcn_alignbit(lt, u - C[b], 31);
  }
  return lt;
}

// input plane k of a record's input word: byte k is a plane index, or with BY (the pipelined
// kernel's LDS records for W <= 2) the plane's byte offset, so that the address is one add of
// a byte field (v_add_u32 with an SDWA byte select) instead of extract + shift-add
template <bool BY>
__device__ __forceinline__ uint32_t plane_in(const uint32_t* __restrict__ S, uint32_t ins, int k) {
  const uint32_t f = k == 3 ? ins >> 24 : (ins >> (8 * k)) & 0xFFu;
  if constexpr (BY) return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(S) + f);
  else return S[f];
}

// chain over padded records (every node has max_nf <= kNodeRecs records, the last function
// repeated; lanes past N have all-zero selectors and evaluate to 0): x = F_{K-1}; x = lt_q ? F_q
// : x, with no per-lane function count
template <int K, bool BY>
__device__ __forceinline__ uint32_t chain_padded(const uint4* __restrict__ rec, const uint4* __restrict__ sel,
                                                 int stride, const uint32_t* __restrict__ S,
                                                 const uint32_t* __restrict__ lt, int lt_stride) {
  uint32_t xin[K][4], ltv[K];
  uint4 sa[K], sb[K];
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const uint32_t ins = rec[q * stride].x;
#pragma unroll
    for (int k = 0; k < 4; ++k) xin[q][k] = plane_in<BY>(S, ins, k);
    sa[q] = sel[(2 * q) * stride];
    sb[q] = sel[(2 * q + 1) * stride];
    ltv[q] = q < K - 1 ? lt[q * lt_stride] : 0u;
  }
  uint32_t x = 0;
#pragma unroll
  for (int q = K - 1; q >= 0; --q) {
    const uint32_t fj = eval_sel_in(xin[q], sa[q], sb[q]);
    x = (q == K - 1) ? fj : bfi(ltv[q], fj, x);
  }
  return x;
}

}  // namespace
