// rollout_settle.h -- pbn_rollout_settle, the pipelined rollout under the settle law, and what it
// alone uses: the packed two-node compares, the output rows' pointers (StageOut) and the per-env
// update plan (EnvPlan).
#pragma once
#include "step_parts.h"

namespace {

// settle_lt_word two nodes per instruction: U biased (^ 0x80008000) makes each 16-bit field a
// signed value whose order is the unsigned one, so the saturating v_pk_sub_i16 of the packed biased
// thresholds has the sign of (u < C) in bits 15 and 31 of each node pair's difference.  v_perm_b32's
// sign-replicating selectors (8-11: byte 1, 3, 5, 7's bit 7 as 0x00 / 0xFF) turn two pairs (four
// nodes) into four byte masks, and v_and_or_b32 drops four-node word m at bit offset m of every
// byte: bit 8c + m of the result = node 4m + c (pk_lane_node, the inverse, is applied at the
// planes' LDS write).  32 VALU per 32 nodes where settle_lt_word spends 64.
typedef short s16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t settle_lt_word_pk(const uint32_t (&Ub)[16], const uint32_t* Cpk_) {
  ConstU32* Cpk = (ConstU32*)Cpk_;
  uint32_t d[16];
#pragma unroll
  for (int j = 0; j < 16; ++j)
    d[j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2_t, Ub[j]),
                                                                     __builtin_bit_cast(s16x2_t, Cpk[j])));
  uint32_t lt = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    // byte masks: node 4m (d[2m] bit 15), 4m+1 (d[2m] bit 31), 4m+2 (d[2m+1] bit 15), 4m+3 (d[2m+1] bit 31)
    const uint32_t e = __builtin_amdgcn_perm(d[2 * m + 1], d[2 * m], 0x0B0A0908u);
    lt = (e & (0x01010101u << m)) | lt;
  }
  return lt;
}
// settle_lt_word_pk with the packed thresholds in registers (read from the kernel's LDS copy
// ahead of the iteration's Philox calls: as scalar loads next to their use, two s_waitcnt on the
// selection wave's chain)
__device__ __forceinline__ uint32_t settle_lt_word_pk_v(const uint32_t (&Ub)[16], const uint4 (&Cv)[4]) {
  uint32_t d[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint4 c4 = Cv[j >> 2];
    const uint32_t c = (j & 3) == 0 ? c4.x : ((j & 3) == 1 ? c4.y : ((j & 3) == 2 ? c4.z : c4.w));
    d[j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2_t, Ub[j]),
                                                                     __builtin_bit_cast(s16x2_t, c)));
  }
  uint32_t lt = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const uint32_t e = __builtin_amdgcn_perm(d[2 * m + 1], d[2 * m], 0x0B0A0908u);
    lt = (e & (0x01010101u << m)) | lt;
  }
  return lt;
}
// the node whose plane lane l32 holds after transposing a settle_lt_word_pk word
__device__ __forceinline__ int pk_lane_node(int l32) { return 4 * (l32 & 7) + (l32 >> 3); }

// ------------------------------- settle-law rollout, three waves per pair of 32-env groups
// pbn_rollout under the settle law (settle_max = K >= 2, include/pbn_env.h "Step law"): the
// intervention, then synchronous updates until the env's state is in an attractor or K updates
// have run.  The roles of pbn_rollout_pipe, but one iteration is one UPDATE (t, k) of a step t,
// and every env runs its own sequence of updates: the settle law keys each update's selection per
// env (SETTLE_SEL call (k << 8 | i >> 3) of env e; DESIGN.md "Step law"), so an env that settles
// starts its next step while the other envs of its 32-env word are still updating.
//   wave 1 (env draws, lane = env): the update's draws: k = 0 the ENV call (actions, the step's
//     autoreset draws, gaps 0-2), k >= 1 the SETTLE_ENV call (gaps), one call per lane with a
//     per-lane counter; flip mask, perturbation mask (and at k = 0 the reset state, target and
//     action count) to the slot, env-major;
//   wave 2 (selection, lane = env): the env's SETTLE_SEL words of its update, compared with the
//     thresholds env-major (a subtract and a v_alignbit per node and threshold), transposed to
//     the (u < c_j) bit planes of every node;
//   wave 0 (state): the update of every env whose update is valid (s1 = s ^ m, bit-slice, node
//     chains, back-transpose, perturbed envs s1 ^ gamma), the attractor lookup, the per-env
//     decision to continue or end the step, and the step's epilogue (reward, flags, s', update
//     count, autoreset, next obs) in the iteration that ends it.
// Iteration i: the RNG waves produce each env's update R(i) into slot i & 1 while the state wave
// applies R(i-1) (EnvPlan); the state wave publishes each env's decision C (next update) in LDS.
// Results are bit-identical to pbn_step_wave's settle variants and to oracle/pbn_oracle.c.
constexpr uint32_t kNoUpd = 0xFFFFFFFFu;

// pbn_rollout_settle's output rows in LDS: every env ends its steps in its
// own iterations, so the per-env stores of the round-5 kernel were a few lanes wide and went out
// as partial-line write-backs (2.1x the outputs' bytes at 20 steps, 12.6x at 100).  The block's
// 64 envs now put step t's outputs into row t mod R of a ring in LDS, and the env-draw wave (the
// role with the most barrier slack) stores a row with full-line non-temporal stores once every
// env of the block has ended step t.  An env at most R - 1 steps ahead of the block's slowest
// waits (its update is produced and not applied), so a row is never reused before it is stored.
// Row layout (words): final [W][64] | obs [W][64] | flip mask [W][64] | reward [64] | flags
// [64 bytes] | update counts [64 u16].
// (settle_stage_rows, settle_row_words: net_layout.h, with the kernel's whole LDS carving.)
struct StageOut {   // the output pointers the row stores use, copied to LDS at kernel start
  uint32_t* final_state;
  uint32_t* obs;
  uint32_t* flipmask;
  float* reward;
  uint8_t* flags;
  uint16_t* updates;
};
static_assert(sizeof(StageOut) == kStageOutWords * 4, "StageOut is part of settle_lds_words");
constexpr uint32_t kSettleStampIt = 300;   // stamps build: the iteration the settle kernel clocks

// The per-env update plan of pbn_rollout_settle, in that env's lane of every wave (VGPRs; the
// same values in all three waves).  P = R(i-1), the update the RNG waves produced in the previous
// iteration (kNoUpd: none); C = the next update the env needs, the state wave's decision in
// iteration i-1; R = R(i), the update produced in iteration i.  R(i-1) is applied in iteration i
// iff it equals C.  A valid R(i-1) = (t, k) continues speculatively as (t, k+1), or (t+1, 0) at
// the cap; when the state wave finds the env settled the speculation is dropped and C re-issued
// (one idle iteration per step that ends before the cap).
struct EnvPlan {
  uint32_t Pt = kNoUpd, Pk = 0, Rt = 0, Rk = 0;
  bool v = false;
  __device__ __forceinline__ void next(uint32_t Ct, uint32_t Ck, uint32_t K) {
    v = Pt == Ct && Pk == Ck;
    const bool cap = Pk + 1 >= K;
    Rt = v ? (cap ? Pt + 1 : Pt) : Ct;
    Rk = v ? (cap ? 0u : Pk + 1) : Ck;
  }
  __device__ __forceinline__ void done() { Pt = Rt; Pk = Rk; }
};

template <int W, int B>
__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(4, 8)))
pbn_rollout_settle(StepArgs a) {
  extern __shared__ uint32_t smem[];   // carved below; sized by settle_lds_words (net_layout.h)
  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (role == 0) __builtin_amdgcn_s_setprio(kStatePrio);
  // the env-draw wave ahead of the selection wave (it was the iteration's pole at equal priority:
  // +5 % at the driver's shape, profiles/r05_k_ab.json)
  if (role == 1) __builtin_amdgcn_s_setprio(1);

  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int64_t g = (int64_t)blockIdx.x * 2 + half;
  const bool valid = g < a.n_groups;
  const int N = a.n_nodes;
  const int64_t n = a.n_envs;
  const int64_t le = g * 32 + l32;
  const uint64_t ge = a.env_offset + (uint64_t)le;
  const size_t plane = (size_t)W * n;
  const uint32_t n_steps = (uint32_t)a.n_steps;
  const uint32_t K = (uint32_t)a.settle_max;
  const int lq = a.lq;
  // iterations that always suffice (a step takes at most K updates and one dropped speculation):
  // a guard every wave reaches, never the exit
  const uint64_t max_it = (uint64_t)n_steps * (K + 1) + 1;
  // the first step's index: by value, or from device memory (pbn_step_dev's one-step launch)
  const uint64_t step0 = a.step_ptr ? *a.step_ptr : a.step;
  uint32_t* L = smem;
  const float* rtab = reinterpret_cast<const float*>(L + a.cdf_len);
  const uint32_t* htab = L + a.cdf_len + 4 * (N + 1);
  const uint4* selq = reinterpret_cast<const uint4*>(L + a.sel_off);
  const uint4* recL = reinterpret_cast<const uint4*>(L + a.nrec_off);
  uint32_t* Sg = smem + a.tab_words + half * 32 * W;
  // slot (per iteration parity), env-major [.][64]: flip mask [W] | perturbation mask [W] | k = 0:
  // reset state [W] | k = 0: {reset target, action count} | selection planes [lq][2][32W]
  uint32_t* slots = smem + a.tab_words + pipe_planes_words(W);
  constexpr int kFM = pipe_slot_flip(W), kGP = pipe_slot_pert(W), kRS = pipe_slot_reset(W), kIN = pipe_slot_info(W),
                kLT = pipe_slot_sel(W);
  // what follows the slots: every pointer below from SettleTail's offsets (net_layout.h)
  const SettleTail tl = {W, lq};
  uint32_t* tail = slots + 2 * (size_t)a.slot_words;
  // [parity][64]{C.t, C.k, R.t, R.k}: per env the state wave's decision C and the plan R of the
  // next iteration (EnvPlan, derived once by the state wave for all three)
  uint4* ctl = reinterpret_cast<uint4*>(tail + tl.ctl());
  if (threadIdx.x < 64) {   // C = R = (0, 0) before iteration 0; envs of groups past the end: finished
    const uint32_t c0 = valid ? 0u : n_steps;
    ctl[64 + threadIdx.x] = make_uint4(c0, 0u, c0, 0u);
  }
  // the packed thresholds (settle_pk), [lq][W][16] words after ctl: the selection wave reads them
  // by broadcast LDS reads
  uint32_t* thr_l = tail + tl.thr();
  if (a.settle_pk) {
    for (int i = (int)threadIdx.x; i < lq * W * 16; i += (int)blockDim.x) thr_l[i] = a.sthr_pk[i];
  }
  // the output rows [R][settle_row_words(W)] after the thresholds, then the lowest step not yet
  // stored, by iteration parity (written by the env-draw wave in iteration i, read by the state
  // wave in iteration i + 1)
  constexpr int R = settle_stage_rows(W), RW = settle_row_words(W);
  constexpr int kSF = settle_row_final(W), kSO = settle_row_obs(W), kSM = settle_row_flip(W), kSR = settle_row_reward(W),
                kSFL = settle_row_flags(W), kSU = settle_row_updates(W);
  uint32_t* stg = tail + tl.rows();
  uint32_t* stg_base = tail + tl.counter();
  uint64_t* stg_out = reinterpret_cast<uint64_t*>(tail + tl.out());   // the row stores' pointers (StageOut)
  if (threadIdx.x < 2) stg_base[threadIdx.x] = 0u;
  if (threadIdx.x == 0) {
    stg_out[0] = reinterpret_cast<uint64_t>(a.final_state);
    stg_out[1] = reinterpret_cast<uint64_t>(a.obs);
    stg_out[2] = reinterpret_cast<uint64_t>(a.flipmask);
    stg_out[3] = reinterpret_cast<uint64_t>(a.reward);
    stg_out[4] = reinterpret_cast<uint64_t>(a.flags);
    stg_out[5] = reinterpret_cast<uint64_t>(a.updates);
  }
  uint32_t st[W];
  uint32_t tt0 = 0, tg0 = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] = 0;
  if (role == 0 && valid) {
#pragma unroll
    for (int w = 0; w < W; ++w) st[w] = a.state[CK((size_t)w * n + le, plane, 1)];
    tt0 = a.t[CK(le, n, 2)];
    tg0 = a.target[CK(le, n, 3)];
  }
  copy_image(L, a);
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] &= valid_word_mask(N, w);
  uint32_t u_k0 = (uint32_t)a.seed, u_k1 = (uint32_t)(a.seed >> 32);
  const uint32_t u_fl = __builtin_amdgcn_readfirstlane((a.obs ? 1u : 0u) | (a.final_state ? 2u : 0u) |
                                                       ((a.mode & PBN_MODE_RANDOM_ACTIONS) ? 4u : 0u) |
                                                       ((a.mode & PBN_MODE_AUTORESET) ? 8u : 0u) |
                                                       (a.updates ? 32u : 0u));
  __syncthreads();
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the initial state loads (see pbn_rollout_pipe)
  const int mnf = __builtin_amdgcn_readfirstlane(a.max_nf);
  const uint32_t ge_lo = (uint32_t)ge;

  // one loop per role; every role derives the same plans and loop exit from the same C values
  // (the env draws' fast path: random actions, the gap bucket table, two or more single-state
  // attractors and N <= 31 for single-word states -- every kaban network -- branch-free)
  const bool env_fast = __builtin_amdgcn_readfirstlane((u_fl & 4u) && a.gap_exact == 2 && a.n_attr >= 2 &&
                                                       a.att_single && (W > 1 || N <= 31) ? 1 : 0) != 0;
  // the env-draw wave's row stores: rows [base, t_lo) once every env of the block has ended those
  // steps (t_lo = the block's lowest current step, from the decisions C), full-line non-temporal
  // stores of 64 consecutive envs; at the loop's exit every remaining row
  uint32_t base = 0;
  const int nv = (int64_t)blockIdx.x * 2 + 1 < a.n_groups ? 64 : 32;   // envs of this block (an odd group
                                                                       // count leaves a phantom half)
  auto flush_rows = [&](uint32_t ct, uint32_t it) __attribute__((always_inline)) {
    while (base < n_steps && __ballot(valid && ct <= base) == 0) {
      // the output pointers from their LDS copy, read here on this rare path (taken from the
      // kernel arguments, the compiler hoisted them out of the step loops, where they held SGPRs
      // and spilled: 2 -> 25 SGPR spills); stores through VGPR addresses
      const StageOut* ap = reinterpret_cast<const StageOut*>(stg_out);
      const uint32_t* row = stg + (size_t)(base % R) * RW;
      const size_t er = (size_t)base * (size_t)n + (size_t)blockIdx.x * 64 + (size_t)lane;   // [t][n] element
      const size_t ep = (size_t)base * plane + (size_t)blockIdx.x * 64 + (size_t)lane;      // [t][W][n] element
      if (valid) {
        if (u_fl & 2u) {
#pragma unroll
          for (int w = 0; w < W; ++w) __builtin_nontemporal_store(row[kSF + w * 64 + lane], ap->final_state + CK(ep + (size_t)w * n, (size_t)n_steps * plane, 10));
        }
        if (u_fl & 1u) {
#pragma unroll
          for (int w = 0; w < W; ++w) __builtin_nontemporal_store(row[kSO + w * 64 + lane], ap->obs + CK(ep + (size_t)w * n, (size_t)n_steps * plane, 7));
        }
        if (u_fl & 4u) {
#pragma unroll
          for (int w = 0; w < W; ++w) __builtin_nontemporal_store(row[kSM + w * 64 + lane], ap->flipmask + CK(ep + (size_t)w * n, (size_t)n_steps * plane, 8));
        }
        __builtin_nontemporal_store(__uint_as_float(row[kSR + lane]), ap->reward + CK(er, (size_t)n_steps * n, 11));
      }
      const size_t eb = (size_t)base * (size_t)n + (size_t)blockIdx.x * 64;   // the row's first env
      if (lane < nv / 4)   // the flags, four envs per dword
        __builtin_nontemporal_store(row[kSFL + lane], reinterpret_cast<uint32_t*>(ap->flags) + CK(eb / 4 + lane, (size_t)n_steps * n / 4, 15));
      if ((u_fl & 32u) && lane < nv / 2)   // the update counts, two envs per dword
        __builtin_nontemporal_store(row[kSU + lane], reinterpret_cast<uint32_t*>(ap->updates) + CK(eb / 2 + lane, (size_t)n_steps * n / 2, 23));
      ++base;
    }
    if (lane == 0) stg_base[it & 1] = base;
  };
  // (the env-draw loops below, in line: as functions of their own over a context struct each changes the
  // kernel's listing, tools/listing_diff.py)
  if (role == 1 && env_fast) {
    // ---- the draws of each env's update R(i), env `lane`: one Philox call (ENV at k = 0,
    // SETTLE_ENV at k >= 1); the step's draws are computed on every lane and kept where k = 0
    const uint2* lut = reinterpret_cast<const uint2*>(L + a.gap_lut_off);
    const uint32_t* att_words = L + a.att_off + a.n_attr + 1;
    const uint32_t A = (uint32_t)a.n_attr, n1 = (uint32_t)(N + 1);
    for (uint32_t it = 0;; ++it) {
      asm volatile("" : "+s"(u_k0), "+s"(u_k1));
      PBN_ISA_LOOP("settle_env_fast", W);
      PBN_PSTAMP(it - kSettleStampIt + 10, 0);
      uint4 C = ctl[((it + 1) & 1) * 64 + lane];   // {C(i), R(i)}
      // all four words from one read, ahead of the exit test (split, R came in a second round trip)
      asm volatile("" : "+v"(C.x), "+v"(C.y), "+v"(C.z), "+v"(C.w));
      flush_rows(C.x, it);
      if (__ballot(C.x < n_steps) == 0 || (uint64_t)it > max_it) break;
      const uint32_t t = C.z, k = C.w;
      uint32_t* slot = slots + (size_t)(it & 1) * a.slot_words;
      PBN_PSTAMP_AT(it - kSettleStampIt + 10, 16);
      const bool live = valid && t < n_steps, first = k == 0;
      const uint64_t step = step0 + (uint64_t)t;
      const uint32_t st_lo = (uint32_t)step;
      const uint32_t ge_hi = (uint32_t)((ge >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16);
      const uint32_t c2 = first ? (pbn::kStreamEnv << 28) : ((pbn::kStreamSettleEnv << 28) | ((k - 1) << 8));
      const Word4 E = pbn::philox(ge_lo, st_lo, c2, ge_hi, u_k0, u_k1);
      // the step's draws from X = ENV words 3:2 (used where k = 0): actions, the autoreset pair,
      // gap 2's uniform (what the two draws leave of X's top word, hi32(X * x_mult); att_single:
      // no third draw)
      uint32_t xhi = E.w, xlo = E.z;
      const uint32_t c_act = ext64(xhi, xlo, n1 * n1 * n1);
      const uint32_t c = ext64(xhi, xlo, A * (A - 1));   // pair_draw (A >= 2), its halves apart
      const uint32_t as = pbn::pair_start(c, a.am1_magic);
      const uint32_t u2 = first ? xhi : E.z;
      uint32_t rs[W];
#pragma unroll
      for (int w = 0; w < W; ++w) rs[w] = att_words[(size_t)as * W + w];
      const uint2 e0 = lut[min(E.x >> a.gap_shift, (uint32_t)a.gap_nb)];
      const uint2 e1 = lut[min(E.y >> a.gap_shift, (uint32_t)a.gap_nb)];
      const uint2 e2 = lut[min(u2 >> a.gap_shift, (uint32_t)a.gap_nb)];
      const uint32_t rt = pbn::pair_target(c, as, A);
      uint32_t m[W], gam[W];
#pragma unroll
      for (int w = 0; w < W; ++w) { m[w] = 0; gam[w] = 0; }
      if constexpr (W == 1) m[0] = actions_mask31(c_act, n1, a.n1_magic, valid_word_mask(N, 0));   // N <= 31
      else actions_from_draw<W>(c_act, N, a.n1_magic, m);
      uint32_t pcv = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        m[w] = live && first ? m[w] : 0u;
        pcv += __builtin_popcount(m[w]);
      }
      const int g0 = (int)e0.y + (E.x >= e0.x ? 1 : 0);   // gap_lut
      const int g1 = (int)e1.y + (E.y >= e1.x ? 1 : 0);
      const int g2 = (int)e2.y + (u2 >= e2.x ? 1 : 0);
      int p2;
      if constexpr (W == 1) p2 = pbn::first_gaps_mask31(g0, g1, g2, valid_word_mask(N, 0), gam[0]);   // N <= 31
      else p2 = pbn::first_gaps_mask<W>(g0, g1, g2, N, gam);
      if (live && p2 < N - 1) {   // rare: more gaps (k >= 1: gap 3 is the call's word 3)
        pbn::gap_tail<W>(
            k, 3, p2, N, E,
            [&](int jj) { return pbn::philox(ge_lo, st_lo, pbn::gap_call_c2(k, jj), ge_hi, u_k0, u_k1); },
            [&](uint32_t u) { return gap_lut(lut, a.gap_shift, a.gap_nb, u); }, gam);
      }
      if (live && first && t < base + R) {   // (an update past the ring is not applied: no row)
        uint32_t* row = stg + (size_t)(t % R) * RW;
#pragma unroll
        for (int w = 0; w < W; ++w) row[kSM + w * 64 + lane] = m[w];
      }
      PBN_PSTAMP_AT(it - kSettleStampIt + 10, 17);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        slot[kFM + w * 64 + lane] = m[w];
        slot[kGP + w * 64 + lane] = live ? gam[w] : 0u;
        slot[kRS + w * 64 + lane] = rs[w];
      }
      slot[kIN + lane] = rt | (pcv << 8);
      PBN_PSTAMP(it - kSettleStampIt + 10, 1);
      lds_barrier();
      PBN_PSTAMP(it - kSettleStampIt + 10, 2);
    }
  } else if (role == 1) {
    // ---- the draws of each env's update R(i), env `lane` (general networks and modes)
    for (uint32_t it = 0;; ++it) {
      asm volatile("" : "+s"(u_k0), "+s"(u_k1));
      PBN_PSTAMP(it - kSettleStampIt + 10, 0);
      uint4 C = ctl[((it + 1) & 1) * 64 + lane];   // {C(i), R(i)}
      // all four words from one read, ahead of the exit test (split, R came in a second round trip)
      asm volatile("" : "+v"(C.x), "+v"(C.y), "+v"(C.z), "+v"(C.w));
      flush_rows(C.x, it);
      if (__ballot(C.x < n_steps) == 0 || (uint64_t)it > max_it) break;
      const uint32_t t = C.z, k = C.w;
      uint32_t* slot = slots + (size_t)(it & 1) * a.slot_words;
      PBN_PSTAMP_AT(it - kSettleStampIt + 10, 16);
      uint32_t m[W], gam[W];
#pragma unroll
      for (int w = 0; w < W; ++w) { m[w] = 0; gam[w] = 0; }
      if (valid && t < n_steps) {
        const uint64_t step = step0 + (uint64_t)t;
        const uint32_t st_lo = (uint32_t)step;
        const uint32_t ge_hi = (uint32_t)((ge >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16);
        const bool first = k == 0;
        // one call per update: ENV at k = 0, SETTLE_ENV call (k-1) << 8 at k >= 1
        const uint32_t c2 = first ? (pbn::kStreamEnv << 28) : ((pbn::kStreamSettleEnv << 28) | ((k - 1) << 8));
        const Word4 E = pbn::philox(ge_lo, st_lo, c2, ge_hi, u_k0, u_k1);
        uint32_t u2 = E.z;
        if (first) {
          // the step's draws from X = ENV words 3:2: actions, the autoreset draws, gap 2's uniform
          uint32_t xhi = E.w, xlo = E.z;
          const uint32_t n1 = (uint32_t)(N + 1);
          const uint32_t c_act = ext64(xhi, xlo, n1 * n1 * n1);
          uint64_t xr = ((((uint64_t)E.w) << 32) | E.z) * a.x_mult;
          uint32_t rs[W], rtv;
          if (a.n_attr >= 1) {
            const int32_t* att_first = reinterpret_cast<const int32_t*>(L + a.att_off);
            const uint32_t* att_words = L + a.att_off + a.n_attr + 1;
            uint32_t as;
            pbn::pair_draw(xhi, xlo, (uint32_t)a.n_attr, a.am1_magic, as, rtv);
            const uint32_t row = pbn::start_pick(xhi, xlo, as, a.att_single != 0,
                                                 [&](uint32_t i) { return att_first[i]; }, xr);
#pragma unroll
            for (int w = 0; w < W; ++w) rs[w] = att_words[(size_t)row * W + w];
          } else {
            rtv = pbn::random_reset_state<W>(ge_lo, st_lo, ge_hi, u_k0, u_k1, N, rs);
          }
          u2 = (uint32_t)(xr >> 32);
          if (u_fl & 4u) {
            actions_from_draw<W>(c_act, N, a.n1_magic, m);
            if (t < base + R) {   // (an update past the ring is not applied: no row)
              uint32_t* row = stg + (size_t)(t % R) * RW;
#pragma unroll
              for (int w = 0; w < W; ++w) row[kSM + w * 64 + lane] = m[w];
            }
          } else {
#pragma unroll
            for (int w = 0; w < W; ++w)
              m[w] = a.flipmask[CK(((size_t)t * plane + (size_t)w * n) + (size_t)le, (size_t)n_steps * plane, 6)] & valid_word_mask(N, w);
          }
          uint32_t pcv = 0;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            pcv += __builtin_popcount(m[w]);
            slot[kRS + w * 64 + lane] = rs[w];
          }
          slot[kIN + lane] = rtv | (pcv << 8);
        }
        // gaps 0, 1 = words 0, 1; gap 2 = u2 (k = 0) or word 2 (k >= 1); then, rarely, more
        int g0, g1, g2;
        first_gaps(a.gap_exact, L, a, E.x, E.y, u2, g0, g1, g2);
        const int p2 = pbn::first_gaps_mask<W>(g0, g1, g2, N, gam);
        if (p2 < N - 1)   // rare: more gaps (k >= 1: gap 3 is the call's word 3)
          pbn::gap_tail<W>(
              k, 3, p2, N, E,
              [&](int jj) { return pbn::philox(ge_lo, st_lo, pbn::gap_call_c2(k, jj), ge_hi, u_k0, u_k1); },
              [&](uint32_t u) { return gap_any(a.gap_exact, L, a, u); }, gam);
      }
      PBN_PSTAMP_AT(it - kSettleStampIt + 10, 17);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        slot[kFM + w * 64 + lane] = m[w];
        slot[kGP + w * 64 + lane] = gam[w];
      }
      PBN_PSTAMP(it - kSettleStampIt + 10, 1);
      lds_barrier();
      PBN_PSTAMP(it - kSettleStampIt + 10, 2);
    }
  } else if (role == 2) {
    // ---- selection planes of each env's update R(i), env `lane`; one loop per threshold count
    // NQ (= mnf - 1) and compare form PK, so that neither is a branch inside the loop (NQ = 0: every
    // node has one function, no draws are needed)
    const int pk_node = pk_lane_node(l32);
    // (the key by value: captured by reference it left the env role's laundered copy in VGPRs; a
    // lambda: as a function template over a context struct the kernel's register allocation changes)
    auto sel_loop = [&, s_k0 = u_k0, s_k1 = u_k1](auto nq_c, auto pk_c) __attribute__((always_inline)) {
    constexpr int NQ = decltype(nq_c)::value;
    constexpr bool PK = decltype(pk_c)::value;
    for (uint32_t it = 0;; ++it) {
      PBN_ISA_LOOP("settle_sel", 2 * NQ + (PK ? 1 : 0));
      PBN_PSTAMP(it - kSettleStampIt + 10, 0);
      uint4 C = ctl[((it + 1) & 1) * 64 + lane];   // {C(i), R(i)}
      // all four words from one read, ahead of the exit test (split, R came in a second round trip)
      asm volatile("" : "+v"(C.x), "+v"(C.y), "+v"(C.z), "+v"(C.w));
      if (__ballot(C.x < n_steps) == 0 || (uint64_t)it > max_it) break;
      const uint32_t t = C.z, k = C.w;   // (no update: the words are computed and discarded)
      // PK: this iteration's packed thresholds, requested now (used after the Philox calls)
      uint4 thv[W][NQ > 0 ? NQ : 1][4];
      if constexpr (PK) {
#pragma unroll
        for (int r = 0; r < W; ++r)
#pragma unroll
          for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              thv[r][q][c] = reinterpret_cast<const uint4*>(thr_l + (size_t)(q * W + r) * 16)[c];
            }
      }
      uint32_t* lt_out = slots + (size_t)(it & 1) * a.slot_words + kLT + half * 32 * W;
      const uint64_t step = step0 + (uint64_t)t;
      const uint32_t st_lo = (uint32_t)step;
      const uint32_t ge_hi = (uint32_t)((ge >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16);
      const uint32_t* th = a.sthr;
      asm volatile("" : "+s"(th));   // the thresholds are read per iteration (hoisted: SGPR spills)
#pragma unroll
      for (int r = 0; r < W; ++r) {
        if constexpr (NQ > 0) {
          uint32_t U[16];
          // PK: the compares' bias (^ 0x80008000) folded into words 0 and 2 of every call
          settle_sel_words<PK ? 0x80008000u : 0u>(ge_lo, ge_hi, st_lo, k, r, N, s_k0, s_k1, U);
          PBN_PSTAMP_AT(it - kSettleStampIt + 10, 18);
          if constexpr (PK) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
              if (j & 1) U[j] ^= 0x80008000u;   // words 1 and 3 (the low products) are not
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              const uint32_t lt = settle_lt_word_pk_v(U, thv[r][q]);
              lt_out[q * 64 * W + 32 * r + pk_node] = lane_transpose32(lt, lane);
            }
          } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              const uint32_t lt = settle_lt_word(U, th + (size_t)(q * W + r) * 32);
              lt_out[q * 64 * W + 32 * r + l32] = lane_transpose32(lt, lane);
            }
          }
        }
      }
      PBN_PSTAMP(it - kSettleStampIt + 10, 1);
      lds_barrier();
      PBN_PSTAMP(it - kSettleStampIt + 10, 2);
    }
    };
    const bool pk = __builtin_amdgcn_readfirstlane(a.settle_pk) != 0;
    using T_ = std::true_type;
    using F_ = std::false_type;
    switch (min(mnf - 1, kNodeRecs - 1)) {   // (lq >= 1 in the slot layout; one function per node needs no draws)
      case 0: sel_loop(std::integral_constant<int, 0>{}, F_{}); break;
      case 1: pk ? sel_loop(std::integral_constant<int, 1>{}, T_{}) : sel_loop(std::integral_constant<int, 1>{}, F_{}); break;
      case 2: pk ? sel_loop(std::integral_constant<int, 2>{}, T_{}) : sel_loop(std::integral_constant<int, 2>{}, F_{}); break;
      default: pk ? sel_loop(std::integral_constant<int, 3>{}, T_{}) : sel_loop(std::integral_constant<int, 3>{}, F_{}); break;
    }
  } else {
    // ---- state of env `lane` (env-major), bit-sliced per update for the node chains
    uint32_t rs[W];           // the autoreset state drawn at the current step's first update
    uint32_t rtv = 0, pcv = 0;
    uint32_t Ct = valid ? 0u : n_steps, Ck = 0;
    bool pacc = false;
#pragma unroll
    for (int w = 0; w < W; ++w) rs[w] = 0;
    // one loop per function count KF (mnf, at most kNodeRecs): no switch inside the loop (a lambda: as a
    // function template over a context struct it changes the kernel's listing, tools/listing_diff.py)
    auto state_loop = [&](auto kf_c) __attribute__((always_inline)) {
    constexpr int KF = decltype(kf_c)::value;
    // single-word states: the node records' input indices held in VGPRs, and each update's
    // selection planes and selectors read before the transpose (as pbn_rollout_pipe's state_fast),
    // so that their LDS latency is off the chain slot -> transpose -> gathers -> back-transpose
    uint32_t ins[KF];
#pragma unroll
    for (int q = 0; q < KF; ++q) ins[q] = W == 1 ? recL[q * 32 + l32].x : 0u;
    EnvPlan p;
    p.next(Ct, Ck, K);   // iteration 0's plan (then each iteration's, at the end of the one before)
    for (uint32_t it = 0;; ++it) {
      PBN_ISA_LOOP("settle_state", KF);
      PBN_PSTAMP(it - kSettleStampIt + 10, 0);
      if (__ballot(Ct < n_steps) == 0 || (uint64_t)it > max_it) break;
      // the lowest step whose row is not stored yet, as the env-draw wave left it in the iteration
      // that produced this update: an update R - 1 or more steps past it waits (no row to write)
      const uint32_t sbase = stg_base[(it + 1) & 1];
      const bool proc = p.v && p.Pt < n_steps && p.Pt < sbase + R;
      const uint32_t t = p.Pt, k = p.Pk;
      uint32_t* row = stg + (size_t)(t % R) * RW;
      const uint32_t* slot = slots + (size_t)((it + 1) & 1) * a.slot_words;
      const uint32_t* lt_in = slot + kLT + half * 32 * W;
      uint32_t s1[W], gam[W];
      bool pk = false;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        s1[w] = st[w] ^ slot[kFM + w * 64 + lane];   // (the flip mask is 0 past an update's first)
        gam[w] = slot[kGP + w * 64 + lane];
        pk = pk || gam[w] != 0;
      }
      if (proc && k == 0) {   // the step's reset draw and action count; the step's observation
#pragma unroll
        for (int w = 0; w < W; ++w) row[kSO + w * 64 + lane] = st[w];
#pragma unroll
        for (int w = 0; w < W; ++w) rs[w] = slot[kRS + w * 64 + lane];
        const uint32_t info = slot[kIN + lane];
        rtv = info & 0xFFu;
        pcv = (info >> 8) & 0xFFu;
        pacc = false;
      }
      uint32_t X[W];
      if constexpr (W == 1) {
        uint32_t ltv[KF];
        uint4 sa[KF], sb[KF];
#pragma unroll
        for (int q = 0; q < KF; ++q) {
          ltv[q] = q < KF - 1 ? lt_in[q * 64 + l32] : 0u;
          sa[q] = selq[(2 * q) * 32 + l32];
          sb[q] = selq[(2 * q + 1) * 32 + l32];
        }
        Sg[l32] = lane_transpose32(s1[0], lane);
        PBN_PSTAMP_AT(it - kSettleStampIt + 10, 15);
        __builtin_amdgcn_wave_barrier();
        uint32_t x = 0;
#pragma unroll
        for (int q = KF - 1; q >= 0; --q) {
          uint32_t xin[4];
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) xin[kk] = plane_in<true>(Sg, ins[q], kk);
          const uint32_t fj = eval_sel_in(xin, sa[q], sb[q]);
          x = (q == KF - 1) ? fj : bfi(ltv[q], fj, x);
        }
        X[0] = x;
      } else {
#pragma unroll
        for (int w = 0; w < W; ++w) Sg[32 * w + l32] = lane_transpose32(s1[w], lane);
        PBN_PSTAMP_AT(it - kSettleStampIt + 10, 15);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < W; ++r) {
          int i = l32 + 32 * r;
          asm volatile("" : "+v"(i));   // selector and record reads stay in the loop
          const uint4* rc = recL + i;
          const uint4* sel = selq + i;
          const uint32_t* lti = lt_in + i;
          X[r] = chain_padded<KF, (W <= 2)>(rc, sel, 32 * W, Sg, lti, 64 * W);
        }
      }
      PBN_PSTAMP_AT(it - kSettleStampIt + 10, 3);
      uint32_t cur[W];
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const uint32_t x = lane_transpose32(X[w], lane);
        cur[w] = proc ? (pk ? s1[w] ^ gam[w] : x) : st[w];
      }
      PBN_PSTAMP_AT(it - kSettleStampIt + 10, 12);
      const int att = attractor_lookup<W>(a, htab, cur);
      const bool open = att < 0;
      const bool end = proc && (!open || k + 1 >= K);
      if (proc) {
        pacc = pacc || pk;
        Ct = end ? t + 1 : t;
        Ck = end ? 0u : k + 1;
      }
      // the next iteration's plan, published with the decision (the RNG waves read it)
      p.done();
      p.next(Ct, Ck, K);
      ctl[(it & 1) * 64 + lane] = make_uint4(Ct, Ck, p.Rt, p.Rk);
#pragma unroll
      for (int w = 0; w < W; ++w) st[w] = cur[w];
      if (end) {
        // the epilogue of step t, into the block's row of step t (stored by the env-draw wave)
#pragma unroll
        for (int w = 0; w < W; ++w) row[kSF + w * 64 + lane] = cur[w];
        reinterpret_cast<uint16_t*>(row + kSU)[lane] = (uint16_t)min(k + 1, 0xFFFFu);
        // (pbn::step_outcome restated: through the helper this loop's epilogue changes its listing)
        const bool in_attr = att >= 0;
        const bool term = in_attr && (uint32_t)att == tg0;
        const bool wrong = in_attr && !term;
        int tt = (int)tt0 + 1;
        tt = tt > 255 ? 255 : tt;
        const bool trunc = a.horizon > 0 && tt >= a.horizon;
        const bool rst = (u_fl & 8u) && (term || trunc);
        const uint32_t fl = (uint32_t)term | ((uint32_t)trunc << 1) | ((uint32_t)in_attr << 2) |
                            ((uint32_t)pacc << 3) | ((uint32_t)rst << 4) | ((uint32_t)open << 5);
        // the reward row as one 16-byte read (split by the compiler into reads under the term /
        // wrong branches, it cost two round trips in the epilogue)
        float4 r4 = reinterpret_cast<const float4*>(rtab)[pcv];
        asm volatile("" : "+v"(r4.x), "+v"(r4.y), "+v"(r4.z));
        row[kSR + lane] = __float_as_uint(term ? r4.z : (wrong ? r4.y : r4.x));
        reinterpret_cast<uint8_t*>(row + kSFL)[lane] = (uint8_t)fl;
        tg0 = rst ? rtv : tg0;
        tt0 = rst ? 0u : (uint32_t)tt;
#pragma unroll
        for (int w = 0; w < W; ++w) st[w] = rst ? rs[w] : cur[w];
      }
      PBN_PSTAMP(it - kSettleStampIt + 10, 1);
      lds_barrier();
      PBN_PSTAMP(it - kSettleStampIt + 10, 2);
    }
    };
    switch (mnf) {
      case 1: state_loop(std::integral_constant<int, 1>{}); break;
      case 2: state_loop(std::integral_constant<int, 2>{}); break;
      case 3: state_loop(std::integral_constant<int, 3>{}); break;
      default: state_loop(std::integral_constant<int, 4>{}); break;
    }
    if (valid) {
#pragma unroll
      for (int w = 0; w < W; ++w) a.state_out[CK((size_t)w * n + le, plane, 16)] = st[w];
      a.t[CK(le, n, 17)] = (uint8_t)tt0;
      a.target[CK(le, n, 18)] = (uint8_t)tg0;
    }
  }
}

}  // namespace
