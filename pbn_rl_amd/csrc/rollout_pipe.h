// rollout_pipe.h -- pbn_rollout_pipe, the pipelined one-update rollout (three waves per pair of
// 32-env groups), and what it alone uses: the ride-along copy of pbn_rollout_copy, the digit-mask
// compares, the running step of the fast RNG loops and the node chain of nodes with more than
// kNodeRecs functions.
#pragma once
#include "step_parts.h"

namespace {

// the ride-along copy of pbn_rollout_copy: a fourth wave per block (launched only when there is a
// copy) moves the block's contiguous share of the vectors and exits; s_barrier waits for the
// surviving waves only, so the three step roles run as without it.
//   burst (cp_u = 0): the share at once, kDepth 1-KB loads per lane in flight;
//   paced (cp_u = U): the share in n_steps + 1 portions of U vectors per lane, portion k stored
//   at iteration k's block barrier and requested A = 4 / U iterations ahead, so the copy's HBM
//   traffic spreads over the launch instead of competing with its first iterations (the burst:
//   0.65x of the bare launches' rate at 2,000 steps, paced 0.89x; r05_y, r05_za).
// (The copy folded into the env-draw waves' step loop held every iteration to the loads'
// latency: +48 us on a 100-step launch of 65,536 envs, r05_u, profiles/r05_u_ride_env_wave.patch.)
__device__ __forceinline__ void ride_copy_burst(const StepArgs& a, int lane) {
  constexpr int kDepth = 8;
  const int64_t per = ((a.cp_n16 + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x + 63) & ~(int64_t)63;
  const int64_t i0 = (int64_t)blockIdx.x * per;
  const int64_t i1 = min(i0 + per, a.cp_n16);
  const pbn_u32x4* src = static_cast<const pbn_u32x4*>(a.cp_src);
  pbn_u32x4* dst = static_cast<pbn_u32x4*>(a.cp_dst);
  for (int64_t base = i0 + lane; base < i1; base += kDepth * 64) {
    pbn_u32x4 v[kDepth];
#pragma unroll
    for (int u = 0; u < kDepth; ++u)
      if (base + u * 64 < i1) v[u] = __builtin_nontemporal_load(src + base + u * 64);
#pragma unroll
    for (int u = 0; u < kDepth; ++u)
      if (base + u * 64 < i1) __builtin_nontemporal_store(v[u], dst + base + u * 64);
  }
}

// vectors per lane in flight in the paced copy: 4 measured 0.89x of the bare launches at 2,000
// steps, 2 0.69x, 8 0.81x, 16 (spills) 0.44x (profiles/r05_za_ab.json, r05_z)
constexpr int kRideVecs = 4;
template <int U>
__device__ __forceinline__ void ride_copy_paced(const StepArgs& a, int lane) {
  constexpr int A = kRideVecs / U > 0 ? kRideVecs / U : 1;   // portions in flight
  const int iters = a.n_steps + 1;
  const int64_t per = (int64_t)iters * U * 64;   // the host sized U so that the grid covers cp_n16
  const int64_t i0 = (int64_t)blockIdx.x * per + lane;
  const int64_t i1 = a.cp_n16;
  const pbn_u32x4* src = static_cast<const pbn_u32x4*>(a.cp_src);
  pbn_u32x4* dst = static_cast<pbn_u32x4*>(a.cp_dst);
  pbn_u32x4 v[A][U];
  auto load = [&](int k, pbn_u32x4 (&r)[U]) {
    if (k >= iters) return;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + ((int64_t)k * U + u) * 64;
      if (i < i1) r[u] = __builtin_nontemporal_load(src + i);   // (plain loads: equal, r05_z)
    }
  };
  auto store = [&](int k, const pbn_u32x4 (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + ((int64_t)k * U + u) * 64;
      if (i < i1) __builtin_nontemporal_store(r[u], dst + i);
    }
  };
#pragma unroll
  for (int j = 0; j < A; ++j) load(j, v[j]);
  for (int k0 = 0; k0 < iters; k0 += A) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const int k = k0 + j;
      if (k >= iters) return;
      store(k, v[j]);
      load(k + A, v[j]);
      __builtin_amdgcn_s_barrier();   // the block's barrier of iteration k (no LDS to fence)
    }
  }
}

__device__ __forceinline__ void ride_copy_wave(const StepArgs& a, int lane) {
  switch (a.cp_u) {
    case 1: ride_copy_paced<1>(a, lane); break;
    case 2: ride_copy_paced<2>(a, lane); break;
    case 4: ride_copy_paced<4>(a, lane); break;
    default: ride_copy_burst(a, lane); break;
  }
}

// less_than with the threshold's digit masks read from LDS: cmq[d * stride] = ~0 if bit
// (B-1-d) of the threshold is set, else 0 (built once per block; saves a v_bfe per digit)
// (the masks' layout: sel_mask_stride, net_layout.h)
template <int B>
__device__ __forceinline__ uint32_t less_than_cm4(const uint32_t (&dig)[16], const uint32_t* __restrict__ cmq) {
  const uint4* c4 = reinterpret_cast<const uint4*>(cmq);
  uint4 m[B / 4];
#pragma unroll
  for (int j = 0; j < B / 4; ++j) m[j] = c4[j];
  uint32_t lt = 0;
#pragma unroll
  for (int d = B - 1; d >= 0; --d) {
    const uint4 v = m[d >> 2];
    const uint32_t c = (d & 3) == 0 ? v.x : ((d & 3) == 1 ? v.y : ((d & 3) == 2 ? v.z : v.w));
    lt = __builtin_amdgcn_bitop3_b32(dig[d], lt, c, 0x8E);
  }
  return lt;
}

template <int B>
__device__ __forceinline__ uint32_t less_than_cm(const uint32_t (&dig)[16], const uint32_t* __restrict__ cmq,
                                                 int stride) {
  uint32_t lt = 0;
#pragma unroll
  for (int d = 15; d >= 0; --d) {
    if (d < B) lt = __builtin_amdgcn_bitop3_b32(dig[d], lt, cmq[d * stride], 0x8E);
  }
  return lt;
}

// The running step of an RNG wave's fast loop: its low word (wave-uniform: an SGPR), advanced by
// one.  The fast loops run only where every step of the launch has the same high word
// (step_hi_fixed), so the word does not wrap and no carry leaves.  Written as the instruction: the
// compiler would rebuild the sum from a.step and the loop counter every step.
__device__ __forceinline__ void step_advance(uint32_t& lo) {
  asm("s_add_u32 %0, %0, 1" : "+s"(lo) : : "scc");
}

// Do the steps first .. first + n_steps (the RNG waves compute one step ahead) share the high word
// of the 64-bit step?  Then counter word 3 and with it the Philox prefix (philox.h) of every
// per-step call are launch invariants.  A launch that crosses a multiple of 2^32 takes the general
// role loops.
__device__ __forceinline__ bool step_hi_fixed(uint64_t first, int n_steps) {
  return (uint32_t)(first >> 32) == (uint32_t)((first + (uint64_t)n_steps) >> 32);
}

// ------------------------------- rollout kernel, three waves per pair of 32-env groups
// Block = two groups (64 envs; lanes 32h..32h+31 of every wave work on group 2*block + h).
// The step splits into work that depends only on the counter-based RNG and work that
// depends on the state, so different waves run different steps:
//   wave 1 (env draws): ENV + PERT call 0 of env `lane` -> actions / given flip mask,
//     perturbation mask, autoreset draw;
//   wave 2 (selection): SEL calls of node `lane & 31` -> the (u < c_j) masks of its thresholds;
//   wave 0 (state): s1 = s ^ m, bit-slice, node evaluation from the masks, back-transpose,
//     attractor lookup, reward, flags, autoreset, stores.
// Iteration k: waves 1 and 2 produce step k into slot k&1 while wave 0 consumes step k-1
// from the other slot; the block barrier ends the iteration.  Same results as pbn_step_wave.
// Each wave alone is latency-bound, so the split (three instruction streams per group pair)
// is what fills the SIMDs at small batches.

// node chain from precomputed selection masks: x = F_{nf-1}; x = lt_j ? F_j : x, with every
// LDS read of the K records issued before any use (K = wave-uniform bound, nf per lane)
template <int K, bool BY>
__device__ __forceinline__ uint32_t chain_from_masks(const uint4 (&rec)[kNodeRecs], const uint4* __restrict__ sel,
                                                     int stride, const uint32_t* __restrict__ S,
                                                     const uint32_t* __restrict__ lt, int lt_stride, int nf,
                                                     bool tail, uint32_t x) {
  uint32_t xin[K][4], ltv[K];
  uint4 sa[K], sb[K];
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const uint32_t ins = rec[q].x;
#pragma unroll
    for (int k = 0; k < 4; ++k) xin[q][k] = plane_in<BY>(S, ins, k);
    sa[q] = sel[(2 * q) * stride];
    sb[q] = sel[(2 * q + 1) * stride];
    // mask q exists for q < K - 1, and for q = K - 1 too when some node has more than K
    // (= kNodeRecs) functions
    ltv[q] = (q < K - 1 || tail) ? lt[q * lt_stride] : 0u;
  }
#pragma unroll
  for (int q = K - 1; q >= 0; --q) {
    const uint32_t x0 = xin[q][0], x1 = xin[q][1], x2 = xin[q][2], x3 = xin[q][3];
    const uint32_t nx0 = ~x0;
    const uint32_t v0 = __builtin_amdgcn_perm(nx0, x0, sa[q].x), v1 = __builtin_amdgcn_perm(nx0, x0, sa[q].y);
    const uint32_t v2 = __builtin_amdgcn_perm(nx0, x0, sa[q].z), v3 = __builtin_amdgcn_perm(nx0, x0, sa[q].w);
    const uint32_t v4 = __builtin_amdgcn_perm(nx0, x0, sb[q].x), v5 = __builtin_amdgcn_perm(nx0, x0, sb[q].y);
    const uint32_t v6 = __builtin_amdgcn_perm(nx0, x0, sb[q].z), v7 = __builtin_amdgcn_perm(nx0, x0, sb[q].w);
    const uint32_t w0 = bfi(x1, v1, v0), w1 = bfi(x1, v3, v2), w2 = bfi(x1, v5, v4), w3 = bfi(x1, v7, v6);
    const uint32_t fj = bfi(x3, bfi(x2, w3, w2), bfi(x2, w1, w0));
    const uint32_t y = (q == nf - 1) ? fj : bfi(ltv[q], fj, x);
    x = (q < nf) ? y : x;
  }
  return x;
}

// MANY: some node has more than kNodeRecs functions.  Those chains read records past the LDS
// copy (global fcompact) and hold every record of a node in registers; compiled out of the
// common instances (every bundled network has at most 3 functions per node), they no longer set
// the register allocation of the whole kernel: 167 -> 88 VGPRs at three state words (pbn70),
// 121 -> 83 at two, 242 -> 93 at four.
// Waves per SIMD the register allocation must allow for single-word states: 6 (<= 80 VGPRs,
// no spill in the step loops) runs 1M envs 10 % faster than the unconstrained 86 VGPRs (5 waves);
// 7 and 8 spill to scratch in the state loop and lose (profiles/r02_ab_waves_per_eu.jsonl).
// Multi-word states: 5 waves without MANY; with MANY, three words are held to 3 waves (167 VGPRs,
// where the compiler's choice is 181: 2 waves) and two words fit 4 waves as they are.
#define PBN_PIPE_ATTR __attribute__((amdgpu_waves_per_eu(W == 1 ? 6 : (MANY ? (W == 3 ? 3 : 1) : 5), 8)))
template <int W, int B, bool MANY>
__global__ void __launch_bounds__(256) PBN_PIPE_ATTR pbn_rollout_pipe(StepArgs a) {
  constexpr int CPN = B / 4;              // selection calls per node
  extern __shared__ uint32_t smem[];   // carved below; sized by pipe_lds_words (net_layout.h)
  const int lane = threadIdx.x & 63;
  const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar branches
  // the state wave bounds every iteration: let it win VALU issue against the RNG waves of
  // other blocks sharing its SIMD
  PBN_RSTAMP(0);
  if (role == 0) __builtin_amdgcn_s_setprio(kStatePrio);
  // with one block per SIMD triple (every SIMD holds one wave of each role) the selection wave,
  // the longest instruction stream, also goes ahead of the env-draw wave: -5 % per step at
  // 65,536 envs; with more blocks resident it loses 4-8 % (profiles/r02_ab_wave_priority.jsonl)
  if (role == 2 && a.sel_prio) __builtin_amdgcn_s_setprio(1);
#ifdef PBN_STAMPS
  // placement of this wave: HW_ID (wave, SIMD, CU, SH, SE) in the low word, XCC_ID above it
  if (a.stamps && lane == 0)
    a.stamps[(size_t)blockIdx.x * 32 + (role == 0 ? 14 : role * 4 + 3)] =
        (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
        ((unsigned long long)__builtin_amdgcn_s_getreg((15 << 11) | 20) << 32);
#endif
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int64_t g = (int64_t)blockIdx.x * 2 + half;
  const bool valid = g < a.n_groups;
  const int N = a.n_nodes;
  const int64_t n = a.n_envs;
  const int64_t le = g * 32 + l32;
  const uint64_t ge = a.env_offset + (uint64_t)le;
  const uint64_t G = ge >> 5;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const bool random_actions = (a.mode & PBN_MODE_RANDOM_ACTIONS) != 0;
  const size_t plane = (size_t)W * n;
  const int n_steps = a.n_steps;
  const int LQ = a.lq;
  // LDS: table image | S planes [2][32W] | two slots (net_layout.h: the carving, a slot's fields)
  uint32_t* L = smem;
  const float* rtab = reinterpret_cast<const float*>(L + a.cdf_len);
  const uint32_t* htab = L + a.cdf_len + 4 * (N + 1);
  const uint4* selq = reinterpret_cast<const uint4*>(L + a.sel_off);
  uint32_t* Sg = smem + a.tab_words + half * 32 * W;   // this half's group
  uint32_t* slots = smem + a.tab_words + pipe_planes_words(W);
  constexpr int kFM = pipe_slot_flip(W), kGP = pipe_slot_pert(W), kRS = pipe_slot_reset(W), kIN = pipe_slot_info(W),
                kLT = pipe_slot_sel(W);
  uint32_t st[W];
  uint32_t tt0 = 0, tg0 = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] = 0;
  if (role == 0 && valid) {   // issued first: their latency overlaps the image copy
#pragma unroll
    for (int w = 0; w < W; ++w) st[w] = a.state[CK((size_t)w * n + le, plane, 1)];
    tt0 = a.t[CK(le, n, 2)];
    tg0 = a.target[CK(le, n, 3)];
  }
  copy_image(L, a);
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] &= valid_word_mask(N, w);
  // node records live in LDS (L + nrec_off), record-major [kNodeRecs][32W] so that a wave's
  // lanes (nodes) read consecutive 16-byte records without bank conflicts: each role reads
  // what it needs per step, so no record is carried in VGPRs across the step loop
  const uint4* recL = reinterpret_cast<const uint4*>(L + a.nrec_off);
  // wave-uniform parameters, re-defined (laundered) every iteration: hoisted out of the step
  // loop, the conditions built from them occupy SGPR pairs and spill to VGPR lanes
  uint32_t u_k0 = k0, u_k1 = k1;
  int u_gx = a.gap_exact, u_na = a.n_attr,  u_mnf = a.max_nf, u_hb = a.hash_bits,
      u_hp = a.hash_probes, u_hz = a.horizon;
  uint32_t u_fl = __builtin_amdgcn_readfirstlane((a.obs ? 1u : 0u) | (a.final_state ? 2u : 0u) |
                                                 (random_actions ? 4u : 0u) | ((a.mode & PBN_MODE_AUTORESET) ? 8u : 0u) |
                                                 (a.att_single ? 16u : 0u));
  // digit masks of the first kNodeRecs - 1 thresholds of every node, lane-major
  // [32][sel_mask_stride(B)], for the selection wave's compares: built on the host into the table
  // image (single-word states only: for W > 1 the extra LDS cost more occupancy than it saved,
  // measured -15 % on pbn70 x 1M).  Built here from the records, they took a second barrier.
  const uint32_t* cm = L + a.cm_off;
  __syncthreads();
  PBN_RSTAMP(1);
  if (role == 3) {   // (pbn_rollout_copy) past the block's last __syncthreads
    ride_copy_wave(a, lane);
    return;
  }
  // drain the initial state loads here: otherwise the loop-carried st / t / target copies at
  // the bottom of the loop wait on vmcnt(0), which also waits for every store of the step
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) expcnt(7) lgkmcnt(15)
  PBN_RSTAMP(2);

  // one loop per role: every wave passes the same n_steps + 1 block barriers, and each role's
  // loop-carried values (hoisted invariants) occupy registers only in that role's loop
  const bool u_hi_fixed = step_hi_fixed(a.step, n_steps);   // wave-uniform: the fast RNG loops' Philox prefix holds
  // (in line: as a function of its own over a context struct this role changes the kernel's listing, tools/listing_diff.py)
  if (role == 1 && (u_fl & 4u) && u_gx == 2 && u_na >= 2 && (u_fl & 16u) && (W > 1 || N <= 31) && u_hi_fixed) {
    // env draws, common configuration (random actions, gap bucket table, two or more
    // single-state attractors): the same draws as the general loop below, branch-free apart from
    // the rare fourth-flip tail, so that the next step's ENV call
    // (computed here, one step ahead) interleaves with this step's dependent draws and LDS reads
    // instead of following them
    const uint32_t A = (uint32_t)u_na;
    const uint32_t n1 = (uint32_t)(N + 1);
    const uint32_t* att_words = L + a.att_off + u_na + 1;
    const uint2* lut = reinterpret_cast<const uint2*>(L + a.gap_lut_off);
    // the Philox key schedule, built once per wave (pinned: opaque SGPR values that are not
    // rematerialised as adds of literals in the loop), and the low word of the running step of the
    // ENV call being computed, one ahead of the step being drawn.  Counter word 3 (the env id's
    // and the step's high halves; the shift drops bits 48 and up) is the same for every step of
    // the launch (step_hi_fixed), so the part of the ENV call's first three rounds that does not
    // depend on the step's low word is built once per lane (philox_prefix; pinned: opaque VGPR
    // values whose products are not rematerialised in the loop)
    uint32_t rk0[pbn::kPhiloxRounds], rk1[pbn::kPhiloxRounds];
    pbn::philox_round_keys(k0, k1, rk0, rk1);
#pragma unroll
    for (int r = 0; r < pbn::kPhiloxRounds; ++r) asm volatile("" : "+s"(rk0[r]), "+s"(rk1[r]));
    const uint32_t ge_hi = (uint32_t)((ge >> 32) & 0xFFFFu) | ((uint32_t)(a.step >> 32) << 16);
    uint32_t step_lo = (uint32_t)a.step;
    pbn::PhiloxPrefix pre = pbn::philox_prefix((uint32_t)ge, pbn::kStreamEnv << 28, ge_hi, rk0, rk1);
    asm volatile("" : "+v"(pre.A), "+v"(pre.B), "+v"(pre.D), "+v"(pre.E), "+v"(pre.d3));
    // PERT call 0 of the lane (the rare fourth-flip tail) differs from its ENV call in counter word 2
    // alone: the same B and D, and three more pinned values
    pbn::PhiloxPrefix pre_pert = pbn::philox_prefix_sibling(pre, (uint32_t)ge, pbn::kStreamPert << 28, ge_hi, rk0, rk1);
    asm volatile("" : "+v"(pre_pert.A), "+v"(pre_pert.E), "+v"(pre_pert.d3));
    auto env_call = [&]() { return pbn::philox_tail(pre, step_lo, rk0, rk1); };
    StepRows<uint32_t> fm_rows = rows_open(a.flipmask, n, (size_t)n_steps * plane);
    // one step (k < n_steps; `odd` = k & 1, known at compile time: the slot costs no select):
    // this step's draws from E, the next step's ENV call into E_next
    auto env_step = [&](int k, auto odd, const Word4& E, Word4& E_next) {
      asm volatile("" : "+s"(u_gx), "+s"(u_na), "+s"(u_mnf));
      asm volatile("" : "+s"(u_hb), "+s"(u_hp), "+s"(u_hz), "+s"(u_fl));
      PBN_ISA_LOOP("env_fast", W);
      PBN_PSTAMP(k, 0);
      {
        uint32_t* slot = slots + (decltype(odd)::value ? (size_t)a.slot_words : (size_t)0);
        // part 1: the draws that feed LDS reads, and the reads themselves
        uint32_t xhi = E.w, xlo = E.z;
        const uint32_t c_act = ext64(xhi, xlo, n1 * n1 * n1);
        const uint32_t c = ext64(xhi, xlo, A * (A - 1));   // pair_draw (A >= 2), its halves apart
        const uint32_t as = pbn::pair_start(c, a.am1_magic);
        // gap 2's uniform: what the two draws leave of X's top word (att_single: no third draw),
        // hi32(X * x_mult) without a product of its own
        const uint32_t u2 = xhi;
        uint32_t rs[W];
#pragma unroll
        for (int w = 0; w < W; ++w) rs[w] = att_words[(size_t)as * W + w];   // (att_single: start_pick is `as`)
        const uint2 e0 = lut[min(E.x >> a.gap_shift, (uint32_t)a.gap_nb)];
        const uint2 e1 = lut[min(E.y >> a.gap_shift, (uint32_t)a.gap_nb)];
        const uint2 e2 = lut[min(u2 >> a.gap_shift, (uint32_t)a.gap_nb)];
        // part 2: the next step's ENV call runs while those reads are in flight (the scheduling
        // barriers keep the compiler from hoisting it above them or sinking it to the latch)
        asm volatile("" ::: "memory");   // the LDS reads above are issued here
        __builtin_amdgcn_sched_barrier(0);
        PBN_PSTAMP_AT(k, 16);
        step_advance(step_lo);
        E_next = env_call();   // (one unused call per launch)
        asm volatile("" : "+v"(E_next.x), "+v"(E_next.y), "+v"(E_next.z), "+v"(E_next.w));
        __builtin_amdgcn_sched_barrier(0);
        PBN_PSTAMP_AT(k, 17);
        // part 3: the rest of step k's draws
        const uint32_t rt = pbn::pair_target(c, as, A);
        uint32_t m[W], gam[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { m[w] = 0; gam[w] = 0; }
        if constexpr (W == 1) m[0] = actions_mask31(c_act, n1, a.n1_magic, valid_word_mask(N, 0));   // N <= 31
        else actions_from_draw<W>(c_act, N, a.n1_magic, m);
        uint32_t pc = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) pc += __builtin_popcount(m[w]);
        const int g0 = (int)e0.y + (E.x >= e0.x ? 1 : 0);   // gap_lut
        const int g1 = (int)e1.y + (E.y >= e1.x ? 1 : 0);
        const int g2 = (int)e2.y + (u2 >= e2.x ? 1 : 0);
        int p2;
        if constexpr (W == 1) p2 = pbn::first_gaps_mask31(g0, g1, g2, valid_word_mask(N, 0), gam[0]);   // N <= 31
        else p2 = pbn::first_gaps_mask<W>(g0, g1, g2, N, gam);
        bool pert = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          pert = pert || gam[w] != 0;
          slot[kFM + w * 64 + lane] = m[w];
          slot[kGP + w * 64 + lane] = gam[w];
          slot[kRS + w * 64 + lane] = rs[w];
        }
        slot[kIN + lane] = rt | (pc << 8) | ((uint32_t)pert << 16);
#pragma unroll
        for (int w = 0; w < W; ++w) rows_store(fm_rows, w, (size_t)w * n, le, valid, 8, m[w]);
        rows_advance(fm_rows, plane);
        PBN_PTAIL(k, p2 < N - 1);
        // the rare fourth-flip tail (a lane in 400 at p = 0.01, N = 28: one iteration in six of a
        // 64-lane wave): PERT call 0 from its pinned prefix, the fourth gap in line unless its word
        // falls in the table's last bucket (no flip, three times in four), the further gaps out of
        // line (gap_tail_split); then the two slot fields that hold the mask again.  (Deciding
        // first and writing each field once was 2.5 % slower: the writes then trail the branch in
        // every iteration.)  The state wave is waiting for this one by now: its ~30 dependent
        // instructions issue at that wave's priority instead of behind the other two waves'
        if (p2 < N - 1) {
          PBN_ISA_ARM("gap_tail");   // (tools/isa_budget.py walks the iteration without it)
          __builtin_amdgcn_s_setprio(kStatePrio);
          // this step's low word: the running step is one ahead (no borrow: step_hi_fixed)
          const uint32_t step_lo_k = step_lo - 1u;
          pbn::gap_tail_split<W>(
              p2, N, pbn::philox_tail(pre_pert, step_lo_k, rk0, rk1),
              [&](int jj) { return pbn::philox_rk((uint32_t)ge, step_lo_k, pbn::gap_call_c2(0, jj), ge_hi, rk0, rk1); },
              [&](uint32_t u) { return gap_lut(lut, a.gap_shift, a.gap_nb, u); },
              [&](uint32_t u) { return (u >> a.gap_shift) >= (uint32_t)a.gap_nb; }, gam);
          pert = false;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            pert = pert || gam[w] != 0;
            slot[kGP + w * 64 + lane] = gam[w];
          }
          slot[kIN + lane] = rt | (pc << 8) | ((uint32_t)pert << 16);
          __builtin_amdgcn_s_setprio(0);
        }
      }
      PBN_PSTAMP(k, 1);
      lds_barrier();
      PBN_PSTAMP(k, 2);
    };
    // two steps per trip with the ENV words alternating between EA and EB: no copies between
    // steps; the block's last barrier (the state wave's step n_steps - 1) follows the loop
    Word4 EA = env_call(), EB = EA;
    for (int k = 0; k < n_steps; k += 2) {
      env_step(k, std::false_type{}, EA, EB);
      if (k + 1 < n_steps) env_step(k + 1, std::true_type{}, EB, EA);
    }
    PBN_PSTAMP(n_steps, 0);
    PBN_PSTAMP(n_steps, 1);
    lds_barrier();
    PBN_PSTAMP(n_steps, 2);
  } else if (role == 1) {
    // (in line: as a function of its own this loop changes the kernel's listing, tools/listing_diff.py)
    StepRows<uint32_t> fm_rows = rows_open(a.flipmask, n, (size_t)n_steps * plane);
    for (int k = 0; k <= n_steps; ++k) {
      asm volatile("" : "+s"(u_k0), "+s"(u_k1), "+s"(u_gx), "+s"(u_na), "+s"(u_mnf));
      asm volatile("" : "+s"(u_hb), "+s"(u_hp), "+s"(u_hz), "+s"(u_fl));
      PBN_PSTAMP(k, 0);
      if (k < n_steps) {
        // ---- env draws of step k, env `lane`
        uint32_t* slot = slots + (size_t)(k & 1) * a.slot_words;
        const uint64_t step = a.step + (uint64_t)k;
        const uint32_t st_lo = (uint32_t)step;
        const uint32_t ge_hi = (uint32_t)((ge >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16);
        const uint32_t ge_lo = (uint32_t)ge;
        // one ENV call: words 0, 1 = gaps 0, 1; X = words 3:2 gives, in order, the action draw
        // (every mode), the autoreset draws and gap 2's uniform u2 (DESIGN.md "Step semantics")
        const Word4 E = pbn::philox(ge_lo, st_lo, pbn::kStreamEnv << 28, ge_hi, u_k0, u_k1);
        StepRows<uint32_t> fm_k = fm_rows;   // (the store sits in a divergent arm: the step's advance here)
        rows_advance(fm_rows, plane);
        if (valid) {
          uint32_t m[W], gam[W], rs[W];
#pragma unroll
          for (int w = 0; w < W; ++w) { m[w] = 0; gam[w] = 0; rs[w] = 0; }
          uint32_t xhi = E.w, xlo = E.z;
          const uint32_t n1 = (uint32_t)(N + 1);
          const uint32_t c_act = ext64(xhi, xlo, n1 * n1 * n1);
          // X after the action and pair draws, X * x_mult mod 2^64, as one product off the
          // draws' dependency chain
          uint64_t xr = ((((uint64_t)E.w) << 32) | E.z) * a.x_mult;
          // autoreset draw (used by wave 0 only if the env's episode ends): (start, target) in
          // one draw over the A(A-1) pairs, then the state within the start attractor
          uint32_t rt;
          if (u_na >= 1) {
            const int32_t* att_first = reinterpret_cast<const int32_t*>(L + a.att_off);
            const uint32_t* att_words = L + a.att_off + u_na + 1;
            uint32_t as;
            pbn::pair_draw(xhi, xlo, (uint32_t)u_na, a.am1_magic, as, rt);
            const uint32_t row = pbn::start_pick(xhi, xlo, as, (u_fl & 16u) != 0,
                                                 [&](uint32_t i) { return att_first[i]; }, xr);
#pragma unroll
            for (int w = 0; w < W; ++w) rs[w] = att_words[(size_t)row * W + w];
          } else {
            rt = pbn::random_reset_state<W>(ge_lo, st_lo, ge_hi, u_k0, u_k1, N, rs);
          }
          const uint32_t u2 = (uint32_t)(xr >> 32);   // = xhi
          if (u_fl & 4u) {
            actions_from_draw<W>(c_act, N, a.n1_magic, m);
#pragma unroll
            for (int w = 0; w < W; ++w) rows_store(fm_k, w, (size_t)w * n, le, valid, 8, m[w]);
          } else {
#pragma unroll
            for (int w = 0; w < W; ++w)
              m[w] = LANE_AT(a.flipmask, k * plane + (size_t)w * n, le, (size_t)n_steps * plane, 6) & valid_word_mask(N, w);
          }
          uint32_t pc = 0;
#pragma unroll
          for (int w = 0; w < W; ++w) pc += __builtin_popcount(m[w]);
          int g0, g1, g2;
          first_gaps(u_gx, L, a, E.x, E.y, u2, g0, g1, g2);
          const int p2 = pbn::first_gaps_mask<W>(g0, g1, g2, N, gam);
          if (p2 < N - 1)   // rare: a fourth flip is possible
            pbn::gap_tail<W>(
                0u, 3, p2, N, E,
                [&](int jj) { return pbn::philox(ge_lo, st_lo, pbn::gap_call_c2(0, jj), ge_hi, u_k0, u_k1); },
                [&](uint32_t u) { return gap_any(u_gx, L, a, u); }, gam);
          bool pert = false;
#pragma unroll
          for (int w = 0; w < W; ++w) pert = pert || gam[w] != 0;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            slot[kFM + w * 64 + lane] = m[w];
            slot[kGP + w * 64 + lane] = gam[w];
            slot[kRS + w * 64 + lane] = rs[w];
          }
          slot[kIN + lane] = rt | (pc << 8) | ((uint32_t)pert << 16);
        }
      }
      PBN_PSTAMP(k, 1);
      lds_barrier();
    }
  } else if (role == 2 && W == 1 && u_mnf >= 2 && u_mnf <= kNodeRecs && u_hi_fixed) {
    // selection, single-word states with at most kNodeRecs functions per node: branch-free over
    // the lanes (lanes past N, single-function nodes and thresholds past a node's last compute
    // values the padded chain ignores), one loop per threshold count, and the next step's
    // SEL calls computed in the same block as this step's compares
    // (a lambda: as a function template over a context struct the kernel's register allocation changes)
    auto sel_fast = [&](auto nq_c) {
      constexpr int NQ = decltype(nq_c)::value;   // thresholds per node: max_nf - 1
      const uint32_t* cmi = cm + l32 * sel_mask_stride(B);
      uint32_t* lt_base = slots + kLT + half * 32 * W + l32;
      // the key schedule and the running step of the calls being computed, as in env_fast
      uint32_t rk0[pbn::kPhiloxRounds], rk1[pbn::kPhiloxRounds];
      pbn::philox_round_keys(k0, k1, rk0, rk1);
#pragma unroll
      for (int r = 0; r < pbn::kPhiloxRounds; ++r) asm volatile("" : "+s"(rk0[r]), "+s"(rk1[r]));
      // the Philox prefixes of the node's CPN calls, built once per lane (philox_prefix; pinned as
      // in env_fast): the calls differ in counter word 2 alone, so B and D are one pair for all of
      // them and A, E, d3 are per call
      const uint32_t G_hi = (uint32_t)((G >> 32) & 0xFFFFu) | ((uint32_t)(a.step >> 32) << 16);
      uint32_t step_lo = (uint32_t)a.step;
      uint32_t pre_B = 0, pre_D = 0, pre_A[CPN], pre_E[CPN], pre_d3[CPN];
#pragma unroll
      for (int c = 0; c < CPN; ++c) {
        const pbn::PhiloxPrefix p =
            pbn::philox_prefix((uint32_t)G, (pbn::kStreamSel << 28) | (uint32_t)(4 * l32 + c), G_hi, rk0, rk1);
        if (c == 0) { pre_B = p.B; pre_D = p.D; }
        pre_A[c] = p.A; pre_E[c] = p.E; pre_d3[c] = p.d3;
        asm volatile("" : "+v"(pre_A[c]), "+v"(pre_E[c]), "+v"(pre_d3[c]));
      }
      asm volatile("" : "+v"(pre_B), "+v"(pre_D));
      auto sel_calls = [&](uint32_t (&d)[16]) {
#pragma unroll
        for (int c = 0; c < CPN; ++c) {
          const Word4 o = pbn::philox_tail(pbn::PhiloxPrefix{pre_A[c], pre_B, pre_D, pre_E[c], pre_d3[c]}, step_lo,
                                           rk0, rk1);
          d[4 * c + 0] = o.x; d[4 * c + 1] = o.y; d[4 * c + 2] = o.z; d[4 * c + 3] = o.w;
        }
      };
      // one step: this step's compares from `cur`, the next step's calls into `nxt`
      auto sel_step = [&](int k, auto odd, const uint32_t (&cur)[16], uint32_t (&nxt)[16]) {
        PBN_ISA_LOOP("sel_fast", NQ);
        PBN_PSTAMP(k, 0);
        {
          step_advance(step_lo);
          sel_calls(nxt);   // (one unused set per launch)
#ifdef PBN_STAMPS
#pragma unroll
          for (int d = 0; d < 16; ++d) asm volatile("" : "+v"(nxt[d]));
#endif
          PBN_PSTAMP_AT(k, 18);
          uint32_t* lt_out = lt_base + (decltype(odd)::value ? (size_t)a.slot_words : (size_t)0);
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            lt_out[q * 64] = less_than_cm4<B>(cur, cmi + q * B);
          // keeps the next calls in this block (LLVM would sink them to the loop latch)
#pragma unroll
          for (int d = 0; d < 16; ++d) asm volatile("" : "+v"(nxt[d]));
        }
        PBN_PSTAMP(k, 1);
        lds_barrier();
        PBN_PSTAMP(k, 2);
      };
      // two steps per trip with the digit arrays swapping roles: no copies between steps
      uint32_t dA[16], dB[16];
#pragma unroll
      for (int d = 0; d < 16; ++d) { dA[d] = 0; dB[d] = 0; }
      sel_calls(dA);
      for (int k = 0; k < n_steps; k += 2) {
        sel_step(k, std::false_type{}, dA, dB);
        if (k + 1 < n_steps) sel_step(k + 1, std::true_type{}, dB, dA);
      }
      PBN_PSTAMP(n_steps, 0);
      PBN_PSTAMP(n_steps, 1);
      lds_barrier();   // the block's last barrier: the state wave's step n_steps - 1
      PBN_PSTAMP(n_steps, 2);
    };
    switch (u_mnf) {
      case 2: sel_fast(std::integral_constant<int, 1>{}); break;
      case 3: sel_fast(std::integral_constant<int, 2>{}); break;
      default: sel_fast(std::integral_constant<int, 3>{}); break;
    }
  } else if (role == 2) {
    // (in line: as a function of its own this loop changes the kernel's listing, tools/listing_diff.py)
    for (int k = 0; k <= n_steps; ++k) {
      asm volatile("" : "+s"(u_k0), "+s"(u_k1), "+s"(u_gx), "+s"(u_na), "+s"(u_mnf));
      asm volatile("" : "+s"(u_hb), "+s"(u_hp), "+s"(u_hz), "+s"(u_fl));
      PBN_PSTAMP(k, 0);
      if (k < n_steps) {
        // ---- selection masks of step k: node l32 + 32r of group g
        uint32_t* lt_out = slots + (size_t)(k & 1) * a.slot_words + kLT + half * 32 * W;
        const uint64_t step = a.step + (uint64_t)k;
        const uint32_t st_lo = (uint32_t)step;
        const uint32_t G_hi = (uint32_t)((G >> 32) & 0xFFFFu) | ((uint32_t)((step >> 32) & 0xFFFFu) << 16);
        const uint32_t G_lo = (uint32_t)G;
#pragma unroll
        for (int r = 0; r < W; ++r) {
          const int i = l32 + 32 * r;
          const int ic = i < N ? i : 0;
          const uint4 r0 = recL[ic];
          if (valid && i < N && (int)r0.w > 1) {
            uint32_t dig[16];
#pragma unroll
            for (int c = 0; c < CPN; ++c) {
              const Word4 o = pbn::philox(G_lo, st_lo, (pbn::kStreamSel << 28) | (uint32_t)(4 * i + c), G_hi, u_k0, u_k1);
              dig[4 * c + 0] = o.x; dig[4 * c + 1] = o.y; dig[4 * c + 2] = o.z; dig[4 * c + 3] = o.w;
            }
            const int nf = (int)r0.w;
            {   // per-lane thresholds: the selection wave has slack, the SGPRs are scarce
#pragma unroll
              for (int q = 0; q < kNodeRecs - 1; ++q)
                if (q < nf - 1) {
                  if constexpr (W == 1)
                    lt_out[q * 64 * W + i] = less_than_cm<B>(dig, cm + i * sel_mask_stride(B) + q * B, 1);
                  else
                    lt_out[q * 64 * W + i] = less_than(dig, recL[q * 32 * W + ic].z, B);
                }
              if constexpr (MANY) {   // nodes with more than kNodeRecs functions
                const int f0 = (int)recL[32 * W + ic].w;
                for (int j = kNodeRecs - 1; j < nf - 1; ++j)
                  lt_out[j * 64 * W + i] = less_than(dig, a.fcompact[CK(f0 + j, a.n_funcs, 9)].z, B);
              }
            }
          }
        }
      }
      PBN_PSTAMP(k, 1);
      lds_barrier();
    }
  } else {
    // the state wave.  (in line: as a function of its own over a context struct this role changes the kernel's listing, tools/listing_diff.py)
    // the epilogue of step t (after the back-transpose): perturbed envs, outputs, attractor
    // hash, reward, flags, autoreset
    // the per-step outputs, one descriptor each (a null obs / final_state: stores dropped)
    StepRows<uint32_t> obs_rows = rows_open(a.obs, n, (size_t)n_steps * plane);
    StepRows<uint32_t> fin_rows = rows_open(a.final_state, n, (size_t)n_steps * plane);
    StepRows<float> rwd_rows = rows_open(a.reward, n, (size_t)n_steps * n);
    StepRows<uint8_t> flg_rows = rows_open(a.flags, n, (size_t)n_steps * n);
    // launch invariants as values instead of tests in the loop: no truncation is a horizon no
    // step count reaches (t <= 255)
    u_hz = u_hz > 0 ? u_hz : 0x7FFFFFFF;
    // the hash's shift (32 - bits) instead of its bit count: 32 = no attractor table
    int u_hs = u_hb > 0 ? 32 - u_hb : 32;
    auto store_obs = [&](const uint32_t (&s)[W]) {
#pragma unroll
      for (int w = 0; w < W; ++w) rows_store(obs_rows, w, (size_t)w * n, le, valid, 7, s[w]);
      rows_advance(obs_rows, plane);
    };
    auto finish = [&](bool autoreset, uint32_t (&sp)[W], const uint32_t (&s1)[W], const uint32_t (&gam)[W],
                      const uint32_t (&rs)[W], uint32_t info) {
      {
        // branch-free epilogue (this wave bounds the iteration), unguarded stores (StepRows)
        const bool pert = (info >> 16) & 1u;
        const uint32_t pc = (info >> 8) & 0xFFu;
#pragma unroll
        for (int w = 0; w < W; ++w) sp[w] = pert ? (s1[w] ^ gam[w]) : sp[w];
#pragma unroll
        for (int w = 0; w < W; ++w) rows_store(fin_rows, w, (size_t)w * n, le, valid, 10, sp[w]);
        rows_advance(fin_rows, plane);
        // reward candidates depend only on popcount(flipmask): one 16-byte row {none, wrong,
        // term, -} read beside the hash
        const float4 r4 = reinterpret_cast<const float4*>(rtab)[pc];
        const float r_none = r4.x, r_wrong = r4.y, r_term = r4.z;
        int att = -1;
        if (u_hs < 32) {
          uint32_t h = 0;
#pragma unroll
          for (int w = 0; w < W; ++w) h += sp[w] * a.hash_mult[w];
          h >>= u_hs;
          // the table is usually collision-free (one probe, h < 2^bits needs no mask); keys
          // are unique, so probe order does not matter
          att = hash_probe<W>(htab, h, sp);
          // further probes (a table with collisions) are a rolled loop behind an unlikely branch,
          // out of line: unrolled in line, their ~150 instructions sat in the hot loop behind a
          // branch taken every step
          if (__builtin_expect(u_hp > 1, 0)) {
            const uint32_t hmask = 0xFFFFFFFFu >> u_hs;
#pragma nounroll
            for (int pr = 1; pr < u_hp; ++pr) {
              const int id = hash_probe<W>(htab, (h + pr) & hmask, sp);
              if (id >= 0) att = id;
            }
          }
        }
        // (pbn::step_outcome restated, the horizon test as a value: through the helper the state
        // wave's epilogue gains a scalar instruction)
        const bool in_attr = att >= 0;
        const bool term = in_attr && (uint32_t)att == tg0;
        const bool wrong = in_attr && !term;
        int tt = (int)tt0 + 1;
        tt = tt > 255 ? 255 : tt;
        const bool trunc = tt >= u_hz;   // (no horizon: INT_MAX)
        const bool reset = autoreset && (term || trunc);
        const uint32_t fl = (uint32_t)term | ((uint32_t)trunc << 1) | ((uint32_t)in_attr << 2) |
                            ((uint32_t)pert << 3) | ((uint32_t)reset << 4);
        rows_store(rwd_rows, 0, 0, le, valid, 11, __float_as_uint(term ? r_term : (wrong ? r_wrong : r_none)));
        rows_store(flg_rows, 0, 0, le, valid, 15, fl);   // (fl < 32: one byte)
        rows_advance(rwd_rows, (size_t)n);
        rows_advance(flg_rows, (size_t)n);
        tg0 = reset ? (info & 0xFFu) : tg0;
        tt0 = reset ? 0u : (uint32_t)tt;
#pragma unroll
        for (int w = 0; w < W; ++w) st[w] = reset ? rs[w] : sp[w];
      }
    };
    if (W == 1 && u_mnf >= 1 && u_mnf <= kNodeRecs) {
      // single-word states with at most kNodeRecs functions per node: the loop-invariant record
      // inputs held in VGPRs, and this step's selection masks and selectors read before the
      // transpose, so that their LDS latency is off the chain slot -> transpose -> gathers ->
      // mux trees -> back-transpose
      auto state_fast = [&](auto k_c) {
        constexpr int K = decltype(k_c)::value;
        uint32_t ins[K];
#pragma unroll
        for (int q = 0; q < K; ++q) ins[q] = recL[q * 32 + l32].x;
        // iteration 0 (the other waves produce step 0) is the barrier alone, peeled; iteration
        // k >= 1 runs step t = k - 1 from slot t & 1, whose byte offset toggles by one s_xor
        PBN_PSTAMP(0, 0);
        PBN_PSTAMP(0, 1);
        lds_barrier();
        PBN_PSTAMP(0, 2);
        PBN_RSTAMP(3);
        uint32_t slot_bytes = 0;
        const uint32_t slot_toggle = (uint32_t)a.slot_words * 4u;
        // the one launch-invariant condition left in this loop, held as a lane mask
        const bool autoreset = (u_fl & 8u) != 0;
        for (int k = 1; k <= n_steps; ++k) {
          asm volatile("" : "+s"(u_hs), "+s"(u_hp), "+s"(u_hz));
          // the 4K plane addresses of the gathers are re-derived from ins[] every step: hoisted
          // out of the loop they are 4K more live VGPRs, one was spilled, and its reload's
          // s_waitcnt vmcnt(0) waited on the step's streaming stores in the middle of the chain
#pragma unroll
          for (int q = 0; q < K; ++q) asm volatile("" : "+v"(ins[q]));
          PBN_ISA_LOOP("state_fast", K);
          PBN_PSTAMP(k, 0);
          {
            const uint32_t* slot = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(slots) + slot_bytes);
            slot_bytes ^= slot_toggle;
            const uint32_t* lt_in = slot + kLT + half * 32 + l32;
            uint32_t s1[W], gam[W], rs[W];
            s1[0] = st[0] ^ slot[kFM + lane];
            gam[0] = slot[kGP + lane];
            rs[0] = slot[kRS + lane];
            const uint32_t info = slot[kIN + lane];
            uint32_t ltv[K];
            uint4 sa[K], sb[K];
#pragma unroll
            for (int q = 0; q < K; ++q) {
              ltv[q] = q < K - 1 ? lt_in[q * 64] : 0u;
              sa[q] = selq[(2 * q) * 32 + l32];
              sb[q] = selq[(2 * q + 1) * 32 + l32];
            }
            store_obs(st);
            PBN_PSTAMP_AT(k, 15);
            Sg[l32] = lane_transpose32(s1[0], lane);
            __builtin_amdgcn_wave_barrier();
            PBN_PSTAMP_AT(k, 3);
            uint32_t x = 0;
#pragma unroll
            for (int q = K - 1; q >= 0; --q) {
              uint32_t xin[4];
#pragma unroll
              for (int kk = 0; kk < 4; ++kk) xin[kk] = plane_in<true>(Sg, ins[q], kk);
              const uint32_t fj = eval_sel_in(xin, sa[q], sb[q]);
              x = (q == K - 1) ? fj : bfi(ltv[q], fj, x);
            }
            PBN_PSTAMP_AT(k, 12);
            uint32_t sp[W];
            sp[0] = lane_transpose32(x, lane);
            PBN_PSTAMP_AT(k, 13);
            finish(autoreset, sp, s1, gam, rs, info);
          }
          PBN_PSTAMP(k, 1);
          lds_barrier();
          PBN_PSTAMP(k, 2);
          if (k == 1) PBN_RSTAMP(4);
        }
      };
      switch (u_mnf) {
        case 1: state_fast(std::integral_constant<int, 1>{}); break;
        case 2: state_fast(std::integral_constant<int, 2>{}); break;
        case 3: state_fast(std::integral_constant<int, 3>{}); break;
        default: state_fast(std::integral_constant<int, 4>{}); break;
      }
    } else
    for (int k = 0; k <= n_steps; ++k) {
      asm volatile("" : "+s"(u_k0), "+s"(u_k1), "+s"(u_gx), "+s"(u_na), "+s"(u_mnf));
      asm volatile("" : "+s"(u_hs), "+s"(u_hp), "+s"(u_hz), "+s"(u_fl));
      PBN_PSTAMP(k, 0);
      if (k >= 1) {
        // ---- state part of step t = k - 1
        const int t = k - 1;
        const uint32_t* slot = slots + (size_t)(t & 1) * a.slot_words;
        const uint32_t* lt_in = slot + kLT + half * 32 * W;
        uint32_t s1[W], gam[W], rs[W];
        uint32_t info = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          s1[w] = st[w] ^ slot[kFM + w * 64 + lane];
          gam[w] = slot[kGP + w * 64 + lane];
          rs[w] = slot[kRS + w * 64 + lane];
        }
        info = slot[kIN + lane];
        store_obs(st);
#pragma unroll
        for (int w = 0; w < W; ++w) Sg[32 * w + l32] = lane_transpose32(s1[w], lane);
        __builtin_amdgcn_wave_barrier();
        PBN_PSTAMP_AT(k, 3);
        uint32_t X[W];
        if (!MANY || u_mnf <= kNodeRecs) {
#pragma unroll
          for (int r = 0; r < W; ++r) {
            int i = l32 + 32 * r;
            asm volatile("" : "+v"(i));   // selector and record reads stay in the step loop
            const uint4* rc = recL + i;
            const uint4* sel = selq + i;
            const uint32_t* lti = lt_in + i;
            switch (u_mnf) {
              case 1: X[r] = chain_padded<1, (W <= 2)>(rc, sel, 32 * W, Sg, lti, 64 * W); break;
              case 2: X[r] = chain_padded<2, (W <= 2)>(rc, sel, 32 * W, Sg, lti, 64 * W); break;
              case 3: X[r] = chain_padded<3, (W <= 2)>(rc, sel, 32 * W, Sg, lti, 64 * W); break;
              default: X[r] = chain_padded<4, (W <= 2)>(rc, sel, 32 * W, Sg, lti, 64 * W); break;
            }
          }
        } else
#pragma unroll
        for (int r = 0; r < W; ++r) {
          const int i = l32 + 32 * r;
          int ii = i < N ? i : 0;
          asm volatile("" : "+v"(ii));   // selector and record reads stay in the step loop
          uint4 rec_r[kNodeRecs];
#pragma unroll
          for (int q = 0; q < kNodeRecs; ++q) rec_r[q] = recL[q * 32 * W + ii];
          const int nf = (int)rec_r[0].w;
          uint32_t x = 0;
          if (u_mnf > kNodeRecs) {   // chain tail of nodes with more than kNodeRecs functions
            const int f0 = (int)rec_r[1].w;
            for (int j = nf - 1; j >= kNodeRecs; --j) {
              const uint4 rc = a.fcompact[CK(f0 + j, a.n_funcs, 9)];
              const uint32_t fj = eval_compact(rc.x, rc.y, Sg);
              x = (j == nf - 1) ? fj : bfi(lt_in[j * 64 * W + ii], fj, x);
            }
          }
          const uint4* sel = selq + ii;
          const uint32_t* lti = lt_in + ii;
          switch (u_mnf) {
            case 1: x = chain_from_masks<1, (W <= 2)>(rec_r, sel, 32 * W, Sg, lti, 64 * W, nf, u_mnf > kNodeRecs, x); break;
            case 2: x = chain_from_masks<2, (W <= 2)>(rec_r, sel, 32 * W, Sg, lti, 64 * W, nf, u_mnf > kNodeRecs, x); break;
            case 3: x = chain_from_masks<3, (W <= 2)>(rec_r, sel, 32 * W, Sg, lti, 64 * W, nf, u_mnf > kNodeRecs, x); break;
            default: x = chain_from_masks<4, (W <= 2)>(rec_r, sel, 32 * W, Sg, lti, 64 * W, nf, u_mnf > kNodeRecs, x); break;
          }
          X[r] = i < N ? x : 0u;
        }
        PBN_PSTAMP_AT(k, 12);
        uint32_t sp[W];
#pragma unroll
        for (int w = 0; w < W; ++w) sp[w] = lane_transpose32(X[w], lane);
        PBN_PSTAMP_AT(k, 13);
        finish((u_fl & 8u) != 0, sp, s1, gam, rs, info);
      }
      PBN_PSTAMP(k, 1);
      lds_barrier();
      PBN_PSTAMP(k, 2);
    }
    PBN_RSTAMP(5);
    if (valid) {
#pragma unroll
      for (int w = 0; w < W; ++w) a.state_out[CK((size_t)w * n + le, plane, 16)] = st[w];
      a.t[CK(le, n, 17)] = (uint8_t)tt0;
      a.target[CK(le, n, 18)] = (uint8_t)tg0;
    }
#ifdef PBN_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    PBN_RSTAMP(6);
#endif
  }
}

}  // namespace
