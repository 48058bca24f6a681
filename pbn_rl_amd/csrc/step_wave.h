// step_wave.h -- pbn_step_wave, the step kernel with one wave per 32-env group (pbn_step, the
// lean rollout, the settle-law variants, the policy rollout), and what it alone uses: the
// threshold classes, the gate levels of lowered wide functions, the node updates and the
// settle law's update loop.
#pragma once
#include "step_parts.h"

namespace {

// ------------------------------------------- step kernel, one wave per 32-env group
//
// Lane j of the wave is env j (lanes 0-31) for the per-env work and node j (+32r) for
// the node work.  Blocks of kWavesPerBlock waves share one LDS copy of the tables; all
// global loads are issued before the Philox batch so their latency hides under it.
//   1. Philox: the lower half computes each env's ENV call and the first half of
//      its node's selection calls, the upper half the other selection calls plus
//      each env's first continuation-gap call; results meet via lane swaps;
//   2. per env (lower lanes): interventions, perturbation (gap = linear count
//      against the CDF in SGPRs for N <= 32), reset word;
//   3. 32x32 bit transposes as 5-stage cross-lane butterflies on DPP
//      (quad_perm, row_ror) and v_permlane16_swap: lane p ends up holding plane p;
//   4. lane i evaluates node i; selection digits stay in its registers;
//   5. butterfly back to per-env words, reward/termination/autoreset, stores.

// (u < c_q) for the wave-uniform threshold classes: one bit-sliced comparison per class with
// SGPR digit masks, then a per-lane pick by class index (record .y)
template <int B>
__device__ __forceinline__ void class_masks(const uint32_t (&dig)[16], const uint32_t (&uthr)[kNodeRecs], int n_cls,
                                            uint32_t (&ltc)[kNodeRecs]) {
#pragma unroll
  for (int v = 0; v < kNodeRecs; ++v) {
    ltc[v] = 0;
    if (v < n_cls) {
      uint32_t c = uthr[v];
      asm volatile("" : "+s"(c));   // digits re-extracted per step on the SALU (hoisted: SGPR spills)
      ltc[v] = less_than(dig, c, B);
    }
  }
}

__device__ __forceinline__ uint32_t pick_class(const uint32_t (&ltc)[kNodeRecs], uint32_t cls) {
  return cls == 0 ? ltc[0] : (cls == 1 ? ltc[1] : (cls == 2 ? ltc[2] : ltc[3]));
}

// Lower lanes receive the upper lanes' four words (upper lanes end with junk): per pair of
// words two v_permlane32_swap and no copies.  swap(X, Y) moves X's upper half into Y's
// lower half; swap(Y', X') then moves Y's upper half into X''s lower half.
__device__ __forceinline__ pbn::Word4 upper_to_lower(pbn::Word4 v) {
  const auto a1 = __builtin_amdgcn_permlane32_swap(v.x, v.y, false, false);
  const auto a2 = __builtin_amdgcn_permlane32_swap(a1[1], a1[0], false, false);
  const auto b1 = __builtin_amdgcn_permlane32_swap(v.z, v.w, false, false);
  const auto b2 = __builtin_amdgcn_permlane32_swap(b1[1], b1[0], false, false);
  return pbn::Word4{a2[0], a2[1], b2[0], b2[1]};
}

// combinational gates of the lowered wide functions (lowering.py), level by level, all 64 lanes:
// gate record {input S indices, 16-bit table, output S index}; one wave's LDS operations execute
// in order, so level l + 1 reads what level l wrote
__device__ __forceinline__ void eval_gate_levels(const StepArgs& a, const uint32_t* __restrict__ L, uint32_t* S,
                                                 int lane) {
  const uint4* grec = reinterpret_cast<const uint4*>(L + a.gate_off);
  const int32_t* glev = reinterpret_cast<const int32_t*>(L + a.glayer_off);
  for (int lv = 0; lv < a.n_glayers; ++lv) {
    const int end = glev[lv + 1];
    for (int gi = glev[lv] + lane; gi < end; gi += 64) {
      const uint4 r = grec[gi];
      S[r.z] = eval_compact(r.x, r.y, S);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// node l32 + 32r on lane l32: the rule update of every env of the group from the bit-sliced
// planes S, the selection digit planes dig (perturbed envs are replaced by the caller)
template <int W, int B>
__device__ __forceinline__ void node_update(const StepArgs& a, const uint4 (&rec_)[W][kNodeRecs],
                                            const uint4* __restrict__ selq, const uint32_t* __restrict__ S,
                                            const uint32_t (&dig)[W][16], bool lo, int l32, uint32_t (&X)[W]) {
  const int N = a.n_nodes;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    X[r] = 0;
    const int i = l32 + 32 * r;
    const int ii = lo && i < N ? i : 0;   // other lanes evaluate node 0 and discard it
    uint32_t x = 0;
    if (a.n_cls > 0 && a.max_nf <= kNodeRecs) {
      // thresholds from a few wave-uniform classes (all kaban networks: 1/3, 2/3)
      const int nf = (int)rec_[r][0].w;
      uint32_t ltc[kNodeRecs];
      class_masks<B>(dig[r], a.uthr, a.n_cls, ltc);
#pragma unroll
      for (int q = kNodeRecs - 1; q >= 0; --q) {
        if (q < a.max_nf) {
          const uint4 rc = rec_[r][q];
          const uint32_t fj = eval_sel(rc.x, selq[(2 * q) * 32 * W + ii], selq[(2 * q + 1) * 32 * W + ii], S);
          const uint32_t y = (q == nf - 1) ? fj : bfi(pick_class(ltc, rc.y), fj, x);
          x = (q < nf) ? y : x;
        }
      }
    } else {
      const int nf = (int)rec_[r][0].w;
      const int f0 = (int)rec_[r][1].w;
      // selection chain from the last function down: x = F_{nf-1}; x = lt_j ? F_j : x
      for (int j = nf - 1; j >= kNodeRecs; --j) {   // nodes with more than kNodeRecs functions (slow path)
        const uint4 rc = a.fcompact[CK(f0 + j, a.n_funcs, 9)];
        const uint32_t fj = eval_compact(rc.x, rc.y, S);
        x = (j == nf - 1) ? fj : bfi(less_than(dig[r], rc.z, B), fj, x);
      }
#pragma unroll
      for (int q = kNodeRecs - 1; q >= 0; --q) {
        if (q < nf) {
          const uint4 rc = rec_[r][q];
          const uint32_t fj = eval_sel(rc.x, selq[(2 * q) * 32 * W + ii], selq[(2 * q + 1) * 32 * W + ii], S);
          x = (q == nf - 1) ? fj : bfi(less_than(dig[r], rc.z, B), fj, x);
        }
      }
    }
    if (lo && i < N) X[r] = x;
  }
}

// settle law: node l32 + 32r's rule update on lane l32 (lower lanes) from the planes S, with env
// l32's per-env selection uniforms of update k (settle_sel_words; every lane computes its env's
// words, the upper half repeating the lower's: the settle variants are off the hot path).  The
// chain runs from the widest node's last function down (uniform q); threshold q's plane of every
// node is compared env-major and transposed once per q, so that only one word's uniforms are live.
template <int W, int B>
__device__ __forceinline__ void node_update_settle(const StepArgs& a, const uint4 (&rec_)[W][kNodeRecs],
                                                   const uint4* __restrict__ selq, const uint32_t* __restrict__ S,
                                                   uint32_t ge_lo, uint32_t ge_hi, uint32_t st_lo, uint32_t k,
                                                   int lane, uint32_t (&X)[W]) {
  const int N = a.n_nodes;
  const bool lo = lane < 32;
  const int l32 = lane & 31;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const int mnf = a.max_nf;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    X[r] = 0;
    const int i = l32 + 32 * r;
    const int ii = lo && i < N ? i : 0;   // other lanes evaluate node 0 and discard it
    uint32_t U[16];
    settle_sel_words(ge_lo, ge_hi, st_lo, k, r, N, k0, k1, U);
    const int nf = (int)rec_[r][0].w;
    const int f0 = (int)rec_[r][1].w;
    uint32_t x = 0;
    for (int q = mnf - 1; q >= 0; --q) {
      uint32_t pl = 0;
      if (q < mnf - 1) pl = lane_transpose32(settle_lt_word(U, a.sthr + (size_t)(q * W + r) * 32), lane);
      if (q < nf) {
        uint32_t fq;
        if (q < kNodeRecs) {
          const uint4 rc = q == 0 ? rec_[r][0] : (q == 1 ? rec_[r][1] : (q == 2 ? rec_[r][2] : rec_[r][3]));
          fq = eval_sel(rc.x, selq[(2 * q) * 32 * W + ii], selq[(2 * q + 1) * 32 * W + ii], S);
        } else {
          const uint4 rc = a.fcompact[CK(f0 + q, a.n_funcs, 9)];
          fq = eval_compact(rc.x, rc.y, S);
        }
        x = (q == nf - 1) ? fq : bfi(pl, fq, x);
      }
    }
    if (lo && i < N) X[r] = x;
  }
}

// The settle law (settle_max >= 2, include/pbn_env.h "Step law"): updates k = 1 ..
// settle_max - 1 of the envs (lower lanes) whose state sp is outside every attractor, until all
// of the wave's envs are in one.  Update k: perturbation gaps j = 0, 1, ... from the SETTLE_ENV
// stream (pbn::gap_tail, per env); unperturbed envs take the rule update with their own
// SETTLE_SEL uniforms of update k (node_update_settle).  Returns true on lanes whose env is
// still outside after the last update (PBN_FLAG_UNSETTLED).
template <int W, int B>
__device__ __forceinline__ bool settle_updates(const StepArgs& a, const uint32_t* __restrict__ L, uint32_t* S,
                                            const uint4 (&rec_)[W][kNodeRecs], int lane, uint32_t ge_lo,
                                            uint32_t ge_hi, uint32_t st_lo, uint32_t (&sp)[W], int& att, bool& pert,
                                            uint32_t& nupd, bool live) {
  const bool lo = lane < 32;
  const int l32 = lane & 31;
  const int N = a.n_nodes;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const uint4* selq = reinterpret_cast<const uint4*>(L + a.sel_off);
  const uint32_t* htab = L + a.cdf_len + 4 * (N + 1);
  bool open = live && att < 0;   // (envs past n_envs take part in the transposes only)
  for (int k = 1; k < a.settle_max; ++k) {
    if (__ballot(open) == 0) return false;
    uint32_t gam[W];
    bool pk = false;
#pragma unroll
    for (int w = 0; w < W; ++w) gam[w] = 0;
    if (open) {   // every gap of the update through the tail: from word 0, position -1
      pbn::gap_tail<W>(
          (uint32_t)k, 0, -1, N, Word4{0, 0, 0, 0},
          [&](int jj) { return pbn::philox(ge_lo, st_lo, pbn::gap_call_c2((uint32_t)k, jj), ge_hi, k0, k1); },
          [&](uint32_t u) { return gap_any(a.gap_exact, L, a, u); }, gam);
#pragma unroll
      for (int w = 0; w < W; ++w) pk = pk || gam[w] != 0;
    }
    // bit-slice sp (every lane takes part in the cross-lane transposes)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t pl = lane_transpose32(sp[w], lane);
      if (lo) S[32 * w + l32] = pl;
    }
    __builtin_amdgcn_wave_barrier();
    if (a.n_glayers > 0) eval_gate_levels(a, L, S, lane);
    uint32_t X[W], x[W];
    node_update_settle<W, B>(a, rec_, selq, S, ge_lo, ge_hi, st_lo, (uint32_t)k, lane, X);
#pragma unroll
    for (int w = 0; w < W; ++w) x[w] = lane_transpose32(X[w], lane);
    if (open) {
#pragma unroll
      for (int w = 0; w < W; ++w) sp[w] = pk ? sp[w] ^ gam[w] : x[w];
      pert = pert || pk;
      ++nupd;
      att = attractor_lookup<W>(a, htab, sp);
      open = att < 0;
    }
  }
  return open;
}

// VARIANT 1: exactly one step (pbn_step; no loop, lowest VGPR count);
// 2: rollout with invariants recomputed per step (occupancy first; the rollout of networks
//    with gates, which the pipelined kernel does not run);
// 3, 4: 1 and 2 under the settle law (settle_max >= 2: settle_updates after the first update).
// POL: empty, or PolicyArgs (the policy rollout, pbn_rollout_dqn; variants 2 and 4): a second kernel
// argument, the DQN whose action on the env's current (state, target) is the step's flip mask, a
// third source beside the in-kernel random actions and a given mask.
template <class P>
__device__ __forceinline__ const P& policy_arg(const P& p) { return p; }

template <int W, int B, int VARIANT, class... POL>
__global__ void __launch_bounds__(64 * kWavesPerBlock) pbn_step_wave(StepArgs a, POL... pol) {
  constexpr bool LEAN = VARIANT == 2 || VARIANT == 4;
  constexpr bool POLICY = sizeof...(POL) == 1;
  static_assert(sizeof...(POL) <= 1 && (!POLICY || LEAN), "the policy is evaluated in the multi-step loop");
  constexpr bool SINGLE = VARIANT == 1 || VARIANT == 3;
  constexpr bool SETTLE = VARIANT >= 3;
  constexpr int CPN = SETTLE ? 0 : B / 4;  // group selection calls per node (the settle law's are per env)
  constexpr int H = (CPN + 1) / 2;         // of which the lower half computes H
  constexpr int NLO = 1 + W * H;           // lower list: ENV, SEL(c < H)
  constexpr int NUP = W * (CPN - H);       // upper list: SEL(c >= H)
  constexpr int IT = NLO > NUP ? NLO : NUP;
  constexpr int UPC = (CPN - H) > 0 ? (CPN - H) : 1;  // divisor guard (B = 4: no upper calls)
  extern __shared__ uint32_t smem[];   // carved below; sized by wave_lds_words (net_layout.h)
  PBN_STAMP(0);
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  const int N = a.n_nodes;
  // LDS: the block's table image [cdf | reward | hash | attractors | leaf selectors], then
  // each wave's S planes
  uint32_t* L = smem;
  uint32_t* S = smem + a.tab_words + (size_t)wv * a.wave_words;
  const float* rtab = reinterpret_cast<const float*>(L + a.cdf_len);
  const uint32_t* htab = L + a.cdf_len + 4 * (N + 1);
  const int64_t n = a.n_envs;
  const bool lo = lane < 32;
  const int l32 = lane & 31;
  const int64_t le = g * 32 + l32;
  const uint64_t ge = a.env_offset + (uint64_t)le;
  const uint64_t G = ge >> 5;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const bool random_actions = (a.mode & PBN_MODE_RANDOM_ACTIONS) != 0;
  const size_t plane = (size_t)W * n;   // words per step of a [steps][W][n] output
  // env le exists (pbn_step takes any n_envs: the last group may be ragged; its other lanes
  // compute, take part in the cross-lane work, and load or store nothing)
  const bool live = lo && le < n;

  // ---- 0. issue the one-time global loads: env state, node records, tables
  uint32_t st[W];      // current observation s of env l32 (lower lanes), carried across steps
  uint32_t tt0 = 0, tg0 = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] = 0;
  if (live) {   // (waves past the end only help copy the tables; the bits past N are cleared after
                // the barrier: an AND here waited for the load ahead of the records and the image)
#pragma unroll
    for (int w = 0; w < W; ++w) st[w] = a.state[CK((size_t)w * n + le, plane, 1)];
    tt0 = a.t[CK(le, n, 2)];
    tg0 = a.target[CK(le, n, 3)];
  }
  // pbn_step_dev_store: the transition's row, and the env's branch actions requested now
  // (unguarded, clamped: a guarded load's select would wait for it here, ahead of the node records
  // and the table image); the row is written after the step (s, the target, the actions, s'
  // before an autoreset, the reward, done)
  // one-step launches: the step index (pbn_step_dev) and the env's flip mask requested here too
  // (after the barrier each was a round trip of its own before the Philox calls and the update)
  uint64_t step_pre = a.step;
  uint32_t mpre[W];
  if constexpr (SINGLE) {
    if (a.step_ptr) step_pre = *a.step_ptr;
    const int64_t lc = le < n ? le : n - 1;   // (unguarded; random-action launches ignore it)
#pragma unroll
    for (int w = 0; w < W; ++w) mpre[w] = a.flipmask[CK((size_t)w * n + lc, plane, 6)];
  }
  int64_t rj = 0;
  int32_t rav[kRingMaxK];
  if constexpr (!SETTLE) {
    if (a.r_state) {
      rj = (int64_t)(((uint64_t)*a.r_pos + (uint64_t)le) % (uint64_t)a.r_cap);
      const int64_t lc = le < n ? le : n - 1;
#pragma unroll
      for (int k = 0; k < kRingMaxK; ++k)
        rav[k] = a.r_act_in[CK((size_t)lc * a.r_k + (k < a.r_k ? k : a.r_k - 1), (size_t)n * a.r_k, 43)];
    }
  }
  // node l32 + 32r: its first kNodeRecs compact records {inputs, table, threshold, meta}
  // (node-major, fixed stride: no dependent load); meta of record 0 = nf, of record 1 = f0
  uint4 rec_[W][kNodeRecs];
#pragma unroll
  for (int r = 0; r < W; ++r) {
    const int i = l32 + 32 * r;
    const int ic = i < N ? i : 0;
#pragma unroll
    for (int q = 0; q < kNodeRecs; ++q) rec_[r][q] = a.nrec[CK((size_t)ic * kNodeRecs + q, N * kNodeRecs, 4)];
  }
  copy_image(L, a);
  __syncthreads();   // the kernel's only block barrier
  if (g >= a.n_groups) return;  // whole wave
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] &= valid_word_mask(N, w);
  asm volatile("" : "+v"(tt0), "+v"(tg0));   // (their first uses here, not hoisted above the barrier)
  const uint4* selq = reinterpret_cast<const uint4*>(L + a.sel_off);

  const int n_steps = SINGLE ? 1 : a.n_steps;
  // Random-action mode issues no global load inside the step loop (attractor tables live in
  // LDS), so stores never have to drain (vmcnt retires in issue order).  A given flip mask
  // is loaded and consumed inside its own branch, so the wait for it stays on that path.
  for (int ks = 0; ks < n_steps; ++ks) {
  if constexpr (LEAN) {
    // keep loop-invariant expansions (leaf masks, threshold digits, key schedule, first-round
    // products) inside the loop so VGPRs stay low and occupancy high
#pragma unroll
    for (int r = 0; r < W; ++r) {
#pragma unroll
      for (int q = 0; q < kNodeRecs; ++q) {
        asm volatile("" : "+v"(rec_[r][q].x), "+v"(rec_[r][q].z));
      }
    }
  }
  const uint32_t kk0 = k0, kk1 = k1, ge_lo = (uint32_t)ge, G_lo = (uint32_t)G;
  uint64_t step = a.step + (uint64_t)ks;
  if constexpr (SINGLE) step = step_pre;   // (by value, or pbn_step_dev's device step index)
  const uint32_t st_lo = (uint32_t)step;
  const uint32_t st_hi = (uint32_t)((step >> 32) & 0xFFFFu) << 16;
  const uint32_t ge_hi = (uint32_t)((ge >> 32) & 0xFFFFu) | st_hi;
  const uint32_t G_hi = (uint32_t)((G >> 32) & 0xFFFFu) | st_hi;
  uint32_t m[W], s1[W];
#pragma unroll
  for (int w = 0; w < W; ++w) { m[w] = 0; s1[w] = st[w]; }
  if (live && a.obs) {
#pragma unroll
    for (int w = 0; w < W; ++w) a.obs[CK(ks * plane + (size_t)w * n + le, (size_t)n_steps * plane, 7)] = st[w];
  }

  // ---- 0p. the policy's flip mask: Q of the wave's 32 envs in two 16-row passes of dqn_act's
  // forward (the whole wave: the MFMAs), the argmax, the EXPLORE draw.  The forward reads the
  // state and the target the step before left in st / tg0, an autoreset's new target included.
  if constexpr (POLICY) {
    const PolicyArgs* p = &policy_arg(pol...);
    const Dims& d = p->d;
    const int qg = lane >> 4, r16 = lane & 15;
    int greedy[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {   // lane 16 qg + r16 works on env 16 ps + r16
      uint32_t sw[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t x = w < W ? (uint32_t)__shfl((int)st[w < W ? w : 0], 16 * ps + r16) : 0u;
        if (w == d.W - 1 && (d.N & 31)) x &= (1u << (d.N & 31)) - 1u;   // (as load_words)
        sw[w] = x;
      }
      const int t = __shfl((int)tg0, 16 * ps + r16);
      float4 y0[kMaxHT], y1[kMaxHT];
      float best = -INFINITY;
      int bi = INT_MAX;
      // (PRELOAD: the same arithmetic with the dense layers' operands requested early; the wave
      // has its SIMD to itself, so nothing else hides a round trip)
      forward16<true>(d, p->img, sw, t, lane, y0, y1, [&](int at, f32x4 q) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int ai = 16 * at + 4 * qg + v;
          if (ai < d.A && better(q[v], ai, best, bi)) {
            best = q[v];
            bi = ai;
          }
        }
      });
      greedy[ps] = row_argmax(best, bi);
    }
    // env l32's argmax: lane l32 & 15 of pass l32 >> 4
    const int g0 = __shfl(greedy[0], r16), g1 = __shfl(greedy[1], r16);
    if (lo) {
      // EXPLORE law (DESIGN.md "Step semantics" 6), as dqn_act_kernel
      const Word4 rw = pbn::draw(a.seed, ge, a.step + (uint64_t)ks, pbn::kStreamExplore, 0);
      const int act = (uint64_t)rw.x < p->eps_u ? (int)__umulhi(rw.y, (uint32_t)d.A) : ((l32 >> 4) ? g1 : g0);
#pragma unroll
      for (int w = 0; w < W; ++w) m[w] = action_mask_word(act, N, w);
      if (live) {
#pragma unroll
        for (int w = 0; w < W; ++w) a.flipmask[CK(ks * plane + (size_t)w * n + le, (size_t)n_steps * plane, 48)] = m[w];
        if (p->actions) p->actions[CK(ks * n + le, n_steps * n, 49)] = act;
      }
    }
  }

  // ---- 1. all Philox calls of the group, two half-wave work lists
  PBN_STAMP(1);
  Word4 out[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    uint32_t lc0, lc2, lc3, uc0, uc2, uc3;
    if (it == 0) {
      lc0 = ge_lo; lc2 = pbn::kStreamEnv << 28; lc3 = ge_hi;
    } else {
      constexpr int HD = H > 0 ? H : 1;   // (the settle variants have no group selection calls)
      const int idx = it - 1;
      const int r = (idx / HD) < W ? idx / HD : W - 1;
      const int c = idx % HD;
      lc0 = G_lo; lc2 = (pbn::kStreamSel << 28) | (uint32_t)(4 * (l32 + 32 * r) + c); lc3 = G_hi;
    }
    if (it < W * (CPN - H)) {
      const int r = it / UPC;
      const int c = H + it % UPC;
      uc0 = G_lo; uc2 = (pbn::kStreamSel << 28) | (uint32_t)(4 * (l32 + 32 * r) + c); uc3 = G_hi;
    } else {   // (upper list done: a discarded call)
      uc0 = ge_lo; uc2 = pbn::kStreamEnv << 28; uc3 = ge_hi;
    }
    out[it] = pbn::philox(lo ? lc0 : uc0, st_lo, lo ? lc2 : uc2, lo ? lc3 : uc3, kk0, kk1);
  }
  // digits of node l32 + 32r: calls c < H from this lane, c >= H from lane + 32
  uint32_t dig[W][16];
#pragma unroll
  for (int r = 0; r < W; ++r) {
#pragma unroll
    for (int c = 0; c < CPN; ++c) {
      const Word4 d = c < H ? out[(1 + r * H + c) < IT ? (1 + r * H + c) : 0]
                            : upper_to_lower(out[r * (CPN - H) + (c - H)]);
      dig[r][4 * c + 0] = d.x; dig[r][4 * c + 1] = d.y; dig[r][4 * c + 2] = d.z; dig[r][4 * c + 3] = d.w;
    }
  }
  const Word4 E = out[0];

  // ---- 2. per env (lower lanes): interventions, perturbation, reset word
  PBN_STAMP(2);
  uint32_t gam[W];
  uint32_t pc = 0;
  bool pert = false;
#pragma unroll
  for (int w = 0; w < W; ++w) gam[w] = 0;
  // ENV words 3:2 = a 64-bit uniform X: the action draw (every mode), the autoreset draws,
  // then gap 2's uniform u2 = what remains of X's top word (DESIGN.md "Step semantics")
  uint32_t r_row = 0, r_nt = 0, u2 = 0;
  if (lo) {
    uint32_t xhi = E.w, xlo = E.z;
    const uint32_t n1 = (uint32_t)(N + 1);
    const uint32_t c_act = ext64(xhi, xlo, n1 * n1 * n1);
    if (a.n_attr >= 1) {
      const int32_t* att_first = reinterpret_cast<const int32_t*>(L + a.att_off);
      uint32_t as;
      uint64_t xr = 0;   // (u2 is taken from the chain here)
      pbn::pair_draw(xhi, xlo, (uint32_t)a.n_attr, a.am1_magic, as, r_nt);
      r_row = pbn::start_pick(xhi, xlo, as, a.att_single != 0, [&](uint32_t i) { return att_first[i]; }, xr);
    }
    u2 = xhi;
    if constexpr (POLICY) {
      // (m is the policy's, above)
    } else if (random_actions) {
      actions_from_draw<W>(c_act, N, a.n1_magic, m);
      if (live) {
#pragma unroll
        for (int w = 0; w < W; ++w) a.flipmask[CK(ks * plane + (size_t)w * n + le, (size_t)n_steps * plane, 8)] = m[w];
      }
    } else if (live) {
#pragma unroll
      for (int w = 0; w < W; ++w)
        m[w] = (SINGLE ? mpre[w] : a.flipmask[CK(ks * plane + (size_t)w * n + le, (size_t)n_steps * plane, 6)]) &
               valid_word_mask(N, w);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
      pc += __builtin_popcount(m[w]);
      s1[w] ^= m[w];
    }
    // perturbation positions are prefix sums of geometric gaps; the first three gaps
    // (u = E.x, E.y, u2) are independent, so they are computed side by side
    int g0, g1, g2;
    first_gaps(a.gap_exact, L, a, E.x, E.y, u2, g0, g1, g2);
    const int p2 = pbn::first_gaps_mask<W>(g0, g1, g2, N, gam);
    if (p2 < N - 1)   // rare: a fourth flip is possible
      pbn::gap_tail<W>(
          0u, 3, p2, N, E,
          [&](int jj) { return pbn::philox(ge_lo, st_lo, pbn::gap_call_c2(0, jj), ge_hi, kk0, kk1); },
          [&](uint32_t u) { return gap_any(a.gap_exact, L, a, u); }, gam);
#pragma unroll
    for (int w = 0; w < W; ++w) pert = pert || gam[w] != 0;
  }

  // ---- 3. bit-slice s1: lane p <- plane p (node p over the 32 envs), to LDS
  PBN_STAMP(3);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const uint32_t sp = lane_transpose32(s1[w], lane);
    if (lo) S[32 * w + l32] = sp;
  }
  __builtin_amdgcn_wave_barrier();
  if (a.n_glayers > 0) eval_gate_levels(a, L, S, lane);

  // ---- 4. node l32 + 32r on lane l32: X = rule update of every env (perturbed envs are
  // replaced after the back-transpose)
  PBN_STAMP(4);
  uint32_t X[W];
  if constexpr (SETTLE) node_update_settle<W, B>(a, rec_, selq, S, ge_lo, ge_hi, st_lo, 0u, lane, X);
  else node_update<W, B>(a, rec_, selq, S, dig, lo, l32, X);

  // ---- 5. back to per-env words, reward, termination, autoreset, stores
  PBN_STAMP(5);
  uint32_t sp[W];
#pragma unroll
  for (int w = 0; w < W; ++w) sp[w] = lane_transpose32(X[w], lane);
  PBN_STAMP(6);
  if (lo && pert) {
#pragma unroll
    for (int w = 0; w < W; ++w) sp[w] = s1[w] ^ gam[w];
  }
  int att = lo ? attractor_lookup<W>(a, htab, sp) : 0;
  bool unsettled = false;
  uint32_t nupd = 1;   // synchronous updates applied this step
  if constexpr (SETTLE) {   // the whole wave (cross-lane transposes)
    unsettled = settle_updates<W, B>(a, L, S, rec_, lane, ge_lo, ge_hi, st_lo, sp, att, pert, nupd, live);
  }
  if (live) {
  if constexpr (!SINGLE) {
    if (a.updates) a.updates[CK(ks * n + le, n_steps * n, 23)] = (uint16_t)min(nupd, 0xFFFFu);
  }
  if (a.final_state) {
#pragma unroll
    for (int w = 0; w < W; ++w) a.final_state[CK(ks * plane + (size_t)w * n + le, (size_t)n_steps * plane, 10)] = sp[w];
  }
  if constexpr (!SETTLE) {
    if (a.r_state) {   // (st and tg0 are still the step's inputs here: the autoreset comes below)
#pragma unroll
      for (int w = 0; w < W; ++w) {
        a.r_state[CK((size_t)w * a.r_cap + rj, (size_t)W * a.r_cap, 40)] = st[w];
        a.r_next[CK((size_t)w * a.r_cap + rj, (size_t)W * a.r_cap, 44)] = sp[w];
      }
      a.r_target[CK(rj, a.r_cap, 41)] = (uint8_t)tg0;
#pragma unroll
      for (int k = 0; k < kRingMaxK; ++k)
        if (k < a.r_k) a.r_action[CK((size_t)rj * a.r_k + k, (size_t)a.r_cap * a.r_k, 42)] = rav[k];
    }
  }
  const pbn::StepOutcome o = pbn::step_outcome(att, tg0, tt0, a.horizon, (a.mode & PBN_MODE_AUTORESET) != 0, pert,
                                               unsettled);
  const float rwd = rtab[(int)pc * 4 + pbn::reward_slot(o)];
  a.reward[CK(ks * n + le, n_steps * n, 11)] = rwd;
  if (o.reset) {
    if (a.n_attr >= 1) {   // the attractor draws of step 2 (attractor states from the LDS image)
      const uint32_t* att_words = L + a.att_off + a.n_attr + 1;
#pragma unroll
      for (int w = 0; w < W; ++w) sp[w] = att_words[(size_t)r_row * W + w];
      tg0 = r_nt;
    } else {
      tg0 = pbn::random_reset_state<W>(ge_lo, st_lo, ge_hi, kk0, kk1, N, sp);
    }
  }
  a.flags[CK(ks * n + le, n_steps * n, 15)] = (uint8_t)o.flags;
  if constexpr (!SETTLE) {
    if (a.r_state) {   // done as pbn_replay_store derives it from the flags byte
      const uint8_t d = a.r_done_mask ? ((o.flags & a.r_done_mask) ? 1 : 0) : ((uint8_t)o.flags ? 1 : 0);
      a.r_reward[CK(rj, a.r_cap, 45)] = rwd;
      a.r_done[CK(rj, a.r_cap, 46)] = d;
      if (a.r_done_out) a.r_done_out[CK(le, n, 47)] = d;
    }
  }
  tt0 = o.t;
#pragma unroll
  for (int w = 0; w < W; ++w) st[w] = sp[w];
  }  // live
  PBN_STAMP(7);
  }  // steps

  if (live) {
#pragma unroll
    for (int w = 0; w < W; ++w) a.state_out[CK((size_t)w * n + le, plane, 16)] = st[w];
    a.t[CK(le, n, 17)] = (uint8_t)tt0;
    a.target[CK(le, n, 18)] = (uint8_t)tg0;
  }
}

}  // namespace
