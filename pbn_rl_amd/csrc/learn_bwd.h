// learn_bwd.h -- the second of the fused BDQ update's three launches (pbn_learn.hip):
//
//   learn_bwd    B/16 blocks.  The TD error of bdq_update per (transition, branch): both duelings,
//                the online argmax over s', the target network's value there, the MSE's partial
//                sum, and the gradient at the head outputs; then the backward through the heads
//                and the trunk (transposed MFMA tiles, LeakyReLU derivative from the stored
//                activation), storing every layer's delta.  With importance weights
//                (pbn_bdq_learn_per, the <true> instantiation) the TD pass scales each row's
//                gradient by its weight and writes the row's priority.
#pragma once
#include "learn_args.h"

namespace {

// ---- backward tiles: dX[k][r] = sum_o W[o][k] dY[o][r] for the 16 inputs k0..k0+15 (A operand
// lane l: W[o][k0 + (l & 15)] for the k-step's o = 16 ob + 4g + v; B operand: the blocked dY
// plane, as the forward's X).  The accumulator holds dX[k0 + 4g + v][r].  Fragments (bwd_frag)
// are loaded ahead of the layer that uses them (bwd_mma).
// times LeakyReLU' (from the stored activation: y > 0 exactly when its input was), into the
// blocked LDS plane (rows kk0..) when Ys is set and the [K][B] plane
// the stored activations a backward tile's derivative needs (loaded ahead, like the weights)
__device__ __forceinline__ f32x4 act_frag(const float* __restrict__ act, int kk0, int B, int b0, int lane) {
  const int g = lane >> 4, rr = lane & 15;
  f32x4 y;
#pragma unroll
  for (int v = 0; v < 4; ++v) y[v] = act[(size_t)(kk0 + 4 * g + v) * B + b0 + rr];
  return y;
}

__device__ __forceinline__ void bwd_store(f32x4 acc, f32x4 yv, int kk0, float slope, float* __restrict__ Ys,
                                          float* __restrict__ out, int B, int b0, int lane) {
  const int g = lane >> 4, rr = lane & 15;
  float4 d;
  float* dp = &d.x;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int k = kk0 + 4 * g + v;
    const float y = yv[v];
    dp[v] = y > 0.f ? acc[v] : acc[v] * slope;
    out[(size_t)k * B + b0 + rr] = dp[v];
  }
  if (Ys) *reinterpret_cast<float4*>(Ys + ((kk0 >> 4) * 16 + rr) * 16 + 4 * g) = d;
}

// a layer's weight fragments for bwd_mma: input tile kt of a layer with KT input tiles, NOB
// output blocks from ob0, from its bwd tiles in the image (0 past n_ob)
template <int NOB>
__device__ __forceinline__ void bwd_frag(float (&w)[NOB][4], const float* __restrict__ tiles, int KT, int kt, int ob0,
                                         int n_ob, int lane) {
#pragma unroll
  for (int u = 0; u < NOB; ++u) {
    const bool ok = ob0 + u < n_ob;
    const float4 x = reinterpret_cast<const float4*>(tiles)[((size_t)(ok ? ob0 + u : 0) * KT + kt) * 64 + lane];
    w[u][0] = ok ? x.x : 0.f;
    w[u][1] = ok ? x.y : 0.f;
    w[u][2] = ok ? x.z : 0.f;
    w[u][3] = ok ? x.w : 0.f;
  }
}

template <int NOB>
__device__ __forceinline__ f32x4 bwd_mma(f32x4 acc, const float (&w)[NOB][4], int ob0, int n_ob,
                                         const float* __restrict__ dYs, int lane) {
  const int g = lane >> 4, rr = lane & 15;
#pragma unroll
  for (int u = 0; u < NOB; ++u) {
    if (ob0 + u < n_ob) {
      const float4 y = *reinterpret_cast<const float4*>(dYs + ((ob0 + u) * 16 + rr) * 16 + 4 * g);
      acc = mfma(w[u][0], y.x, acc);
      acc = mfma(w[u][1], y.y, acc);
      acc = mfma(w[u][2], y.z, acc);
      acc = mfma(w[u][3], y.w, acc);
    }
  }
  return acc;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

// kPer (pbn_bdq_learn_per): the TD pass is td_loss_kernel<true>'s (pbn_agent.hip).  Batch row b
// carries an importance weight w_b, read by batch position (a batch may hold a ring row twice):
// l_b = (sum_k (expected - current)^2, k ascending) / K, g is the unweighted g times w_b,
// priority[b] = |w_b l_b| + replay_constant, and the block's partial is the sum of its w_b l_b
// (learn_apply divides the total by B: loss = mean_b w_b l_b).  Everything after the pass is the
// same code; without kPer the kernel is the unweighted one, expression for expression.
template <bool kPer>
__global__ void __launch_bounds__(kThreads) learn_bwd_kernel(LearnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // carved by BwdLds (bdq_layout.h), which also sizes it
  const int H = a.H, A = a.A, Ap = a.Apad, K = a.K, B = a.B;
  const BwdLds at(H, Ap, K);
  float* DH = lds + at.dh;
  // (DHH's offset in line and the trunk from DHH: as lds + at.dhh() and lds + at.trunk() the
  // kernel's listing changes, tools/listing_diff.py)
  float* DHH = DH + H * Ap * kRows;   // = lds + at.dhh()
  float* trunk = DHH + at.dhh_words();
  float* DH4 = trunk + at.dh4;
  float* DH3 = trunk + at.dh3;
  float* DH2 = trunk + at.dh2;
  float* part = trunk + at.part;
  float* sg = lds + at.td();   // (past the TD pass's staged heads)
  float* sd = sg + at.td_words();
  int* sact = reinterpret_cast<int*>(sd + at.td_words());
  const int tile = blockIdx.x, b0 = tile * kRows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, rr = lane & 15;
  const float* Tw = a.Tq;   // the online network's weight tiles
  PBN_LSTAMP(1, 31);
  PBN_LSTAMP(1, 0);
  // Issue order (vmcnt retires in order: a wait for a load waits for every load issued before
  // it): the TD pass's operands first -- the sampled rows' indices, the block's head rows, then
  // the rows' actions, rewards and done flags -- and only then the weight fragments and stored
  // activations the backward layers need after the pass, so that the pass waits for its own loads
  // alone (it waited for all of them; profiles/r06_ad_bwd_issue_order_ab.json)
  float* SH = lds + at.sh;   // the staged head rows
  const int pitch = at.pitch();
  const int per4 = kRows * Ap / 4;   // float4s of one (set, head) block of rows
  const int n4 = 3 * H * per4;
  // the TD pass: four lanes per (row r, branch k) pair p = tid >> 2 (r = p & 15, k = p >> 4)
  const bool tdl = tid < 4 * kRows * K;
  const int tp = tid >> 2, tq = tid & 3;
  int64_t jrow = 0;
  if (tdl) jrow = row_index(a, b0 + (tp & 15));
  int64_t jw = 0;   // wave 7: the rows' words for learn_apply
  const bool wrow = tid >= 64 * (kWaves - 1) && tid - 64 * (kWaves - 1) < kRows;
  if (wrow) jw = row_index(a, b0 + tid - 64 * (kWaves - 1));
  constexpr int kHeadPre = 4;   // head float4s per thread issued ahead (n4 <= 2048: every K <= 3 shape
                                // with N <= 31; more in the loop below)
  float4 hv[kHeadPre];
  auto head_src = [&](int e) __attribute__((always_inline)) {
    const int sh = e / per4, f = e - sh * per4;   // sh = set * H + h
    return reinterpret_cast<const float4*>(a.heads + ((size_t)sh * B + b0) * Ap)[f];
  };
  auto head_dst = [&](int e) __attribute__((always_inline)) {
    const int sh = e / per4, f = e - sh * per4;
    const int r = f / (Ap / 4), c = f - r * (Ap / 4);
    return reinterpret_cast<float4*>(SH + ((size_t)sh * kRows + r) * pitch + 4 * c);
  };
#pragma unroll
  for (int k = 0; k < kHeadPre; ++k) hv[k] = head_src(min(tid + kThreads * k, n4 - 1));
  int ak = 0;
  float rwj = 0.f, dnj = 0.f, wj = 1.f;
  if (tdl) {
    ak = a.act[(size_t)jrow * K + (tp >> 4)];
    rwj = a.rew[jrow];
    dnj = (float)a.done[jrow];
    if constexpr (kPer) wj = a.wts[b0 + (tp & 15)];   // (with the pass's other operands: issue order above)
  }
  if (wrow) {
    const int b = b0 + tid - 64 * (kWaves - 1);
    const int tg = a.tgt[jw];
    for (int w = 0; w < a.W; ++w) {
      a.srow[(size_t)w * B + b] = a.st[(size_t)w * a.cap + jw];
      a.trow[(size_t)w * B + b] = tg < a.n_attr ? a.att_first[(size_t)tg * a.W + w] : 0u;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // the weight fragments of the first four backward layers: second head layers (tiles wave, wave
  // + 8 of H x 4), the first head layers split four ways per output tile (wave & 1 = tile, wave >> 1
  // = quarter of the 4 H blocks), 32 -> 64 (waves < 4) and 64 -> 128
  const int at16 = Ap / 16;
  float wh2[2][2][4], wh1[8][4], w4[2][4], w3[4][4];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tt = min(wave + kWaves * u, H * (kDH / 16) - 1), h = tt >> 2;
    bwd_frag<2>(wh2[u], Tw + a.ibw[LYH2] + (size_t)h * at16 * (kDH / 16) * 256, kDH / 16, tt & 3, 0, at16, lane);
  }
  const int q1 = wave >> 1;   // quarter of the first head layers' 4 H output blocks: [q H, q H + H)
  bwd_frag<8>(wh1, Tw + a.ibw[LYH1], kD3 / 16, wave & 1, q1 * H, q1 * H + H, lane);
  bwd_frag<2>(w4, Tw + a.ibw[LY4], kD2 / 16, wave & 3, 0, kD3 / 16, lane);
  bwd_frag<4>(w3, Tw + a.ibw[LY3], kD1 / 16, wave, 0, kD2 / 16, lane);
  // and the stored activations of the same tiles (the LeakyReLU derivative)
  f32x4 yh2[2], y4 = act_frag(a.h4, 16 * (wave & 1), B, b0, lane), y3 = act_frag(a.h3, 16 * (wave & 3), B, b0, lane),
        y2 = act_frag(a.h2, 16 * wave, B, b0, lane), y1v[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tt = min(wave + kWaves * u, H * (kDH / 16) - 1);
    yh2[u] = act_frag(a.hh, (tt >> 2) * kDH + 16 * (tt & 3), B, b0, lane);
    y1v[u] = act_frag(a.y1, 16 * (wave + kWaves * u), B, b0, lane);
  }
  __builtin_amdgcn_sched_barrier(0);
  PBN_LSTAMP(1, 1);

  // the TD error per (row, branch): bdq_update / update_policy (:111-126) on the raw heads.  The
  // block's head rows of the three sets come into LDS (coalesced; the staging area is the delta
  // planes', written only after this pass), then thread (row r, branch k) runs the duelings and
  // the online argmax over s' as sequential sums (the order of pbn_bdq_td_loss).
#pragma unroll
  for (int k = 0; k < kHeadPre; ++k)
    if (tid + kThreads * k < n4) *head_dst(tid + kThreads * k) = hv[k];
  for (int e = tid + kThreads * kHeadPre; e < n4; e += kThreads) *head_dst(e) = head_src(e);
  ak = ak < 0 ? 0 : (ak >= A ? A - 1 : ak);
  lds_barrier();
  PBN_LSTAMP(1, 2);
  if (tdl) {
    const int r = tp & 15, k = tp >> 4;
    auto hrow = [&](int set, int h) { return SH + ((size_t)(set * H + h) * kRows + r) * pitch; };
    const float* adv0 = hrow(0, k + 1);
    const float* adv1 = hrow(1, k + 1);
    const float* adv2 = hrow(2, k + 1);
    // the three duelings' means: lane tq < 3 sums set tq's row in order (eight LDS reads in
    // flight, the next eight requested before these are added); the means to every lane of the pair
    const float* mine = tq == 0 ? adv0 : (tq == 1 ? adv1 : adv2);
    float ssum = 0.f;
    float xc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) xc[u] = mine[min(u, A - 1)];
    for (int o0 = 0; o0 < A; o0 += 8) {
      float xn[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) xn[u] = mine[min(o0 + 8 + u, A - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (o0 + u < A) ssum += xc[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) xc[u] = xn[u];
    }
    const float mq = ssum / (float)A;   // (lane 3: a fourth copy of set 2's, unused)
    const int l0 = lane & ~3;
    const float m0 = __shfl(mq, l0), m1 = __shfl(mq, l0 + 1), m2 = __shfl(mq, l0 + 2);
    // the online argmax over s' (torch.argmax: first maximum, NaN is the maximum): each lane scans
    // a quarter of actions 1 .. A-1 with the sequential rule, then the quarters are combined in
    // order with the same rule (which makes the combination the sequential scan's result)
    const float v1 = hrow(1, 0)[0];
    const int seg = (A - 1 + 3) / 4, lo = 1 + tq * seg, hi = min(lo + seg, A);
    bool have = lo < hi;
    float best = 0.f;
    int am = 0;
    if (have) {
      best = (v1 + adv1[lo]) - m1;
      am = lo;
      for (int o = lo + 1; o < hi; ++o) {
        const float qo = (v1 + adv1[o]) - m1;
        const bool take = !isnan(best) && (isnan(qo) || qo > best);
        best = take ? qo : best;
        am = take ? o : am;
      }
    }
    float gbest = (v1 + adv1[0]) - m1;
    int gam = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float b = __shfl(best, l0 + q);
      const int ai = __shfl(am, l0 + q);
      const bool h = __shfl((int)have, l0 + q) != 0;
      const bool take = h && !isnan(gbest) && (isnan(b) || b > gbest);
      gbest = take ? b : gbest;
      gam = take ? ai : gam;
    }
    if (tq == 0) {
      const float current = (hrow(0, 0)[0] + adv0[ak]) - m0;
      const float tnext = (hrow(2, 0)[0] + adv2[gam]) - m2;
      const float expected = rwj + (tnext * a.gamma) * dnj;
      const float d = expected - current;
      sd[r * K + k] = d * d;
      const float gk = 2.f * (current - expected) / (float)(B * K);
      sg[r * K + k] = kPer ? gk * wj : gk;
      sact[r * K + k] = ak;
    }
  }
  PBN_LSTAMP(1, 3);
  lds_barrier();
  PBN_LSTAMP(1, 4);
  // the gradient at the head outputs: d/d adv[k][o] = g_k ([o == a_k] - 1/A), d/d v = sum_k g_k
  // (0 for the value head's other outputs and the padding)
  for (int e = tid; e < H * Ap * kRows; e += kThreads) {
    const int oi = e & 15, r = (e >> 4) & 15, hb = e >> 8;   // hb = h * Apad/16 + o/16
    const int h = hb / at16, o = 16 * (hb - h * at16) + oi;
    float val = 0.f;
    if (o < A) {
      if (h == 0) {
        if (o == 0)
          for (int k = 0; k < K; ++k) val += sg[r * K + k];
      } else {
        const float gk = sg[r * K + h - 1];
        val = (o == sact[r * K + h - 1] ? gk : 0.f) - gk / (float)A;
      }
    }
    DH[e] = val;
    a.dheads[((size_t)h * Ap + o) * B + b0 + r] = val;
  }
  if (wave == 0) {   // the block's squared TD errors, a fixed-order reduction
    float sacc = 0.f;
    if constexpr (kPer) {
      // lane r < 16: row r's weighted loss and priority.  Row r's weight is in lane 4 r of this
      // wave (pair p = r: branch 0 of row r; 4 * 16 * K >= 64, so those lanes ran the pass)
      const float wr = __shfl(wj, 4 * rr);
      if (lane < kRows) {
        float l = 0.f;
        for (int k = 0; k < K; ++k) l += sd[lane * K + k];
        sacc = wr * (l / (float)K);
        a.prio[b0 + lane] = fabsf(sacc) + a.rconst;
      }
    } else {
      for (int p = lane; p < kRows * K; p += 64) sacc += sd[p];
    }
    sacc = wave_sum(sacc);
    if (lane == 0) {
      a.partial[tile] = sacc;
      if (tile == 0) a.step[0] += 1.f;   // Adam's step count, read by learn_apply
    }
  }
  lds_barrier();
  // the last layer's fragments (256 inputs: tiles wave, wave + 8), requested now for the end
  float w2[2][8][4];
#pragma unroll
  for (int u = 0; u < 2; ++u) bwd_frag<8>(w2[u], Tw + a.ibw[LY2], kD0 / 16, wave + kWaves * u, 0, kD1 / 16, lane);
  // second head layers: Apad -> 64 per head
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tt = wave + kWaves * u;
    if (tt < H * (kDH / 16)) {
      const int h = tt >> 2, c0 = 16 * (tt & 3);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = bwd_mma<2>(acc, wh2[u], 0, at16, DH + h * Ap * kRows, lane);
      for (int ob0 = 2; ob0 < at16; ob0 += 2) {   // (A > 32)
        float wl[2][4];
        bwd_frag<2>(wl, Tw + a.ibw[LYH2] + (size_t)h * at16 * (kDH / 16) * 256, kDH / 16, c0 / 16, ob0, at16, lane);
        acc = bwd_mma<2>(acc, wl, ob0, at16, DH + h * Ap * kRows, lane);
      }
      bwd_store(acc, yh2[u], h * kDH + c0, a.slope, DHH, a.dhh, B, b0, lane);
    }
  }
  for (int tt = wave + 2 * kWaves; tt < H * (kDH / 16); tt += kWaves) {   // (H > 4)
    const int h = tt >> 2, c0 = 16 * (tt & 3);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int ob0 = 0; ob0 < at16; ob0 += 2) {
      float wl[2][4];
      bwd_frag<2>(wl, Tw + a.ibw[LYH2] + (size_t)h * at16 * (kDH / 16) * 256, kDH / 16, c0 / 16, ob0, at16, lane);
      acc = bwd_mma<2>(acc, wl, ob0, at16, DH + h * Ap * kRows, lane);
    }
    bwd_store(acc, act_frag(a.hh, h * kDH + c0, B, b0, lane), h * kDH + c0, a.slope, DHH, a.dhh, B, b0, lane);
  }
  PBN_LSTAMP(1, 5);
  lds_barrier();
  PBN_LSTAMP(1, 6);
  {   // first head layers: 64 H -> 32, each output tile split over four waves (H blocks each)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = bwd_mma<8>(acc, wh1, q1 * H, q1 * H + H, DHH, lane);
    *reinterpret_cast<f32x4*>(part + (wave * 64 + lane) * 4) = acc;
  }
  lds_barrier();
  if (wave < kD3 / 16) {   // the four quarters added in order
    f32x4 acc = *reinterpret_cast<const f32x4*>(part + (wave * 64 + lane) * 4);
#pragma unroll
    for (int qq = 1; qq < 4; ++qq) acc += *reinterpret_cast<const f32x4*>(part + ((wave + 2 * qq) * 64 + lane) * 4);
    bwd_store(acc, y4, 16 * wave, a.slope, DH4, a.dh4, B, b0, lane);
  }
  lds_barrier();
  PBN_LSTAMP(1, 7);
  if (wave < kD2 / 16) {   // 32 -> 64
    const f32x4 acc = bwd_mma<2>(f32x4{0.f, 0.f, 0.f, 0.f}, w4, 0, kD3 / 16, DH4, lane);
    bwd_store(acc, y3, 16 * wave, a.slope, DH3, a.dh3, B, b0, lane);
  }
  lds_barrier();
  {   // 64 -> 128
    const f32x4 acc = bwd_mma<4>(f32x4{0.f, 0.f, 0.f, 0.f}, w3, 0, kD2 / 16, DH3, lane);
    bwd_store(acc, y2, 16 * wave, a.slope, DH2, a.dh2, B, b0, lane);
  }
  lds_barrier();
  PBN_LSTAMP(1, 8);
#pragma unroll
  for (int u = 0; u < 2; ++u) {   // 128 -> 256: the bilinear layer's output gradient
    const f32x4 acc = bwd_mma<8>(f32x4{0.f, 0.f, 0.f, 0.f}, w2[u], 0, kD1 / 16, DH2, lane);
    bwd_store(acc, y1v[u], 16 * (wave + kWaves * u), a.slope, nullptr, a.g1, B, b0, lane);
  }
  PBN_LSTAMP(1, 9);
  (void)g;
  (void)rr;
}

}  // namespace
