// learn_args.h -- what the fused BDQ update's three kernels (learn_fwd.h, learn_bwd.h,
// learn_apply.h) and the pack kernels (bdq_pack.h) share: the launch arguments, the diagnostic
// phase clocks and two one-line helpers.  The shapes and layouts behind the arguments are
// bdq_layout.h's.
//
// Parameters, Adam's moments and the gradient share one layout (pbn_bdq_layout): the module's
// nn.Parameters are views into it (pbn_rl_amd/replay.py FusedBDQUpdate), so the acting kernel,
// the checkpoint and the PyTorch forward all see the same weights.  Row sets and activations
// are [feature][batch] in the workspace: both MFMA operands of a gradient tile are float4 loads
// along the batch.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/pbn_env.h"
#include "bdq_layout.h"
#include "wave_util.h"

namespace {

using namespace bdq;

constexpr int kWaves = kLearnWaves;
constexpr int kThreads = 64 * kWaves;

struct LearnArgs {
  // the replay ring and the sampled rows
  const int64_t* idx;
  int B;
  int64_t cap;
  const uint32_t* st;
  const uint32_t* nst;
  const uint8_t* tgt;
  const int32_t* act;
  const float* rew;
  const uint8_t* done;
  // the network's attractor table (first state of attractor t: the target half of the input)
  const uint32_t* att_first;   // [n_attr][W]
  int n_attr, N, W, K, H, A, Apad;
  // parameters (online, updated in place; target, read), their target tables, Adam's state
  float* P;
  float* Tq;          // the online network's image (its table, then the weight tiles: bdq_layout.h make_image)
  const float* PT;
  const float* TqT;   // the target network's
  int64_t ifw[NLAY], ibw[NLAY];   // the weight tiles' offsets in the images
  float* m;
  float* v;
  float* step;
  int64_t off[TOTAL + 1];
  float lr, b1, b2, eps, gamma, clampv, slope;
  // workspace (bdq_layout.h PBN_BDQ_WORK: the planes and their shapes)
#define PBN_X(type, name, n) type* name;
  PBN_BDQ_WORK(PBN_X)
#undef PBN_X
  float* loss;
  float* grad;    // optional: the clamped gradient, parameter layout
  // prioritised replay (pbn_bdq_learn_per; learn_bwd_kernel<true>): the rows' importance weights
  // in, their priorities out, both by batch position; null / 0 otherwise
  const float* wts;   // [B]
  float* prio;        // [B]
  float rconst;
  unsigned long long* stamps;   // diagnostic builds (PBN_STAMPS): [kernel][block][wave][32] s_memtime
  // the frame's counters and the next frame's rows (pbn_frame_advance): learn_apply's extra last
  // block, when adv_on
  int adv_on;
  pbn_frame_advance adv;
};

// Diagnostic phase clocks (tools/learn_stamps.py): lane 0 of every wave of the first 1,024 blocks
// stores s_memtime at numbered points of each kernel (below), and s_memrealtime at entry (31)
constexpr int kLStampRow = 32;
#ifdef PBN_STAMPS
#define PBN_LSTAMP(k, i)                                                                                      \
  do {                                                                                                      \
    if (a.stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 1024)                                           \
      a.stamps[(((size_t)(k) * 1024 + blockIdx.x) * 8 + (threadIdx.x >> 6)) * kLStampRow + (i)] =           \
          (i) == 31 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();                      \
  } while (0)
#else
#define PBN_LSTAMP(k, i) do {} while (0)
#endif

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : x * slope; }

__device__ __forceinline__ int64_t row_index(const LearnArgs& a, int b) {
  const int64_t j = a.idx[b];
  return j < 0 ? 0 : (j >= a.cap ? a.cap - 1 : j);   // (sample_indices keeps 0 <= j < size)
}

// the network's shape, and where its parameters and its image's weight tiles lie; the image's layout
inline ImageLayout set_shape(LearnArgs& a, int N, int W, int n_attr, const uint32_t* att_first, int n_branches) {
  a.att_first = att_first;
  a.n_attr = n_attr;
  a.N = N;
  a.W = W;
  a.K = n_branches;
  a.H = n_branches + 1;
  a.A = N + 1;
  a.Apad = apad(N);
  make_layout(N, a.H, a.off);
  ImageLayout im;
  make_image(N, a.H, n_attr, &im);
  for (int l = 0; l < NLAY; ++l) {
    a.ifw[l] = im.fwd[l];
    a.ibw[l] = im.bwd[l];
  }
  return im;
}

// the workspace pointers, from the one workspace layout
inline void set_workspace(LearnArgs& a, void* d_workspace, const Work& w) {
  float* ws = static_cast<float*>(d_workspace);
#define PBN_X(type, name, n) a.name = reinterpret_cast<type*>(ws + w.name);
  PBN_BDQ_WORK(PBN_X)
#undef PBN_X
}

}  // namespace
