// net_layout.h -- what the host-side descriptor compiler (net_image.h), the launcher
// (pbn_env.hip) and the kernels (step_kernels.h) must agree on: table strides, the LDS carving
// of the three step kernels, the LDS limits and the choice of kernel for a launch.  Plain
// C++17, free of HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PBN_HD __host__ __device__
#else
#define PBN_HD
#endif

namespace {

constexpr int kNodeRecs = 4;       // compact records prefetched per node by the wave kernel
constexpr int kWavesPerBlock = 4;  // wave kernel: waves (32-env groups) per block, sharing one LDS table image
constexpr int kMaxHashBits = 12;

constexpr size_t kLdsDeviceBytes = 160 * 1024;   // LDS of one CU: no block may ask for more
constexpr size_t kLdsPipeBytes = 64 * 1024;      // the pipelined kernels' limit (two blocks per CU)

// words per slot of the attractor hash: W key words and the id, rounded up to a power of two
PBN_HD constexpr int hash_stride(int W) { return W == 1 ? 2 : (W <= 3 ? 4 : 8); }

// pbn_rollout_pipe's threshold digit masks, lane-major: node i's masks of threshold q, digit d at
// cm[i * S + q * B + d], S = sel_mask_stride(B) words: four masks are one 16-byte ds_read_b128,
// and S = 4 x odd puts the 16 lanes of each read quarter on distinct 4-bank groups (conflict
// free; the node-major layout before it read two masks per ds_read2_b32, at twice the LDS-array
// cycles per mask)
PBN_HD constexpr int sel_mask_stride(int B) { return 4 * (((3 * B + 3) / 4) | 1); }

// pbn_rollout_settle's ring of output rows (step_kernels.h "output rows in LDS")
PBN_HD constexpr int settle_stage_rows(int W) { return W == 1 ? 16 : (W == 2 ? 8 : 4); }
PBN_HD constexpr int settle_row_words(int W) { return 3 * 64 * W + 64 + 16 + 32; }
constexpr int kStageOutWords = 12;   // StageOut: six output pointers

// ---- LDS carving, in words; every kernel starts with the table image [tab_words] ----

// pbn_step_wave: image | S planes (+ gate planes) of each wave [kWavesPerBlock][wave_words]
constexpr int wave_plane_words(int W, int n_gates) { return (32 * W + n_gates + 3) & ~3; }
constexpr size_t wave_lds_words(int tab_words, int wave_words) {
  return (size_t)tab_words + (size_t)kWavesPerBlock * wave_words;
}

// the pipelined kernels: image | S planes of the block's two groups [64W] | 2 slots (by
// iteration parity).  pbn_rollout_pipe's slot: flip mask, perturbation mask, reset state [3W][64]
// | reset target [64] | selection planes [lq][64W]
PBN_HD constexpr int pipe_planes_words(int W) { return 2 * 32 * W; }
constexpr int pipe_slot_words(int W, int lq) { return (3 * W + 1) * 64 + lq * 64 * W; }
constexpr size_t pipe_lds_words(int tab_words, int W, int lq) {
  return (size_t)tab_words + (size_t)pipe_planes_words(W) + 2 * (size_t)pipe_slot_words(W, lq);
}

// pbn_rollout_settle's slot: flip mask, perturbation mask, reset state [3W][64] | reset target and
// action count [64] | selection planes [lq][64W]; after the slots: ctl [2][64] uint4 | the packed
// thresholds [lq][W][16] (rounded to 16 bytes) | the output rows | the stored-row counter by
// parity [2] | the rows' output pointers (StageOut), the two padded to 16 bytes
constexpr int settle_slot_words(int W, int lq) { return 192 * W + 64 + lq * 64 * W; }
constexpr int kSettleCtlVecs = 2 * 64;   // uint4
PBN_HD constexpr int settle_thr_words(int W, int lq) { return (lq * W * 16 + 3) & ~3; }
PBN_HD constexpr int settle_rows_words(int W) { return settle_stage_rows(W) * settle_row_words(W); }
constexpr int kSettleRowCounterWords = 2;
constexpr int settle_tail_words() { return (kSettleRowCounterWords + kStageOutWords + 3) & ~3; }
constexpr size_t settle_lds_words(int tab_words, int W, int lq) {
  return (size_t)tab_words + (size_t)pipe_planes_words(W) + 2 * (size_t)settle_slot_words(W, lq) +
         4 * (size_t)kSettleCtlVecs + (size_t)settle_thr_words(W, lq) + (size_t)settle_rows_words(W) +
         (size_t)settle_tail_words();
}
static_assert(settle_tail_words() == 16, "row counter [2] | StageOut [12] | padding [2]");

// ---- which kernel a launch runs ----

enum Kernel { kWave1, kWaveLean, kWaveSettle, kWaveSettleLean, kPipe, kPipeSettle, kNumKernels };

struct RouteNet {   // what routing needs to know of a net
  bool settle;            // the settle law (settle_max >= 2)
  int n_gates;            // lowered wide functions: the wave kernels only
  bool has_pipe_settle;   // pbn_rollout_settle has an instance for this net (max_nf <= kNodeRecs)
  int force_roll;         // PBN_ROLL: 0 none, 2 lean (wave kernel), 3 pipe
  size_t lds_wave, lds_pipe, lds_settle;   // bytes
};

struct Route {
  Kernel kernel;
  size_t lds_bytes;
  int threads;            // per block (the ride-along copy adds a fourth wave to kPipe)
  int groups_per_block;
};

inline size_t kernel_lds_bytes(const RouteNet& n, Kernel k) {
  return k == kPipe ? n.lds_pipe : (k == kPipeSettle ? n.lds_settle : n.lds_wave);
}

// pbn_step (rollout = false) runs the pipelined settle kernel on whole groups under the settle
// law, else a wave kernel; PBN_ROLL=lean forces the wave kernel, PBN_ROLL=pipe changes nothing.
// pbn_rollout runs a pipelined kernel where the net has one that fits kLdsPipeBytes; PBN_ROLL
// overrides that limit in both directions, but not the device's: a pipelined kernel that needs
// more than kLdsDeviceBytes cannot be launched at all (raise_lds_limits skips it), so a forced
// pipe takes the wave kernel there.  The host decides; no launch asks for more LDS than a CU has.
// Networks with gates always run a wave kernel.
inline Route route_launch(const RouteNet& n, bool rollout, bool whole_groups) {
  const bool can_pipe = !n.n_gates && (!n.settle || n.has_pipe_settle);
  bool pipe;
  if (rollout) {
    const size_t pipe_bytes = n.settle ? n.lds_settle : n.lds_pipe;
    pipe = can_pipe && pipe_bytes <= kLdsPipeBytes;
    if (n.force_roll) pipe = can_pipe && n.force_roll == 3 && pipe_bytes <= kLdsDeviceBytes;
  } else {
    pipe = n.settle && whole_groups && can_pipe && n.lds_settle <= kLdsPipeBytes && n.force_roll != 2;
  }
  if (pipe) {
    const Kernel k = n.settle ? kPipeSettle : kPipe;
    return {k, kernel_lds_bytes(n, k), 192, 2};
  }
  const Kernel k = rollout ? (n.settle ? kWaveSettleLean : kWaveLean) : (n.settle ? kWaveSettle : kWave1);
  return {k, n.lds_wave, 64 * kWavesPerBlock, kWavesPerBlock};
}

}  // namespace
