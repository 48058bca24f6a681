// net_layout.h -- what the host-side descriptor compiler (net_image.h), the launcher
// (pbn_env.hip) and the kernels (step_wave.h, rollout_pipe.h, rollout_settle.h) must agree on:
// table strides, the LDS carving of the three step kernels, the LDS limits and the choice of
// kernel for a launch.  Each carving is stated once, as offsets: the host's LDS request is the
// last offset, the kernels take their pointers from the same functions, and carving_ok (at the
// end of the carving) asserts order, alignment and totals.  Plain C++17, free of HIP.
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

// pbn_rollout_settle's ring of output rows (rollout_settle.h "output rows in LDS"): R rows of the
// block's 64 envs, a row's fields at these word offsets: final state [W][64] | observation
// [W][64] | flip mask [W][64] | reward [64] | flags [64 bytes] | update counts [64 u16]
PBN_HD constexpr int settle_stage_rows(int W) { return W == 1 ? 16 : (W == 2 ? 8 : 4); }
PBN_HD constexpr int settle_row_final(int) { return 0; }
PBN_HD constexpr int settle_row_obs(int W) { return settle_row_final(W) + 64 * W; }
PBN_HD constexpr int settle_row_flip(int W) { return settle_row_obs(W) + 64 * W; }
PBN_HD constexpr int settle_row_reward(int W) { return settle_row_flip(W) + 64 * W; }
PBN_HD constexpr int settle_row_flags(int W) { return settle_row_reward(W) + 64; }
PBN_HD constexpr int settle_row_updates(int W) { return settle_row_flags(W) + 64 / 4; }
PBN_HD constexpr int settle_row_words(int W) { return settle_row_updates(W) + 64 / 2; }
constexpr int kStageOutWords = 12;   // StageOut: six output pointers

// ---- LDS carving, in words; every kernel starts with the table image [tab_words] ----

// pbn_step_wave: image | S planes (+ gate planes) of each wave [kWavesPerBlock][wave_words]
constexpr int wave_plane_words(int W, int n_gates) { return (32 * W + n_gates + 3) & ~3; }
constexpr size_t wave_lds_words(int tab_words, int wave_words) {
  return (size_t)tab_words + (size_t)kWavesPerBlock * wave_words;
}

// the pipelined kernels: image | S planes of the block's two groups [64W] | 2 slots (by
// iteration parity).  A slot is env-major, [64] words per field and state word, and its fields are
// the same in both kernels: flip mask [W][64] | perturbation mask [W][64] | reset state [W][64] |
// info [64] (pbn_rollout_pipe: reset target, action count, perturbed; pbn_rollout_settle: reset
// target, action count) | selection planes [lq][64W]
PBN_HD constexpr int pipe_planes_words(int W) { return 2 * 32 * W; }
PBN_HD constexpr int pipe_slot_flip(int) { return 0; }
PBN_HD constexpr int pipe_slot_pert(int W) { return pipe_slot_flip(W) + 64 * W; }
PBN_HD constexpr int pipe_slot_reset(int W) { return pipe_slot_pert(W) + 64 * W; }
PBN_HD constexpr int pipe_slot_info(int W) { return pipe_slot_reset(W) + 64 * W; }
PBN_HD constexpr int pipe_slot_sel(int W) { return pipe_slot_info(W) + 64; }
PBN_HD constexpr int pipe_slot_words(int W, int lq) { return pipe_slot_sel(W) + lq * 64 * W; }
PBN_HD constexpr int settle_slot_words(int W, int lq) { return pipe_slot_words(W, lq); }   // (the same slot)
constexpr size_t pipe_lds_words(int tab_words, int W, int lq) {
  return (size_t)tab_words + (size_t)pipe_planes_words(W) + 2 * (size_t)pipe_slot_words(W, lq);
}

// pbn_rollout_settle, after the slots (word offsets from their end): ctl [2][64] uint4 | the
// packed thresholds [lq][W][16] (rounded to 16 bytes) | the output rows | the stored-row counter
// by parity [2] | the rows' output pointers (StageOut, uint64_t) | end, the two padded to 16 bytes
constexpr int kSettleCtlVecs = 2 * 64;   // uint4
PBN_HD constexpr int settle_thr_words(int W, int lq) { return (lq * W * 16 + 3) & ~3; }
PBN_HD constexpr int settle_rows_words(int W) { return settle_stage_rows(W) * settle_row_words(W); }
constexpr int kSettleRowCounterWords = 2;
struct SettleTail {   // (functions: a kernel pays for the lq arithmetic only where it asks for it)
  int W, lq;
  PBN_HD constexpr int ctl() const { return 0; }
  PBN_HD constexpr int thr() const { return ctl() + 4 * kSettleCtlVecs; }
  PBN_HD constexpr int rows() const { return thr() + settle_thr_words(W, lq); }
  PBN_HD constexpr int counter() const { return rows() + settle_rows_words(W); }
  PBN_HD constexpr int out() const { return counter() + kSettleRowCounterWords; }
  PBN_HD constexpr int end() const { return (out() + kStageOutWords + 3) & ~3; }
};
constexpr size_t settle_lds_words(int tab_words, int W, int lq) {
  return (size_t)tab_words + (size_t)pipe_planes_words(W) + 2 * (size_t)settle_slot_words(W, lq) +
         (size_t)SettleTail{W, lq}.end();
}

// The carvings above, checked for W state words and lq selection masks against each region's
// width, written out once more below: the regions lie in order and do not overlap, what is read as
// uint4 (ctl, the packed thresholds, a slot's rows through ds_read_b128; the table image is a
// multiple of 16 bytes) or as uint64_t (StageOut) is aligned, and the LDS a launch asks for ends
// where the last region ends.  (It catches an offset that no longer leaves room for its
// neighbour, not a width changed here and above alike.)
struct LdsRegion {
  int at, words;
};
template <int N>
constexpr bool lds_in_order(const LdsRegion (&r)[N], int end) {
  for (int i = 0; i < N; ++i)
    if (r[i].at < 0 || r[i].words < 0 || r[i].at + r[i].words > (i + 1 < N ? r[i + 1].at : end)) return false;
  return r[0].at == 0;
}
constexpr bool carving_ok(int W, int lq) {
  const LdsRegion slot[] = {{pipe_slot_flip(W), 64 * W}, {pipe_slot_pert(W), 64 * W}, {pipe_slot_reset(W), 64 * W},
                            {pipe_slot_info(W), 64}, {pipe_slot_sel(W), lq * 64 * W}};
  const LdsRegion row[] = {{settle_row_final(W), 64 * W}, {settle_row_obs(W), 64 * W}, {settle_row_flip(W), 64 * W},
                        {settle_row_reward(W), 64}, {settle_row_flags(W), 64 / 4}, {settle_row_updates(W), 64 / 2}};
  const SettleTail t = {W, lq};
  const LdsRegion tail[] = {{t.ctl(), 4 * kSettleCtlVecs}, {t.thr(), lq * W * 16}, {t.rows(), settle_rows_words(W)},
                         {t.counter(), kSettleRowCounterWords}, {t.out(), kStageOutWords}};
  const int front = pipe_planes_words(W) + 2 * pipe_slot_words(W, lq);   // after the image, before the tail
  return lds_in_order(slot, pipe_slot_words(W, lq)) && lds_in_order(slot, settle_slot_words(W, lq)) &&
         lds_in_order(row, settle_row_words(W)) && lds_in_order(tail, t.end()) &&
         pipe_slot_words(W, lq) % 4 == 0 && settle_row_words(W) % 4 == 0 && front % 4 == 0 && t.ctl() % 4 == 0 &&
         t.thr() % 4 == 0 && t.rows() % 4 == 0 && (front + t.out()) % 2 == 0 && t.end() % 4 == 0 &&
         pipe_lds_words(0, W, lq) == (size_t)front && settle_lds_words(0, W, lq) == (size_t)(front + t.end());
}
constexpr bool carvings_ok() {
  for (int W = 1; W <= 4; ++W)
    for (int lq = 1; lq <= 3; ++lq)
      if (!carving_ok(W, lq)) return false;
  return true;
}
static_assert(carvings_ok(), "the pipelined kernels' LDS carvings, W = 1..4, lq = 1..3");
static_assert(SettleTail{1, 1}.end() - SettleTail{1, 1}.counter() == 16, "row counter [2] | StageOut [12] | padding [2]");

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
