// step_args.h -- the argument structs of the step kernels: StepArgs (every kernel's launch
// arguments, filled by pbn_env.hip from the net image and the call) and PolicyArgs (the policy
// rollout's second argument).  Also what every piece of step_kernels.h starts from: the project
// headers the kernels build on and the names taken from namespace pbn.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/pbn_env.h"
#include "bitslice.h"
#include "dqn_forward.h"
#include "net_layout.h"
#include "philox.h"
#include "step_law.h"

using pbn::bfi, pbn::Word4;
using pbn::actions_from_draw, pbn::actions_mask31, pbn::ext64, pbn::valid_word_mask;   // (step_law.h)

namespace {

struct StepArgs {
  const uint32_t* tab;          // packed LDS image (cdf | reward | hash)
  const int32_t* att_start;     // [A+1]
  const uint32_t* att_states;   // [S*W]
  const uint32_t* state;
  uint32_t* flipmask;
  uint8_t* target;
  uint8_t* t;
  uint32_t* state_out;
  uint32_t* final_state;
  float* reward;
  uint8_t* flags;
  uint64_t seed, step, env_offset;
  const uint64_t* step_ptr;     // single-step kernel: step index read from device memory (nullable)
  int64_t n_envs;
  int64_t n_groups;
  int n_nodes;
  int n_attr;
  int horizon;
  int mode;
  int cdf_len;       // power of two >= N (LDS cdf table length, padded with 0xFFFFFFFF)
  int hash_bits;     // 0 = no attractors
  int hash_probes;   // max probe count (>= 1 when attractors exist)
  int tab_words;     // words of the LDS table image
  int prob_bits;
  int n_funcs;
  int wave_words;    // wave kernel: per-wave LDS words of S planes (after the shared table image)
  int gap_exact;     // 1: binary search for gaps (p == 0 or tiny); 0: log estimate + fix-up;
                     // 2: bucket table (gap_lut_off)
  int gap_lut_off;   // LDS image offset of the gap bucket table, uint2 [gap_nb + 1] {threshold, gap}
  int gap_shift;     // bucket of u = u >> gap_shift
  int gap_nb;        // buckets below C[N-1]; entry gap_nb is the sentinel {0xFFFFFFFF, N+1}
  float inv_log2q;   // 1 / log2(1 - p)
  const uint4* fcompact;   // [n_funcs] {inputs (4 x u8), truth table, threshold, 0}
  const uint4* nrec;       // [N * kNodeRecs] node-major copy of the first records (+ nf, f0 in .w)
  uint32_t hash_mult[4];
  unsigned long long* stamps;  // diagnostic builds (-DPBN_STAMPS) only: per-wave phase clocks
  int n_steps;       // steps per launch (wave kernel); outputs are [n_steps][...] arrays
  uint32_t* obs;     // [n_steps][W][n] observation before each step (nullable)
  int n_states;      // attractor states (bounds of att_states; checked builds)
  int att_off;       // LDS image offset of attractor start[A+1] | states[S][W] (wave kernel)
  int sel_off;       // LDS image offset of the leaf selectors, uint4 [kNodeRecs][2][32W] (wave kernel)
  int nrec_off;      // LDS image offset of the node records, record-major uint4 [kNodeRecs][32W]
  int cm_off;        // LDS image offset of pbn_rollout_pipe's threshold digit masks (W == 1),
                     // [32][sel_mask_stride(B)] lane-major
  int n_cls;         // 1..4: the first kNodeRecs thresholds of every node take one of n_cls values
                     // uthr[0..n_cls) (record .y = class index); 0: per-node thresholds
  uint32_t uthr[kNodeRecs];
  int max_nf;        // largest function count of a node
  int lq;            // pipelined rollout: selection masks per node in a slot (max(max_nf - 1, 1))
  int slot_words;    // pipelined rollout: words of one step slot
  int gate_off;      // wave kernel: LDS image offset of the gate records, uint4 [n_gates] by level
  int glayer_off;    // LDS image offset of the level starts, int32 [n_glayers + 1]
  int n_glayers;     // 0: no gates
  int att_single;    // every attractor is one state: the reset state is attractor a's state a
  uint32_t n1_magic; // ceil(2^32 / (N + 1)): random-action digits
  uint32_t am1_magic;  // ceil(2^32 / (A - 1)) for A >= 2: autoreset (start, target) split
  uint64_t x_mult;     // (N+1)^3 * A(A-1) (A >= 2) mod 2^64: what the ENV draws before gap 2 leave
                       // of X is X * x_mult (times the start attractor's size, multi-state nets)
  int sel_prio;        // pipelined rollout: raise the selection wave's priority (grids of at most
                       // four blocks per CU)
  int settle_max;      // step law: >= 2 = the settle law (wave kernel variants 3, 4,
                       // pbn_rollout_settle)
  uint16_t* updates;   // rollouts: [n_steps][n] synchronous updates applied per env-step (nullable)
  const uint32_t* sthr;  // settle law: thresholds scaled to 16 bits, [lq][32W] (65536 past a node's
                         // last function): the per-env selection compares (settle_lt_word)
  const uint32_t* sthr_pk;  // the same, node pairs packed biased for settle_lt_word_pk: [lq][W][16]
                            // {(C[2j+1] ^ 0x8000) << 16 | (C[2j] ^ 0x8000)}, C clamped to 65535
  int settle_pk;            // 1: every threshold a compare uses is below 65536 (sthr_pk is exact)
  // pbn_rollout_copy: cp_n16 16-byte vectors from cp_src to cp_dst ride along the launch (the
  // pipelined kernel's fourth wave, ride_copy_wave); 0: none.  cp_u: vectors per lane and step
  // iteration (paced: the block's share in n_steps + 1 portions, one per block barrier); 0: the
  // share in one burst
  const void* cp_src;
  void* cp_dst;
  int64_t cp_n16;
  int cp_u;
  // pbn_step_dev_store (ABI 11): the one-update wave kernel also writes the step's transitions into
  // a replay ring (pbn_replay_store's layout), env le at row (*r_pos + le) mod r_cap; r_state null:
  // none
  uint32_t* r_state;
  uint32_t* r_next;
  uint8_t* r_target;
  int32_t* r_action;
  float* r_reward;
  uint8_t* r_done;
  const int32_t* r_act_in;   // [n][r_k] the frame's branch actions
  uint8_t* r_done_out;       // nullable: [n]
  const int64_t* r_pos;
  int64_t r_cap;
  int r_k;
  uint32_t r_done_mask;
};

// The policy of a policy rollout (pbn_step_wave<W, B, 2 | 4, PolicyArgs>'s second argument): a DQN whose image
// (pbn_dqn_pack) the wave reads every step, acting epsilon-greedily under the EXPLORE law
struct PolicyArgs {
  Dims d;
  const float* img;
  uint64_t eps_u;     // explore_threshold(epsilon)
  int32_t* actions;   // [n_steps][n] the actions taken (nullable)
};

constexpr int kRingMaxK = 8;   // pbn_step_dev_store: branch actions per env (BDQ: K + 1 <= kMaxHeads)

}  // namespace
