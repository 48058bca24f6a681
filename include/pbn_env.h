/*
 * pbn_env.h -- C-ABI of the MI355X batched PBN environment step (libpbn_env.so).
 *
 * This is the drop-in boundary for the gym-PBN state-transition hot path that
 * jakub-zarzycki2022/pbn-rl drives.  The reference binds no native code: it
 * calls the external Python package gym_PBN (requirements.txt:11,
 * gym-PBN[vis]==1.1.1 + an unpublished fork) through gymnasium:
 *
 *   gym.make("gym-PBN/PBNEnv", N=, genes=, logic_functions=[, min_attractors=])
 *        train_assa_BQN.py:121-124, model_tester.py:409-413     -> pbn_net_create
 *   env.reset() -> ((state, target), info)
 *        bdq_model/__init__.py:161,204                         -> pbn_reset
 *   env.step(actions) -> (obs, reward, terminated, truncated, info)
 *        bdq_model/__init__.py:177, graph_classifier/__init__.py:148,
 *        model_tester.py:561,624, ddqn_per/__init__.py:354     -> pbn_step
 *   env.close()  train_BDQ.py:116                              -> pbn_net_destroy
 *   T frames of the frame loop bdq_model/__init__.py:172-213     -> pbn_rollout
 *   compute_ssd_hist(env, model, resets, iters) train_pbn_28.py:257 -> pbn_rollout + pbn_state_histogram
 *   BranchingDQN.predict + list(action.unique())
 *        bdq_model/__init__.py:69-98,176                       -> pbn_bilinear_targets (first layer),
 *                                                                 pbn_qnet_heads (the other layers),
 *                                                                 pbn_heads_to_flipmask / pbn_q_to_flipmask,
 *                                                                 or pbn_qnet_flipmask (both in one)
 *   update_policy's np.stack of sampled Transitions
 *        bdq_model/__init__.py:100-109                         -> pbn_obs_unpack, pbn_replay_batch
 *   update_policy (forwards, TD loss, backward, clamp, Adam)
 *        bdq_model/__init__.py:100-139                         -> pbn_bdq_learn (+ pbn_bdq_layout,
 *                                                                 pbn_bdq_pack, pbn_replay_store,
 *                                                                 pbn_replay_advance)
 *   ControlGBDQ.predict (one binary value per control node)
 *        control_gbdq_model/__init__.py:64-86                  -> pbn_gbdq_front, pbn_cgbdq_flipmask
 *   a frame loop captured once and replayed (no reference counterpart)
 *                                                              -> pbn_step_dev, pbn_q_to_flipmask_dev
 *   the hand-off of a rollout's transitions to the learner (north_star's per-rollout gather;
 *   at world 1 the learner's own shard into its receive slot)  -> pbn_copy_async
 *
 * The Python facade (pbn_rl_amd.env.PBNEnv / pbn_rl_amd.vector_env.VectorPBNEnv)
 * keeps that gym surface and calls these entry points through ctypes;
 * INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every entry point returns 0 or a negative PBN_E* code; pbn_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - the caller owns every device buffer (plain device pointers, e.g. from
 *     torch tensors); a pbn_net owns only its device-resident tables;
 *   - calls are asynchronous on the caller's HIP stream (hipStream_t passed as
 *     void*; NULL = the default stream); no entry point synchronises, allocates
 *     or frees inside pbn_reset/pbn_step, so both can be captured in a hipGraph;
 *   - a pbn_net is bound to the device that was current at create time and is
 *     not thread-safe: use one per GPU / process;
 *   - envs are processed in groups of 32 consecutive envs (bit-sliced layout):
 *     n_envs and env_offset must be multiples of 32, except that pbn_reset and
 *     pbn_step take any n_envs (ABI 9: the last group is partial; its missing
 *     envs are neither read nor written, and the others' results do not depend on
 *     them: the scalar gym facade steps n_envs = 1).  Randomness depends only
 *     on (seed, global env id = env_offset + local id, step), so sharding envs
 *     across GPUs gives bit-identical results.
 *
 * Device data layout for n envs with W = ceil(n_nodes / 32) state words:
 *   state, flipmask          uint32 [W][n]   (SoA word planes; bit i of word w = node 32w+i)
 *   target                   uint8  [n]      (attractor id; 0xFF = none)
 *   t                        uint8  [n]      (steps taken in the current episode)
 *   reward                   float  [n]
 *   flags                    uint8  [n]      (PBN_FLAG_* bits)
 *
 * Step semantics: DESIGN.md "Step semantics" (frozen; gym_PBN is unavailable).
 */
#ifndef PBN_ENV_H
#define PBN_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBN_ABI_VERSION 11

#define PBN_MAX_NODES 128
#define PBN_MAX_ARITY 4
#define PBN_MAX_FUNCS_PER_NODE 16
#define PBN_MAX_ATTRACTORS 254
#define PBN_MAX_GATES 224          /* and 32 * ceil(n_nodes / 32) + n_gates <= 256 */
#define PBN_MAX_SETTLE 4096        /* cap of settle_max (synchronous updates per env step) */
#define PBN_NO_TARGET 0xFF

/* error codes */
#define PBN_OK 0
#define PBN_EINVAL (-22)
#define PBN_ENOMEM (-12)
#define PBN_EDEVICE (-5)

/* pbn_step mode bits */
#define PBN_MODE_AUTORESET 1u      /* done envs restart: state_out/target/t hold the new episode */
#define PBN_MODE_RANDOM_ACTIONS 2u /* actions drawn in-kernel (3 uniform ints in [0,N], 0 = no-op,
                                      bdq_model/__init__.py:76); flipmask is an OUTPUT */

/* flags bits */
#define PBN_FLAG_TERMINATED 1u     /* s' is a state of the env's target attractor */
#define PBN_FLAG_TRUNCATED 2u      /* t' == horizon */
#define PBN_FLAG_IN_ATTRACTOR 4u   /* s' is a state of some attractor */
#define PBN_FLAG_PERTURBED 8u      /* a perturbation fired this step */
#define PBN_FLAG_RESET 16u         /* autoreset happened: state_out is a fresh start */
#define PBN_FLAG_UNSETTLED 32u     /* settle law: settle_max updates ran and s' is in no attractor */

/*
 * Network description (semantic form; the library derives its kernel encodings).
 * Function f of node i (node_func_start[i] <= f < node_func_start[i+1]) has
 * func_arity[f] <= 4 inputs func_inputs[4f..4f+arity) (plane references, below) and truth
 * table func_table[f]: bit m = value when input j = bit j of m.
 * func_threshold[f] is the cumulative selection threshold c_f in units of
 * 2^-prob_bits (strictly: c_{f-1} <= c_f, last of a node == 2^prob_bits).
 * perturb_cdf[m-1] = floor(2^32 * (1 - (1-p)^m)), m = 1..n_nodes.
 * Attractor a owns states attractor_start[a] .. attractor_start[a+1]-1; state k
 * is words attractor_states[k*W .. k*W+W).  reward_table[(2*term + wrong)*(N+1) + k]
 * with k = popcount(flipmask), wrong = in some non-target attractor.
 *
 * Step law (settle_max).  0 or 1: one synchronous update per env step (DESIGN.md "Step
 * semantics").  K >= 2, the settle law: after the intervention the network keeps updating
 * synchronously until the state is a state of some attractor, at most K updates in all;
 * flags carry PBN_FLAG_UNSETTLED when the K-th update still left it outside every attractor.
 * That is the "intervene, then run to a (pseudo-)attractor" step that the reference's
 * recorded bb33 evaluation pins (data/results/pbn_33_3.pkl under model_tester.py:587-658;
 * DESIGN.md "Parity status").  Update 0 draws its actions, autoreset and perturbation from the
 * one-update law's ENV / PERT calls, updates k >= 1 their perturbation from SETTLE_ENV; every
 * update's rule selection (k >= 0) is keyed per env (ABI 7): node i's uniform is the top
 * prob_bits bits of 16-bit field i & 1 of word (i >> 1) & 3 of SETTLE_SEL call (k << 8 | i >> 3)
 * of (env, step) -- so every env runs its own sequence of updates (DESIGN.md "Step law").
 */
typedef struct pbn_net_desc {
  int32_t n_nodes;
  int32_t n_funcs;
  int32_t prob_bits;     /* 4, 8, 12 or 16 */
  int32_t horizon;       /* 0 = no truncation, else 1..255 */
  const int32_t* node_func_start;   /* [n_nodes + 1] */
  const int32_t* func_arity;        /* [n_funcs] */
  const int32_t* func_inputs;       /* [n_funcs * 4], unused slots -1 */
  const uint32_t* func_table;       /* [n_funcs] */
  const uint32_t* func_threshold;   /* [n_funcs] */
  const uint32_t* perturb_cdf;      /* [n_nodes] */
  int32_t n_attractors;             /* 0..254 */
  int32_t n_attractor_states;
  const int32_t* attractor_start;   /* [n_attractors + 1] */
  const uint32_t* attractor_states; /* [n_attractor_states * W] */
  const float* reward_table;        /* [4 * (n_nodes + 1)] */
  /* Combinational gates: functions of more than 4 inputs, lowered by the compiler
   * (pbn_rl_amd/lowering.py) into functions of at most 4 "planes".  A plane reference
   * r < n_nodes is node r of the pre-step state s1; r >= n_nodes is gate r - n_nodes.  Gate g
   * may read nodes and gates < g; func_inputs may hold any reference.  All gates are evaluated
   * on s1, like the node functions, so the update stays synchronous.  0 gates = none. */
  int32_t n_gates;
  const int32_t* gate_arity;        /* [n_gates] 0..4 */
  const int32_t* gate_inputs;       /* [n_gates * 4], unused slots -1 */
  const uint32_t* gate_table;       /* [n_gates] */
  int32_t settle_max;               /* 0..PBN_MAX_SETTLE, see "Step law" above (ABI 3) */
} pbn_net_desc;

typedef struct pbn_net pbn_net;

/* Compile + upload the tables to the current device. */
int pbn_net_create(const pbn_net_desc* desc, pbn_net** out);
int pbn_net_destroy(pbn_net* net);
/* W = state words per env. */
int pbn_net_words(const pbn_net* net);

/*
 * Start episodes for envs [env_offset, env_offset + n_envs): state uniform over
 * the states of a uniformly drawn attractor, target a different attractor
 * (or a uniform random state and PBN_NO_TARGET when there are no attractors),
 * t = 0.  Draws are keyed by (seed, global env id, step).
 */
int pbn_reset(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
              uint32_t* d_state, uint8_t* d_target, uint8_t* d_t, void* stream);

/*
 * One env step of every env (the hot path): one synchronous PBN transition, or under the
 * settle law (settle_max >= 2) the intervention followed by updates until an attractor.
 *   d_state        in   [W][n]  current observation s
 *   d_flipmask     in   [W][n]  intervention flips (bit a-1 for action a > 0);
 *                  out  with PBN_MODE_RANDOM_ACTIONS (the actions drawn)
 *   d_target       in/out [n]   rewritten only for envs that autoreset
 *   d_t            in/out [n]
 *   d_state_out    out  [W][n]  next observation (reset state for autoreset envs)
 *   d_final_state  out  [W][n]  s' (the transition result) -- may be NULL
 *   d_reward, d_flags  out [n]
 * d_state_out must not alias d_state.
 */
int pbn_step(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
             uint32_t mode, const uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
             uint8_t* d_t, uint32_t* d_state_out, uint32_t* d_final_state, float* d_reward,
             uint8_t* d_flags, void* stream);

/*
 * pbn_step with the step index read from device memory (*d_step, 8-byte aligned) when the
 * kernel runs instead of passed by value, so one captured hipGraph of a frame (act + step +
 * replay + update) can be replayed for successive steps: the caller advances *d_step on the
 * stream (e.g. a captured add).  Results are bit-identical to pbn_step(step = *d_step).
 */
int pbn_step_dev(pbn_net* net, uint64_t seed, const uint64_t* d_step, uint64_t env_offset, int64_t n_envs,
                 uint32_t mode, const uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                 uint8_t* d_t, uint32_t* d_state_out, uint32_t* d_final_state, float* d_reward,
                 uint8_t* d_flags, void* stream);

/*
 * pbn_step_dev_store (ABI 11): pbn_step_dev that also writes the step's transitions into a replay
 * ring, the layout pbn_replay_store writes (replaces the learning frame's separate ring-store
 * launch, pbn_rl_amd/replay.py BDQLearner's captured frame).  One-update law only (settle_max < 2;
 * PBN_EINVAL otherwise).  d_state is updated in place.  Env e's row is (*d_pos + e) mod capacity
 * (d_pos read when the kernel runs; not advanced): state = s as the step read it (bits past N
 * cleared), next_state = s' before an autoreset (= d_final_state), target = the target before
 * the step, action = d_actions_in's n_branches int32 of env e, reward, done = (flags & done_mask)
 * != 0 (done_mask 0: flags != 0), also into d_done_out[e] when not null.
 */
typedef struct pbn_ring_store {
  int64_t capacity;            /* >= n_envs */
  const int64_t* d_pos;
  uint32_t* d_state;           /* [W][capacity] */
  uint32_t* d_next_state;      /* [W][capacity] */
  uint8_t* d_target;           /* [capacity] */
  int32_t* d_action;           /* [capacity][n_branches] */
  float* d_reward;             /* [capacity] */
  uint8_t* d_done;             /* [capacity] */
  const int32_t* d_actions_in; /* [n_envs][n_branches] */
  int32_t n_branches;          /* 1..8 */
  uint32_t done_mask;
  uint8_t* d_done_out;         /* nullable: [n_envs] */
} pbn_ring_store;

int pbn_step_dev_store(pbn_net* net, uint64_t seed, const uint64_t* d_step, uint64_t env_offset, int64_t n_envs,
                       uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target, uint8_t* d_t,
                       uint32_t* d_final_state, float* d_reward, uint8_t* d_flags, const pbn_ring_store* ring,
                       void* stream);

/*
 * n_steps synchronous transitions in one launch (steps step .. step+n_steps-1), with the
 * envs' state kept on chip between steps.  Bit-identical to n_steps successive pbn_step
 * calls that ping-pong d_state.  State, target and t are updated in place.
 *   d_flipmask     [n_steps][W][n]  in, or out with PBN_MODE_RANDOM_ACTIONS
 *   d_obs          [n_steps][W][n]  out: observation before each step (nullable)
 *   d_final_state  [n_steps][W][n]  out: s' of each step (nullable)
 *   d_reward, d_flags  [n_steps][n] out
 */
int pbn_rollout(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                void* stream);

/*
 * pbn_rollout with one more output (ABI 4):
 *   d_updates  [n_steps][n] uint16 out (nullable): the synchronous updates applied in each
 *              env-step, 1 under the one-update law, 1..settle_max under the settle law (the
 *              settle length; the env-step carries PBN_FLAG_UNSETTLED when it reached settle_max
 *              outside every attractor).
 * Under the settle law the pipelined kernel runs one update per iteration for every env on its
 * own plan (the selection keyed per env): an env starts its next step as soon as its current
 * step ends, whatever the other envs of its 32-env word do.
 *   the frame loop bdq_model/__init__.py:172-213 on the env constructed at train_BDQ.py:50 /
 *   model_tester.py:409-413, whose step runs to an attractor (model_tester.py:616-626)
 */
int pbn_rollout_ex(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                   int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                   uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                   uint16_t* d_updates, void* stream);

/*
 * pbn_rollout_ex with a copy riding along (ABI 8): the launch also copies copy_bytes from
 * d_copy_src to d_copy_dst (16-byte aligned, non-overlapping, neither one of this launch's
 * buffers).  The copy is complete when the launch is, on the same stream.  The pipelined
 * one-update kernel runs with a fourth wave per block that moves the block's share of the copy,
 * paced by the block's step barriers (up to four 16-byte vectors per lane and step, else in one
 * burst), and exits; the settle kernel and the wave kernel get pbn_copy_async right after the
 * launch, as does a launch of no steps.  The world-1 hand-off uses it to move rollout k's records into the learner's
 * receive slot during rollout k + 1 (pbn_rl_amd/distributed.py ShardedRollout.gather): the
 * receive half of the gather's point-to-point exchange, for the learner's own shard.
 */
int pbn_rollout_copy(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                     int32_t n_steps, uint32_t mode, uint32_t* d_state, uint32_t* d_flipmask, uint8_t* d_target,
                     uint8_t* d_t, uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                     uint16_t* d_updates, void* d_copy_dst, const void* d_copy_src, int64_t copy_bytes,
                     void* stream);

/*
 * State histogram, the accumulation step of the steady-state distribution
 * (gym_PBN.utils.eval.compute_ssd_hist, train_pbn_28.py:257, train_pbn_10.py:257):
 * d_hist[d_states[r * row_stride + c] & (2^n_bits - 1)] += 1 for r < n_rows, c < n_cols.
 * Uses word 0 of each state (networks with n_nodes <= 32: pass the [steps][1][n] obs or
 * final_state output of pbn_rollout with row_stride = n).  1 <= n_bits <= 32; 32-bit counters;
 * the caller zeroes d_hist (2^n_bits entries).
 */
int pbn_state_histogram(const uint32_t* d_states, int64_t n_rows, int64_t n_cols, int64_t row_stride,
                        int32_t n_bits, uint32_t* d_hist, void* stream);

/*
 * Visited-state count in a device hash table keyed by the full state (additive export of ABI 11;
 * pbn_rl_amd/csrc/state_table.h states the table, the hash and the probe): the sparse form of
 * pbn_state_histogram for networks of any width, with 64-bit counts.
 *
 * Input: element (row t, word w, column c) of d_states at t * n_words * col_stride +
 * w * col_stride + c, c < n_cols <= col_stride -- the [steps][W][n] obs / final_state output of
 * the rollouts with col_stride = n; columns past n_cols are not counted.  The key is the row's
 * n_words words, the top one masked to n_bits (32 (n_words - 1) + 1 .. 32 n_words).  Flattened
 * row t * n_cols + c adds d_row_counts[t * n_cols + c] visits (0 skips the row), or one where
 * d_row_counts is null; n_rows * n_cols < 2^32 - 1.
 *
 * Table: capacity a power of two >= 64; d_owner u64 [capacity] (0 = empty, else epoch << 32 |
 * claiming row + 1), d_keys u32 [n_words][capacity], d_counts u64 [capacity], d_used / d_lost
 * u64 [1] (slots claimed; rows that found no slot).  The caller zeroes all five once, passes an
 * epoch >= 1 that is larger in every later launch on the same table, and keeps used + rows of the
 * launch <= capacity / 2, so that a probe always meets an empty slot and d_lost stays 0.
 * Rehashing or merging a table is the same call over that table's d_keys (n_rows 1, n_cols =
 * col_stride = its capacity) with its d_counts as d_row_counts.
 *
 * Asynchronous on `stream`; allocates and synchronises nothing.  An empty input returns PBN_OK
 * without a launch; argument errors return PBN_EINVAL before any device call.
 */
int pbn_table_insert(const uint32_t* d_states, int64_t n_rows, int64_t n_cols, int64_t col_stride,
                     int32_t n_words, int32_t n_bits, const uint64_t* d_row_counts, int64_t capacity,
                     uint64_t* d_owner, uint32_t* d_keys, uint64_t* d_counts, uint64_t* d_used,
                     uint64_t* d_lost, uint32_t epoch, void* stream);

/*
 * Agent edges of the batched BDQ frame loop (bdq_model/__init__.py:69-98,172-177;
 * SURVEY.md 8(d) config 5).  The Q-network forward itself runs in PyTorch between them.
 *
 * pbn_obs_unpack replaces the host np.stack((state, target)) -> float tensor of
 * BranchingDQN.predict (bdq_model/__init__.py:92-93) for a whole batch:
 *   d_obs  out  float [2][n][N]: [0][e][i] = bit i of env e's state, [1][e][i] = bit i of
 *               the first state of env e's target attractor (0 without a target)
 *               -- the (2, B, N) input of BranchingQNetwork (bdq_model/network.py:55-57).
 * n_envs multiple of 32, n_envs * n_nodes < 2^31, d_obs 16-byte aligned.
 */
int pbn_obs_unpack(const pbn_net* net, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                   float* d_obs, void* stream);

/*
 * The bilinear first layer of BranchingQNetwork (bdq_model/network.py:8-21) for the
 * observation pbn_obs_unpack would build, straight from the packed state:
 *   d_y[e][o] = d_bias[o] + sum over the set bits i of env e's state of d_T[target_e][i][o]
 *   d_T     in   float [n_attr][n_nodes][out_dim]: T[a][i][o] = sum_j t_a[j] W[o][i][j], t_a the
 *                first state of attractor a (the caller's GEMM; W = the layer's weight)
 *   d_bias  in   float [out_dim];  d_y out float [n][out_dim]
 * Envs without a target (id >= n_attr) get the bias.  n_envs multiple of 32, out_dim a
 * multiple of 4 in 4..1024, d_T / d_bias / d_y 16-byte aligned.
 * Rows are added in ascending i (fp32; not bit-identical to a GEMM's order).  leaky != 0 applies
 * the network's LeakyReLU (x > 0 ? x : x * slope) before the store.
 */
int pbn_bilinear_targets(const pbn_net* net, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                         const float* d_T, const float* d_bias, int32_t out_dim, int32_t leaky, float slope,
                         float* d_y, void* stream);

/*
 * pbn_q_to_flipmask replaces epsilon-greedy predict + list(action.unique()) + the env's
 * action decoding (bdq_model/__init__.py:69-98,176; action a > 0 flips node a-1, :81-84):
 *   d_q         in   float [n][n_branches][n_actions], n_actions == n_nodes + 1, 16-byte aligned
 *   epsilon     explore with probability epsilon: env e explores iff EXPLORE word 0 <
 *               floor(epsilon * 2^32); its branch k action is then
 *               (word (k + 1) * (N+1)) >> 32, words numbered across EXPLORE calls 0, 1
 *               (uniform over [0, N] to (N+1)/2^32, as np.random.randint at :76);
 *               otherwise argmax over the branch (first
 *               maximum, NaN counts as the maximum: torch.argmax at :96).  EXPLORE = Philox
 *               stream 4 keyed by (seed, global env id, step), as in DESIGN.md.
 *   d_flipmask  out  uint32 [W][n]: bit a-1 set for every distinct action a > 0
 *   d_actions   out  int32 [n][n_branches] (nullable): the chosen actions
 * n_branches 1..7.  n_envs and env_offset multiples of 32.
 */
int pbn_q_to_flipmask(const pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                      int32_t n_branches, int32_t n_actions, const float* d_q, float epsilon,
                      uint32_t* d_flipmask, int32_t* d_actions, void* stream);

/*
 * pbn_q_to_flipmask with the step index read from device memory, as pbn_step_dev, and
 * epsilon read from *d_epsilon when that is not NULL (clamped to [0, 1], NaN -> 0), so an
 * epsilon schedule can advance on the device between graph replays.
 */
int pbn_q_to_flipmask_dev(const pbn_net* net, uint64_t seed, const uint64_t* d_step, uint64_t env_offset,
                          int64_t n_envs, int32_t n_branches, int32_t n_actions, const float* d_q,
                          float epsilon, const float* d_epsilon, uint32_t* d_flipmask, int32_t* d_actions,
                          void* stream);

/*
 * pbn_q_to_flipmask on the raw head outputs of BranchingQNetwork instead of Q:
 *   d_heads  in  float [n_branches + 1][n][n_actions], head 0 = the value head (output 0 used),
 *                heads 1.. = the advantage heads (bdq_model/network.py:55-61)
 * The dueling combination is done in the kernel: q_a = (v + adv_a) - mean with mean the
 * sequential sum of adv over a divided by n_actions, then as pbn_q_to_flipmask.  d_step and
 * d_epsilon are optional device pointers (NULL: use step / epsilon), as in the _dev forms.
 */
int pbn_heads_to_flipmask(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step,
                          uint64_t env_offset, int64_t n_envs, int32_t n_branches, int32_t n_actions,
                          const float* d_heads, float epsilon, const float* d_epsilon, uint32_t* d_flipmask,
                          int32_t* d_actions, void* stream);

/*
 * The layers of BranchingQNetwork after the bilinear one (bdq_model/network.py:35-61), fused
 * into one MFMA kernel (v_mfma_f32_32x32x2_f32, exact f32 k-ordered fmaf chains):
 *   d_y     in   float [n][256]: the bilinear layer after its LeakyReLU (pbn_bilinear_targets
 *                with leaky != 0)
 *   d_w1 [128][256], d_b1 [128]; d_w2 [64][128], d_b2 [64]; d_w3 [32][64], d_b3 [32]: the trunk
 *                Linear layers (torch's (out, in) layout), each followed by LeakyReLU(slope)
 *   d_wh1 [64 H][32], d_bh1 [64 H]: the H = n_heads first head layers stacked (value head
 *                first), each followed by LeakyReLU; d_wh2 [H][A][64], d_bh2 [H][A]: the
 *                second head layers (the value head zero-padded to A outputs)
 *   d_heads out  float [H][n][A]: the raw head outputs pbn_heads_to_flipmask consumes
 * n_envs a multiple of 32; n_heads 1..8; n_actions (A) 1..128; d_y and the weight matrices
 * 16-byte aligned.  Summation order differs from a GEMM library's: compare with a tolerance.
 */
int pbn_qnet_heads(const pbn_net* net, int64_t n_envs, const float* d_y, const float* d_w1, const float* d_b1,
                   const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3, const float* d_wh1,
                   const float* d_bh1, const float* d_wh2, const float* d_bh2, int32_t n_heads, int32_t n_actions,
                   float slope, float* d_heads, void* stream);

/*
 * pbn_qnet_heads and pbn_heads_to_flipmask in one launch: the same layers, then, per env, the
 * dueling combination, epsilon-greedy and flip masks exactly as pbn_heads_to_flipmask computes
 * them (same q_a order, same EXPLORE draws), without the (K+1, n, A) head outputs in HBM.
 * Arguments as those two functions (n_branches = K, the heads are K + 1; n_actions = N + 1);
 * d_step / d_epsilon, when non-null, are read when the kernel runs (graph replays).
 *   bdq_model/__init__.py:69-98,176 (predict + list(action.unique())) after the bilinear layer
 */
int pbn_qnet_flipmask(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step, uint64_t env_offset,
                      int64_t n_envs, const float* d_y, const float* d_w1, const float* d_b1, const float* d_w2,
                      const float* d_b2, const float* d_w3, const float* d_b3, const float* d_wh1, const float* d_bh1,
                      const float* d_wh2, const float* d_bh2, int32_t n_branches, int32_t n_actions, float slope,
                      float epsilon, const float* d_epsilon, uint32_t* d_flipmask, int32_t* d_actions,
                      void* stream);

/*
 * pbn_qnet_heads / pbn_qnet_flipmask with the bilinear layer (+ LeakyReLU) computed in the same
 * launch from the packed state, in place of d_y: the arguments of pbn_bilinear_targets (d_state,
 * d_target, d_T, d_b0 = the layer's bias [256], out_dim 256) followed by those of the function
 * it extends.  d_T here is pbn_bilinear_targets' table with every 256-output row stored as 16 x 16
 * transposed (ABI 5): float [n_attr][n_nodes][16][16], element [a][i][j][q] = T[a][i][16 q + j]
 * (a lane's 16 MFMA operands of one node are contiguous); d_T and d_b0 16-byte aligned.  The
 * envs are sorted by target within domains of 1,024 (each block takes its 128-env slice of its
 * domain's order), so a wave's 16 envs mostly share one target's table, and the layer runs on the
 * MFMAs (k = node, 0/1 state bits as the B operand);
 * its sums are exact f32 but grouped differently from pbn_bilinear_targets' sequential adds:
 * compare with a tolerance.  This is config 5's acting frame in one launch before pbn_step.
 */
int pbn_qnet_heads_from_state(const pbn_net* net, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                              const float* d_T, const float* d_b0, const float* d_w1, const float* d_b1,
                              const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3,
                              const float* d_wh1, const float* d_bh1, const float* d_wh2, const float* d_bh2,
                              int32_t n_heads, int32_t n_actions, float slope, float* d_heads, void* stream);
int pbn_qnet_flipmask_from_state(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step,
                                 uint64_t env_offset, int64_t n_envs, const uint32_t* d_state,
                                 const uint8_t* d_target, const float* d_T, const float* d_b0, const float* d_w1,
                                 const float* d_b1, const float* d_w2, const float* d_b2, const float* d_w3,
                                 const float* d_b3, const float* d_wh1, const float* d_bh1, const float* d_wh2,
                                 const float* d_bh2, int32_t n_branches, int32_t n_actions, float slope,
                                 float epsilon, const float* d_epsilon, uint32_t* d_flipmask, int32_t* d_actions,
                                 void* stream);

/*
 * n transitions into the learner's replay ring (pbn_rl_amd/replay.py DeviceReplay), in one launch:
 * env e's state / next_state (uint32 [words][n]), target (uint8 [n]), action (int32 [n][n_branches]),
 * reward (float [n]) and done (uint8 [n], nonzero = done) go to slot (*d_pos + e) mod capacity of
 * the ring arrays (state / next_state uint32 [words][capacity], target uint8 [capacity], action
 * int32 [capacity][n_branches], reward float [capacity], done uint8 [capacity] as 0/1).  d_pos
 * (int64, device memory) is read, not advanced.  capacity >= n.  With done_mask != 0, d_done is the
 * env's flags and done = (flags & done_mask) != 0 (PBN_FLAG_TERMINATED | PBN_FLAG_TRUNCATED: the
 * frame's done); d_done_out (optional, uint8 [n]) receives the same 0/1.  The optional pairs
 * d_state_dst / d_state_src (uint32 [words][n]) and d_target_dst / d_target_src (uint8 [n]) are
 * element copies done in the same pass after each element of d_state / d_target is read (a
 * destination may be d_state / d_target itself): a captured frame's copy of the stepped state back
 * into the env and its carried pre-step target, without launches of their own.
 */
int pbn_replay_store(int64_t n, const int64_t* d_pos, int64_t capacity, int32_t words, int32_t n_branches,
                     const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                     const int32_t* d_action, const float* d_reward, const uint8_t* d_done, uint32_t done_mask,
                     uint8_t* d_done_out, uint32_t* d_ring_state, uint32_t* d_ring_next_state, uint8_t* d_ring_target,
                     int32_t* d_ring_action, float* d_ring_reward, uint8_t* d_ring_done, uint32_t* d_state_dst,
                     const uint32_t* d_state_src, uint8_t* d_target_dst, const uint8_t* d_target_src, void* stream);

/*
 * A captured learning frame's counters and the update's rows, one single-block launch (no
 * reference counterpart: the reference keeps these on the host).  All int64 / double / float
 * one-element device tensors; each optional one is skipped when null:
 *   n_store > 0   *d_pos = (*d_pos + n_store) mod capacity, *d_size = min(*d_size + n_store, capacity)
 *   d_step        += 1 (the env step index of the next frame)
 *   d_eps64       = max(eps_final, *d_eps64 - eps_step) (decrement_epsilon, bdq_model/__init__.py:141-148);
 *                   d_eps32 its fp32 copy
 *   n_idx > 0     d_idx int64 [n_idx]: rows uniform over [0, *d_size) with replacement (row b of draw
 *                 c = *d_counter: mulhi64 of the REPLAY Philox pair of (seed, b, c) and the size);
 *                 *d_counter then advances by 1
 */
int pbn_replay_advance(int64_t n_store, int64_t capacity, int64_t* d_pos, int64_t* d_size, int64_t* d_step,
                       double* d_eps64, float* d_eps32, double eps_final, double eps_step, int64_t n_idx,
                       uint64_t seed, int64_t* d_counter, int64_t* d_idx, void* stream);

/*
 * One replay batch for the learner's update (pbn_rl_amd/replay.py DeviceReplay), in one launch:
 * rows d_idx[0..batch) (int64, < capacity) of the ring -- d_state / d_next_state uint32 [W][capacity],
 * d_target uint8 [capacity], d_action int32 [capacity][n_branches], d_reward float [capacity],
 * d_done uint8 [capacity] -- into
 *   d_x       float [2][2 batch][N]: plane 0 = the states (rows 0..batch-1) and next states
 *             (rows batch..2 batch-1) as 0/1, plane 1 = the first state of each row's target
 *             attractor (zeros without one), i.e. pbn_obs_unpack of both, concatenated by rows
 *   d_actions int64 [batch][n_branches], d_rewards float [batch], d_masks float [batch] (= done)
 */
int pbn_replay_batch(const pbn_net* net, int64_t batch, const int64_t* d_idx, int64_t capacity,
                     const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                     const int32_t* d_action, int32_t n_branches, const float* d_reward, const uint8_t* d_done,
                     float* d_x, int64_t* d_actions, float* d_rewards, float* d_masks, void* stream);

/*
 * The learner's TD loss on raw head outputs (bdq_model/__init__.py:111-126; pbn_rl_amd/replay.py
 * bdq_update), and its gradient, in one launch:
 *   d_online  in   float [K+1][2B][A]: the online network's raw head outputs (head 0 = value,
 *                  output 0) for the batch's states (rows 0..B-1) and next states (rows B..2B-1)
 *   d_target  in   float [K+1][B][A]: the target network's raw head outputs for the next states
 *   d_actions in   int64 [B][K], d_rewards float [B], d_masks float [B]
 *   d_loss    out  float [1]: mean over (b, k) of (r_b + q_T(b, k, a*) gamma m_b - q(b, k, a_bk))^2,
 *                  q = (v + adv_a) - mean(adv) (the dueling), a* = argmax_a q(B + b, k, a) (first
 *                  maximum, NaN maximal)
 *   d_grad    out  float [K+1][2B][A]: d loss / d d_online (0 for rows B.. and the value head's
 *                  outputs past 0)
 *   d_scratch      float [ceil(B / 8)]: per-block partial sums of the loss
 * batch = B, n_branches = K (1..7), n_actions = A (1..128).  fp32; the dueling means are
 * sequential sums, so the values equal PyTorch's to rounding.  Two launches (the pass over the
 * rows, then the partial sums added in order).
 */
int pbn_bdq_td_loss(const float* d_online, const float* d_target, const int64_t* d_actions, const float* d_rewards,
                    const float* d_masks, int32_t batch, int32_t n_branches, int32_t n_actions, float gamma,
                    float* d_loss, float* d_grad, float* d_scratch, void* stream);

/*
 * pbn_bdq_td_loss with per-row importance weights (prioritised replay; DDQNPER._learn_step,
 * ddqn_per/__init__.py:468-483, with the BDQ's MSE).  Additive export (the ABI version is unchanged).
 *   d_weights  in   float [B]: w_b
 *   d_priority out  float [B]: |w_b l_b| + replay_constant, l_b = mean_k (expected - current)^2
 *   d_loss     out  float [1]: mean_b w_b l_b;  d_grad is its gradient (row b's scaled by w_b)
 * Every other argument as pbn_bdq_td_loss; float buffers 4-byte, d_actions 8-byte aligned.
 */
int pbn_bdq_td_loss_per(const float* d_online, const float* d_target, const int64_t* d_actions,
                        const float* d_rewards, const float* d_masks, const float* d_weights, int32_t batch,
                        int32_t n_branches, int32_t n_actions, float gamma, float replay_constant, float* d_loss,
                        float* d_grad, float* d_priority, float* d_scratch, void* stream);

/*
 * The whole update_policy step (bdq_model/__init__.py:100-139) on a flat parameter buffer, for the
 * reference's network BranchingQNetwork((N, N), N + 1, K) (bdq_model/network.py:24-63: bilinear
 * N x N -> 256, trunk 256-128-64-32, K + 1 heads 32-64-(N+1), LeakyReLU).  Replaces the sampled
 * batch's np.stack and upload (:102-109), both forwards, the target, the MSE, the backward, the
 * per-tensor gradient clamp (:129-130) and optimizer.step() (:131): three launches.
 *
 * pbn_bdq_layout: offsets[0..11] (floats, 16-float aligned) of the segments bilinear weight
 *   (256, N, N), bilinear bias (256), the trunk's three weight (out, in) / bias pairs, the heads'
 *   first layers (K+1, 64, 32) and biases (K+1, 64), second layers (K+1, N+1, 64) and biases
 *   (K+1, N+1) -- head 0 is the value head, whose rows / biases past output 0 are zero padding;
 *   offsets[12] = the total.  Parameters, Adam's moments and d_grad share this layout.
 * pbn_bdq_learn_workspace: bytes of the update's workspace at batch B (a multiple of 16).
 * pbn_bdq_image_floats (ABI 10): floats of a network's image, the d_Tq / d_target_Tq buffers.
 * pbn_bdq_pack: the image of the weights d_params into d_Tq: first the bilinear layer contracted
 *   with each attractor's first state, T[t][i][o] = sum_j x_t[j] W[o][i][j], stored
 *   [t][i][j][q] = T[t][i][16 q + j] (the table pbn_qnet_*_from_state read, n_attr * N * 256
 *   floats); then (ABI 10) the dense layers' weights as 16 x 16 tiles in the update kernels'
 *   MFMA-fragment orders (pbn_learn.hip make_image).  Needed once per parameter version not
 *   written by pbn_bdq_learn (initial weights, a loaded checkpoint, the target network after a
 *   soft update).
 * pbn_bdq_learn: rows d_idx [B] of the replay ring (the layout of pbn_replay_store);
 *   d_params / d_Tq the online network and its image (updated in place: Adam step, and the image
 *   of the new weights, equal to pbn_bdq_pack's bit for bit), d_target_params / d_target_Tq the
 *   target network and its image (read; the update reads the dense weights from the images); d_adam_m / d_adam_v the
 *   moments, d_adam_step float [1] Adam's step count (incremented on the device); the loss to
 *   d_loss float [1]; when d_grad is not null, the clamped gradient there.  Same arithmetic as
 *   pbn_rl_amd/replay.py bdq_update + torch.optim.Adam in fp32, to summation order.
 */
int pbn_bdq_layout(int32_t n_nodes, int32_t n_branches, int64_t* offsets);
int pbn_bdq_learn_workspace(int32_t n_nodes, int32_t n_branches, int64_t batch, int64_t* bytes);
int pbn_bdq_image_floats(const pbn_net* net, int32_t n_branches, int64_t* floats);
int pbn_bdq_pack(const pbn_net* net, int32_t n_branches, const float* d_params, float* d_Tq, void* stream);
/*
 * The learning frame's counters, advanced by the fused update's last launch (ABI 9): when
 * pbn_bdq_learn's `advance` is not null, learn_apply runs one more block that does what
 * pbn_replay_advance does for the frame just stored (position and fill level after n_store rows,
 * the env step index, epsilon's decay) and then draws the NEXT frame's n_idx rows into d_idx, over
 * the fill level that frame's store will leave (min(size + n_store, capacity)), with *d_counter,
 * which then advances.  A captured BDQ frame (pbn_rl_amd/replay.py BDQLearner) so needs no
 * launch of its own for the counters; its first rows are drawn before the first replay.  The
 * update itself reads d_idx before this block writes it (an earlier launch of the same call).
 */
typedef struct pbn_frame_advance {
  int64_t n_store, capacity;
  int64_t* d_pos;
  int64_t* d_size;
  int64_t* d_step;      /* nullable */
  double* d_eps64;      /* nullable */
  float* d_eps32;       /* nullable */
  double eps_final, eps_step;
  int64_t n_idx;
  uint64_t seed;
  int64_t* d_counter;
  int64_t* d_idx;
} pbn_frame_advance;

int pbn_bdq_learn(const pbn_net* net, int64_t batch, const int64_t* d_idx, int64_t capacity, const uint32_t* d_state,
                  const uint32_t* d_next_state, const uint8_t* d_target, const int32_t* d_action, int32_t n_branches,
                  const float* d_reward, const uint8_t* d_done, float* d_params, float* d_Tq,
                  const float* d_target_params, const float* d_target_Tq, float* d_adam_m, float* d_adam_v,
                  float* d_adam_step, float lr, float beta1, float beta2, float eps, float gamma, float grad_clamp,
                  float slope, void* d_workspace, int64_t workspace_bytes, float* d_loss, float* d_grad,
                  const pbn_frame_advance* advance, void* stream);

/*
 * pbn_bdq_learn_per: pbn_bdq_learn on a batch drawn by prioritised replay (pbn_per_sample), the
 * update of DDQNPER._learn_step (ddqn_per/__init__.py:468-483) with this MSE.  An additive export
 * (the ABI version is unchanged).  Every argument up to d_grad is pbn_bdq_learn's; then
 *   d_weights   in  float [B]  the rows' importance weights, by batch position (d_weights[b] belongs
 *                              to d_idx[b]; a batch may hold one ring row twice)
 *   d_priority  out float [B]  the rows' new priorities, by batch position (for pbn_per_update)
 * both required and 4-byte aligned.  In fp32, with d_bk = expected - current of row b, branch k:
 *   g_bk        = (2 (current - expected) / (B K)) * w_b   the gradient at the head outputs: the
 *                 unweighted value times w_b, so unit weights give pbn_bdq_learn's gradient, Adam
 *                 step and image bit for bit
 *   l_b         = (sum_k d_bk^2, k ascending) / K
 *   priority[b] = |w_b l_b| + replay_constant
 *   loss        = (sum_b w_b l_b) / B, the rows added in a fixed order (16-row blocks, then the
 *                 blocks in order)
 * The same three launches: the priorities are written by the backward's TD pass.  Rejects what
 * pbn_bdq_learn rejects, and a null or misaligned d_weights / d_priority.
 */
int pbn_bdq_learn_per(const pbn_net* net, int64_t batch, const int64_t* d_idx, int64_t capacity,
                      const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                      const int32_t* d_action, int32_t n_branches, const float* d_reward, const uint8_t* d_done,
                      float* d_params, float* d_Tq, const float* d_target_params, const float* d_target_Tq,
                      float* d_adam_m, float* d_adam_v, float* d_adam_step, float lr, float beta1, float beta2,
                      float eps, float gamma, float grad_clamp, float slope, void* d_workspace, int64_t workspace_bytes,
                      float* d_loss, float* d_grad, const float* d_weights, float replay_constant, float* d_priority,
                      const pbn_frame_advance* advance, void* stream);

/*
 * pbn_copy_async (ABI 7): d_dst[0 .. bytes) <- d_src[0 .. bytes), device to device on `stream`:
 * one kernel of 16-byte non-temporal loads and stores (the world-1 hand-off of a rollout's
 * transition records, pbn_rl_amd/distributed.py; hipMemcpyAsync's blit ran 22 MB at 3.9 TB/s,
 * profiles/r05_a_handoff_summary.json).  Both pointers and `bytes` 16-byte aligned; the ranges
 * must not overlap.
 */
int pbn_copy_async(void* d_dst, const void* d_src, int64_t bytes, void* stream);

/*
 * pbn_host_buffer (ABI 9): `bytes` of pinned host memory, coherent and mapped into the current
 * device's address space (hipHostMalloc, mapped | coherent): *h_ptr is its host address, *d_ptr
 * the address kernels use; pbn_host_buffer_free releases it.  The scalar gym facade (PBNEnv,
 * one env per step, config 1) keeps its 32-env group there, so that a step is one
 * pbn_step launch on those pointers and one pbn_stream_sync, with no copies
 * (gym_PBN's env.step(), bdq_model/__init__.py:177).
 */
int pbn_host_buffer(int64_t bytes, void** h_ptr, void** d_ptr);
int pbn_host_buffer_free(void* h_ptr);
/* pbn_stream_sync (ABI 9): waits until the work issued on `stream` has completed. */
int pbn_stream_sync(void* stream);

/*
 * Batched control evaluation (model_tester.py:587-658; pbn_rl_amd/evaluate.py): every (source
 * attractor, target attractor, run) is one env, and a protocol step is act -> pbn_step_dev ->
 * pbn_eval_track on one stream.  Additive exports (the ABI version is unchanged).
 *
 * pbn_eval_track: the bookkeeping of protocol step k = *d_step - step0 + 1 (d_step read when the
 * kernel runs, as pbn_step_dev reads it; a k outside 1..max_steps touches nothing).  n_alloc is a
 * multiple of 32, envs i >= n_real are padding.
 *   d_flags      in     uint8  [n]     the step's flags
 *   d_actions    in     int32  [n][K]  the acting kernel's actions (nullable without d_strategy)
 *   d_state      in     uint32 [W][n]  the state after the step
 *   d_count      in/out int32  [n]
 *   d_open       in/out uint8  [n]     nonzero = the run has not ended
 *   d_hit_state  in/out uint32 [W][n]  nullable
 *   d_strategy   in/out int16  [max_steps][n][K]  nullable
 *   d_open_after in/out int32  [max_steps + 1]    the caller zeroes it
 * Per env i < n_real with d_open[i]: strategy[k-1][i][:] = actions[i][:]; if flags[i] has
 * PBN_FLAG_TERMINATED, count[i] = k, open[i] = 0 and hit_state[:, i] = state[:, i]; else if
 * k == max_steps, count[i] = max_steps + 1 (the reference's 101, :635) and open[i] = 0.  Closed and
 * padding envs are neither read for actions nor written.  d_open_after[k] += the envs still open
 * after the step, one atomic per wave.  1 <= max_steps <= 254 (the step kernels' t is uint8),
 * K = n_branches 1..64, W = words 1..4; the int32 / uint32 buffers 4-byte, d_strategy 2-byte,
 * d_step 8-byte aligned.
 *
 * pbn_eval_reduce: d_count int32 [n_pairs][runs] (env i = pair * runs + run; runs need not be a
 * multiple of the wave) -> d_pair_sum int64 [n_pairs] (a failure adds max_steps + 1, the
 * reference's `+= 101`), d_pair_fail int32 [n_pairs], and d_hist int64 [max_steps + 2] += the
 * number of runs of every length (bin max_steps + 1 = failures; the caller zeroes it; built per
 * block in LDS, one atomic per non-empty bin).  Counts outside 0..max_steps + 1 are clamped.
 */
int pbn_eval_track(int64_t n_alloc, int64_t n_real, int32_t words, int32_t n_branches, int32_t max_steps,
                   const int64_t* d_step, int64_t step0, const uint8_t* d_flags, const int32_t* d_actions,
                   const uint32_t* d_state, int32_t* d_count, uint8_t* d_open, uint32_t* d_hit_state,
                   int16_t* d_strategy, int32_t* d_open_after, void* stream);
int pbn_eval_reduce(const int32_t* d_count, int64_t n_pairs, int64_t runs, int32_t max_steps, int64_t* d_pair_sum,
                    int32_t* d_pair_fail, int64_t* d_hist, void* stream);

/*
 * Proportional prioritised replay (PrioritisedER, bdq_model/memory.py:73-186) over a sum and a min
 * segment tree held on the device.  Additive exports (the ABI version is unchanged).
 *
 * tree_size = T, a power of two >= capacity (the reference takes the smallest); capacity >= 2.
 * d_sum_tree / d_min_tree are double [2T]: node 1 is the root, leaf i is node T + i, a sum node is
 * left + right, a min node is min(left, right); the caller initialises every sum node to 0.0 and
 * every min node to +inf (empty), *d_max_priority to 1.0.  Every entry keeps each ancestor equal to
 * the operation of its two children, rebuilt level by level.  All counters are read from device
 * memory when the kernels run, so every launch can be captured in a graph.  Pointers are 8-byte
 * (float buffers 4-byte) aligned.
 *
 * pbn_per_store: the n (1..capacity) transitions stored at ring position *d_pos get the priority
 *   *d_max_priority ** alpha, at leaves (*d_pos + 1 + j) mod capacity, j < n -- the slot after
 *   each stored row, as memory.py:114 has it.  *d_pos is the position before the store (the
 *   caller advances it afterwards).  At most two launches: the touched 512-leaf chunks and their
 *   subtrees, then the levels above the chunks.
 * pbn_per_sample: batch (1..1024) rows proportional to priority, one block.  N = *d_size;
 *   p_total = the sum of leaves [0, N - 2] in the association of the reference's recursion
 *   (data_structures.py:33-60); row i searches mass = u_i * (p_total / batch) + i * (p_total /
 *   batch) (find_prefixsum_index) with u_i = ((x << 21) | (y >> 11)) * 2^-53 from the REPLAY Philox
 *   words (x, y) of (seed, id = i, step = *d_counter); the index is clamped to [0, N - 1].
 *   d_weights[i] = float((N leaf_i / S) ** -beta / (N min / S) ** -beta), S the sum root, min the
 *   min root, beta = *d_beta, all in fp64.  Then *d_beta = min(max_beta, beta + beta_step) and
 *   *d_counter += 1.   d_idx int64 [batch], d_weights float [batch].
 * pbn_per_update: leaf d_idx[b] = double(d_priorities[b]) ** alpha in both trees, the pairs applied
 *   in order (of equal indices the highest b wins); *d_max_priority = max of itself and every applied
 *   priority; pairs with an index outside [0, *d_size) are skipped.  One block, batch 1..1024.
 */
int pbn_per_store(int64_t n, const int64_t* d_pos, int64_t capacity, int64_t tree_size, double alpha,
                  const double* d_max_priority, double* d_sum_tree, double* d_min_tree, void* stream);
int pbn_per_sample(int32_t batch, int64_t capacity, int64_t tree_size, const int64_t* d_size,
                   const double* d_sum_tree, const double* d_min_tree, double* d_beta, double max_beta,
                   double beta_step, uint64_t seed, int64_t* d_counter, int64_t* d_idx, float* d_weights,
                   void* stream);
int pbn_per_update(int32_t batch, int64_t capacity, int64_t tree_size, double alpha, const int64_t* d_size,
                   const int64_t* d_idx, const float* d_priorities, double* d_max_priority, double* d_sum_tree,
                   double* d_min_tree, void* stream);

/*
 * The DDQN / DDQNPER agent (ddqn_per/__init__.py, ddqn_per/network.py; pbn_rl_amd/ddqn.py,
 * csrc/pbn_ddqn.hip).  Additive exports (the ABI version is unchanged).  The network is the
 * reference's DQN with one hidden Linear (network.py:24-28): input = nn.Bilinear(N, N, h0), ReLU,
 * linears.0 = Linear(h0, h1), ReLU, output = Linear(h1, N + 1); h0, h1 in 1..64, N + 1 <= 128.
 * None of these allocates or synchronises; every counter is read from device memory when the
 * kernels run, so every launch can be captured in a graph.
 *
 * pbn_dqn_layout: the float offsets of the flat parameter buffer's six segments, each 16-float
 *   aligned, then its size (offsets[7]): input.weight (h0, N, N), input.bias, linears.0.weight
 *   (h1, h0), linears.0.bias, output.weight (N + 1, h1), output.bias.  Parameters, Adam's moments
 *   and the gradient share it.
 * pbn_dqn_image_floats / pbn_dqn_pack: the network's image, what the acting and update kernels
 *   read (H0p, H1p, Ap: h0, h1, N + 1 rounded up to multiples of 16; padding is zero):
 *     T   [n_attr][N][H0p]  T[t][i][o] = sum_j x_t[j] W[o][i][j], x_t attractor t's first state, j
 *                           ascending: DQN.forward's first layer (network.py:40) is
 *                           bias + sum_{i: s_i = 1} T[target][i][:]; target id 255 reads no row
 *     the three biases, padded; then 16 x 16 tiles in v_mfma_f32_16x16x4_f32 fragment order:
 *     linears.0.weight (lane 16g + r of tile (ot, kt) holds W[16 ot + r][16 kt + 4g + v]), the
 *     same for the backward's transposed product (W[16 ot + 4g + v][16 kt + r]), output.weight.
 *   d_params and d_image 16-byte aligned.
 * pbn_dqn_flipmask_from_state: DDQN.predict (ddqn_per/__init__.py:155-179) for n_envs envs (any
 *   multiple of 32) in one launch: packed state uint32 [W][n] + target id uint8 [n] + image -> Q
 *   (d_q float [n][N + 1], nullable) -> epsilon-greedy -> d_actions int32 [n] (nullable) and
 *   d_flipmask uint32 [W][n] (action 0 is the no-op, :351; action a > 0 flips node a - 1).  The
 *   EXPLORE law of pbn_q_to_flipmask with one branch: explore iff EXPLORE word 0 of (seed, env_offset
 *   + env, step) < floor(epsilon * 2^32), then a = (word 1 * (N + 1)) >> 32; else the first maximum
 *   of Q.  d_step / d_epsilon, when not null, replace step / epsilon and are read by the kernel.
 * pbn_ddqn_learn_workspace / pbn_ddqn_learn: DDQN._learn_step (:275-278: _get_loss :218-256,
 *   _back_propagate :258-267) or, with d_weights and d_priority, DDQNPER._learn_step (:468-483) on
 *   rows d_idx[B] of the replay ring (pbn_replay_store's layout, n_branches = 1; B a multiple of 16
 *   in 16..1024).  In fp32, g_b the row's target attractor's first state:
 *     q_b = Q(s_b, g_b)[a_b];  a'_b = argmax_a Q(s'_b, g_b) (first maximum)
 *     y_b = r_b + (1 - done_b) gamma Q_target(s'_b, g_b)[a'_b];  delta_b = q_b - y_b
 *     h_b = 0.5 delta_b^2 if |delta_b| < 1 else |delta_b| - 0.5
 *     l_b = w_b h_b (h_b without weights);  loss = (sum_b l_b, b ascending) / B
 *     d_priority[b] = |l_b| + replay_constant, by batch position
 *     dloss/dq_b = (clamp(delta_b, -1, 1) / B) * w_b: unit weights give the unweighted update's
 *     gradient, Adam step and image bit for bit
 *   then clip_grad_norm_ (total = the L2 norm of the whole gradient, coef = min(1, max_grad_norm /
 *   (total + 1e-6)), every gradient times coef), torch.optim.Adam's step on d_params / d_adam_m /
 *   d_adam_v (layout as d_params; *d_adam_step, a float, is incremented), and the new online image
 *   (bit-equal to pbn_dqn_pack of the new weights).  The target network enters through its image
 *   alone.  Outputs: d_loss[1], d_grad_norm[1] (total, before clipping) and, when d_grad is not null,
 *   the clipped gradient in the layout.  Four launches (forward + TD + backward; gradient tiles and
 *   per-block sums of squares; norm + clip + Adam; image); every sum runs in a fixed order, so two
 *   runs from the same state give the same bits.  Rejects shapes outside the above, a null or
 *   misaligned buffer (parameters, moments, images, workspace, d_grad: 16-byte), one of d_weights /
 *   d_priority without the other, and a workspace smaller than pbn_ddqn_learn_workspace's.
 */
int pbn_dqn_layout(int32_t n_nodes, int32_t h0, int32_t h1, int64_t* offsets);
int pbn_dqn_image_floats(const pbn_net* net, int32_t h0, int32_t h1, int64_t* n_floats);
int pbn_dqn_pack(const pbn_net* net, int32_t h0, int32_t h1, const float* d_params, float* d_image, void* stream);
int pbn_dqn_flipmask_from_state(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step,
                                uint64_t env_offset, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                                int32_t h0, int32_t h1, const float* d_image, float epsilon, const float* d_epsilon,
                                float* d_q, uint32_t* d_flipmask, int32_t* d_actions, void* stream);
int pbn_ddqn_learn_workspace(int32_t n_nodes, int32_t h0, int32_t h1, int64_t batch, int64_t* bytes);
int pbn_ddqn_learn(const pbn_net* net, int32_t h0, int32_t h1, int64_t batch, const int64_t* d_idx, int64_t capacity,
                   const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                   const int32_t* d_action, const float* d_reward, const uint8_t* d_done, float* d_params,
                   float* d_image, const float* d_target_image, float* d_adam_m, float* d_adam_v, float* d_adam_step,
                   float lr, float beta1, float beta2, float eps, float gamma, float max_grad_norm, void* d_workspace,
                   int64_t workspace_bytes, float* d_loss, float* d_grad_norm, float* d_grad, const float* d_weights,
                   float replay_constant, float* d_priority, void* stream);

/*
 * pbn_ddqn_schedule: the device half of _schedule_step (ddqn_per/__init__.py:283-290, :488-490) for a
 * learning frame replayed from a hipGraph (pbn_rl_amd/ddqn.py DDQNLearner.capture).  An additive
 * export (the ABI version is unchanged).  One launch, placed after pbn_ddqn_learn's:
 *   *d_beta = min(*d_beta + beta_increment, 1.0) in fp64 (DDQNPER's increment_beta, :488-490, on the
 *     double pbn_per_sample reads);
 *   when (*d_step - step_base) mod target_update == 0, the hard target copy (:286-287):
 *     d_target_params[0 .. n_params) <- d_params and d_target_image[0 .. n_image) <- d_image, floats,
 *     as 16-byte vector loads and stores; otherwise every block exits after reading *d_step.
 * d_step is the env step index that pbn_replay_advance advanced earlier in the same frame, and
 * step_base its value before the learner's frame 0, so *d_step - step_base counts the frames done
 * and the copy falls on the frames f with (f + 1) mod target_update == 0.  The launch does not write
 * *d_step, so all its blocks decide alike, on every replay.  d_beta and d_step 8-byte, the four
 * buffers 16-byte aligned; n_params and n_image positive multiples of 4 (pbn_dqn_layout's and
 * pbn_dqn_image_floats' sizes are multiples of 16); target_update >= 1; a target buffer must not
 * overlap its source.  No atomics; nothing is allocated or synchronised.
 */
int pbn_ddqn_schedule(double* d_beta, double beta_increment, const int64_t* d_step, int64_t step_base,
                      int64_t target_update, float* d_target_params, const float* d_params, int64_t n_params,
                      float* d_target_image, const float* d_image, int64_t n_image, void* stream);

/*
 * pbn_rollout_dqn: pbn_rollout_ex with a DQN choosing every action inside the launch (the policy
 * rollout).  An additive export (the ABI version is unchanged).  Before step k of the launch the
 * wave that owns an env runs pbn_dqn_flipmask_from_state's forward on the env's current state and
 * target id (the ones step k - 1 left, an autoreset's new target included), takes the first maximum
 * of Q and applies the EXPLORE law at (seed, env_offset + env, step + k): explore iff word 0 <
 * floor(epsilon * 2^32), then a = (word 1 * (N + 1)) >> 32.  The action's flip mask is the step's
 * intervention; from there the step is pbn_rollout_ex's.  The actions, flip masks and every other
 * output equal those of n_steps rounds of pbn_dqn_flipmask_from_state followed by pbn_step, bit
 * for bit, under either step law.
 *   d_image      pbn_dqn_pack's image of the network (h0, h1), 16-byte aligned
 *   d_flipmask   out [n_steps][W][n]: the flip masks of the actions taken
 *   d_actions    out [n_steps][n] int32, nullable
 *   mode         PBN_MODE_AUTORESET or 0; PBN_MODE_RANDOM_ACTIONS is rejected
 * Preconditions and the other buffers as pbn_rollout_ex: whole 32-env groups, the state stepped in
 * place, every element of every given buffer written; n_steps == 0 or n_envs == 0 is a successful
 * no-op.  Shapes as pbn_dqn_pack (N + 1 <= 128, hidden widths 1..64); epsilon in [0, 1].  Every
 * argument error returns PBN_EINVAL before any device call.
 */
int pbn_rollout_dqn(pbn_net* net, uint64_t seed, uint64_t step, uint64_t env_offset, int64_t n_envs,
                    int32_t n_steps, uint32_t mode, uint32_t* d_state, uint8_t* d_target, uint8_t* d_t,
                    int32_t h0, int32_t h1, const float* d_image, float epsilon,
                    uint32_t* d_flipmask /* out [n_steps][W][n] */, int32_t* d_actions /* out [n_steps][n], nullable */,
                    uint32_t* d_obs, uint32_t* d_final_state, float* d_reward, uint8_t* d_flags,
                    uint16_t* d_updates, void* stream);

/*
 * Episode statistics on the device (pbn_rl_amd/episode_stats.py EpisodeStats, csrc/pbn_episode.hip):
 * what the reference logs on the host every frame -- RecordEpisodeStatistics' rollout/ep_rew_mean and
 * rollout/ep_len_mean (ddqn_per/__init__.py:67,357-377), the BDQ loop's ep_len, ep_reward and
 * missed[(state_attractor_id, target_attractor_id)] (bdq_model/__init__.py:179-236) -- kept by one
 * call per frame that a captured frame can hold.  Additive exports (the ABI version is unchanged).
 * All buffers are the caller's; both calls are asynchronous on `stream` and allocate and synchronise
 * nothing.  n_alloc is a multiple of 32 and 0 < n_real <= n_alloc: envs i >= n_real are padding,
 * neither read nor written.
 *
 * Per-env state, [n_alloc] each: d_ret float (return of the open episode, the plain float sum of its
 * rewards in frame order), d_len uint32 (its steps), d_src uint8 (attractor id of its first state,
 * PBN_NO_TARGET if no attractor holds it), d_tgt uint8 (the target at its start).
 *
 * Aggregates, all int64 and written by integer atomics only, so that they do not depend on the
 * order of the adds; the caller zeroes them:
 *   d_totals [8]       frames, episodes, successes (closed with PBN_FLAG_TERMINATED), missed (closed
 *                      with PBN_FLAG_TRUNCATED and not terminated: the reference's `missed`), len_sum,
 *                      ret_sum, last_reward_sum (the closing step's reward: the BDQ loop's ep_reward =
 *                      reward), unpaired (closed episodes whose source or target is no attractor id)
 *   d_pairs [A][A][4]  per (source, target): episodes, missed, len_sum, ret_sum (A = the net's
 *                      attractors; null only when A == 0)
 *   d_hist [256]       closed episodes by length; bin 255 holds every length >= 255
 *   d_series [R][8]    a copy of d_totals every log_every frames (below)
 * A float enters a sum once, at the close, as the int64 __double2ll_rn((double)x * 1048576.0), i.e. in
 * units of 2^-20: ret_sum and last_reward_sum hold while |sum of the returns| < 2^43.
 *
 * pbn_episode_begin opens an episode for every env i < n_real from its current state and target
 * (after a reset or a set_state): ret = 0, len = 0, tgt = d_target[i], src = the attractor that holds
 * d_state[:, i] (the net's attractor hash, the one the step kernels probe; state words 1..4).
 *
 * pbn_episode_track is one frame's bookkeeping, after the step (and after a learner's ring store):
 * d_state / d_target hold what the step left, the fresh start and the new target where it autoreset.
 * Per env i < n_real: ret += d_reward[i], len += 1; if d_flags[i] & done_mask, the episode closes --
 * into the totals and d_hist[min(len, 255)], into d_pairs[src][tgt] when both are attractor ids, else
 * into `unpaired` -- and the next one opens from d_state[:, i] and d_target[i] as pbn_episode_begin
 * opens it.  Without autoreset a finished env keeps producing done steps, each of which closes a
 * one-step episode: the call is meant for autoreset envs.  Two launches: the envs, then one wave that
 * increments `frames` and, when log_every > 0 and frames % log_every == 0, copies the eight totals
 * into row (frames / log_every - 1) mod series_rows of d_series.  With log_every == 0 `frames` still
 * advances and d_series may be null.
 * Rejects: n_alloc not a positive multiple of 32, n_real outside 1..n_alloc, a done_mask that is zero
 * or has bits outside PBN_FLAG_TERMINATED | PBN_FLAG_TRUNCATED, a null buffer, float / uint32
 * buffers not 4-byte and int64 buffers not 8-byte aligned, log_every < 0, series_rows < 1 or a null
 * d_series with log_every > 0, a null d_pairs on a net with attractors.
 */
int pbn_episode_begin(const pbn_net* net, int64_t n_alloc, int64_t n_real, const uint32_t* d_state,
                      const uint8_t* d_target, float* d_ret, uint32_t* d_len, uint8_t* d_src, uint8_t* d_tgt,
                      void* stream);
int pbn_episode_track(const pbn_net* net, int64_t n_alloc, int64_t n_real, uint32_t done_mask, const float* d_reward,
                      const uint8_t* d_flags, const uint32_t* d_state, const uint8_t* d_target, float* d_ret,
                      uint32_t* d_len, uint8_t* d_src, uint8_t* d_tgt, int64_t* d_totals, int64_t* d_pairs,
                      int64_t* d_hist, int64_t log_every, int64_t series_rows, int64_t* d_series, void* stream);

/*
 * Curriculum resets on the device (pbn_rl_amd/curriculum.py Curriculum, csrc/pbn_curriculum.hip; the
 * law is csrc/curriculum_law.h's, DESIGN.md "Curriculum resets"): the reference's
 * env.rework_probas(ep_len) (bdq_model/__init__.py:203) as two stages of a learning frame.  The step
 * kernels keep the step law's uniform autoreset; pbn_curriculum_redraw then restarts the envs the
 * step reset from a draw weighted by pbn_episode_track's pair statistics, and pbn_curriculum_refresh
 * rebuilds the weights' prefix sums from them.  Additive exports (the ABI version is unchanged).  Both
 * calls are asynchronous on `stream` and allocate and synchronise nothing.
 *
 * The table: one caller-owned device buffer of pbn_curriculum_table_bytes(A) bytes, 8-byte aligned,
 * A = the net's attractors, 2..254.  With H = the spec's horizon (20 if it has none), E =
 * d_pairs[s][t].episodes and L = d_pairs[s][t].len_sum:
 *   w[s][t] = 0 if s == t, else min(floor(((H + L) << 8) / (1 + E)), 2^24 - 1)   (in uint64)
 * and the buffer holds, in this order,
 *   uint64 rowcdf[A]   rowcdf[s] = the sum of rows 0..s of w
 *   uint32 cdf[A][A]   cdf[s][t] = w[s][0] + ... + w[s][t]; then padding to a multiple of 8 bytes
 *   uint64 total       rowcdf[A - 1], below 2^40
 *   uint64 refreshes   the rebuilds so far (the caller zeroes it)
 * pbn_curriculum_table_bytes returns the size, or PBN_EINVAL for A outside 2..254.
 *
 * pbn_curriculum_redraw belongs after the step (and a learner's ring store) and before
 * pbn_episode_track, so that the episode it opens is the redrawn one.  For every env i < n_real with
 * d_flags[i] & PBN_FLAG_RESET and (x0, x1, x2, x3) = Philox call 0 of stream CURRICULUM (8) of env
 * env_offset + i at the step's index k:
 *   v = floor((x1:x0) total / 2^64), s = min{s : rowcdf[s] > v}, v' = v - rowcdf[s - 1] (rowcdf[-1] = 0),
 *   t = min{t : cdf[s][t] > v'} (never s), row = att_start[s] + floor((x3:x2) size_s / 2^64)
 * and d_state[:, i] becomes row `row` of the net's attractor-state table, d_target[i] = t, and
 * d_target_copy[i] = t where d_target_copy is given (a captured settle-law frame carries the targets
 * in a second buffer).  k is *d_step when d_step is given (read when the kernel runs: the index the
 * captured frame's step used, before pbn_replay_advance), else `step` (an eager frame: the env's step
 * index minus one after the step).  Every other env, and everything at i >= n_real, is neither read
 * beyond its flag nor written.  d_state is [W][n_alloc] with W the net's state words, 1..4.
 * Rejects, in this order: a null or foreign net, a net with fewer than two attractors, n_alloc not a
 * positive multiple of 32 below 2^31, n_real outside 1..n_alloc, a null d_flags, d_state, d_target or
 * d_table, d_state not 4-byte or d_table not 8-byte aligned, d_step not 8-byte aligned.
 *
 * pbn_curriculum_refresh belongs after pbn_episode_track (whose second launch counted the frame).
 * One single-block launch: when refresh_every > 0 and d_totals[0] % refresh_every == 0, or when
 * refresh_every == -1 ("now"), the whole table is rebuilt from d_pairs [A][A][4] in integers, the
 * same for every schedule, and `refreshes` goes up by one; otherwise nothing is written.
 * refresh_every == 0 never rebuilds and launches nothing.  horizon is H above.
 * Rejects, in this order: n_attr outside 2..254, horizon outside 1..65535, refresh_every < -1, a null
 * d_pairs or d_table, a null d_totals with refresh_every > 0, a buffer not 8-byte aligned.
 */
int pbn_curriculum_table_bytes(int32_t n_attr);
int pbn_curriculum_redraw(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step, uint64_t env_offset,
                          int64_t n_alloc, int64_t n_real, const uint8_t* d_flags, uint32_t* d_state, uint8_t* d_target,
                          uint8_t* d_target_copy, const void* d_table, void* stream);
int pbn_curriculum_refresh(const int64_t* d_totals, const int64_t* d_pairs, int32_t n_attr, int32_t horizon,
                           int64_t refresh_every, void* d_table, void* stream);

/*
 * The GBDQ graph agent's front (gbdq_model/network.py:73-79; DESIGN.md "GBDQ"): the three
 * EdgeConv(add) + BatchNorm1d (training mode, one env at a time) + ReLU layers from the packed state,
 * one launch, the activations in LDS (csrc/pbn_gbdq.hip; layouts and LDS carving: csrc/gbdq_front.h).
 * Additive exports (the ABI version is unchanged).  N = the net's nodes.
 *
 * pbn_gbdq_pack builds the kernel's image (pbn_gbdq_image_floats floats, 16-byte aligned) from
 *   d_conv      in  float, flat, in this order: for layer l = 1, 2, 3 the conv model's first Linear
 *                   weight [64][in_l] and bias [64], its second Linear weight [N][64] and bias [N]
 *                   (in_1 = 4, in_2 = in_3 = 2 N); then BatchNorm weight [N] and bias [N] of bn1, bn2, bn3
 *   d_csr_start in  int32 [N + 1], d_csr_src int32 [n_edges]: the edge list grouped by target node:
 *                   node i receives, in this order, the messages of the source nodes
 *                   d_csr_src[d_csr_start[i] .. d_csr_start[i + 1])
 * The image holds the layer-1 message table M1[16][N] (row = s_i | t_i << 1 | s_j << 2 | t_j << 3,
 * computed in fp32 with sequential, unfused sums: over the 4 inputs from 0, then + bias, ReLU, over
 * the 64 hidden units from 0, then + bias), layers 2 and 3 as [A - Bm | Bm] (the first Linear split
 * in its x_i and x_j - x_i halves) and the transposed second Linear, zero-padded to the MFMA tiles.
 *
 * pbn_gbdq_front: d_out float [n][N N], row e = the (N, N) activations after bn3 + ReLU of env e's
 * observation (node features (state bit, bit of the target attractor's first state; zeros for a
 * target id without an attractor)), each BatchNorm normalising every (env, node) row over its own N
 * features (biased variance, eps 1e-5).  Every sum has a fixed order: two runs give the same bits.
 * n_envs a multiple of 32, n_envs N N < 2^31; d_image and d_out 16-byte aligned.  PBN_EINVAL when the
 * LDS carving of gbdq_front.h does not fit one block.
 */
int pbn_gbdq_image_floats(const pbn_net* net, int32_t n_edges, int64_t* n_floats);
int pbn_gbdq_pack(const pbn_net* net, const float* d_conv, int32_t n_edges, const int32_t* d_csr_start,
                  const int32_t* d_csr_src, float* d_image, void* stream);
int pbn_gbdq_front(const pbn_net* net, int64_t n_envs, const uint32_t* d_state, const uint8_t* d_target,
                   const float* d_image, float* d_out, void* stream);

/*
 * pbn_replay_store into two rings (gbdq_model/__init__.py:183-200: terminated transitions go to
 * memory_positive, all others to memory_negative), a stable partition in env order: with
 * terminated_e = (d_flags[e] & term_mask) != 0, the r-th terminated env goes to slot
 * (*d_pos_p + r) mod capacity_p of the positive ring, the r-th other env to slot
 * (*d_pos_n + r) mod capacity_n of the negative ring; the stored done is (d_flags[e] & done_mask) != 0.
 * Ring arrays as pbn_replay_store's.  Three launches on `stream`, no atomics and no waiting between
 * blocks: per-block counts into d_work (int32 [ceil(n / 256)]); every block adds the counts of the
 * blocks before it, in order, and stores its rows; one thread then writes d_counts (int64 [2]: the
 * positive and the negative count) and advances both rings: *d_pos = (*d_pos + count) mod capacity,
 * *d_size = min(*d_size + count, capacity).  Both capacities >= n; term_mask and done_mask nonzero.
 */
int pbn_replay_store_split(int64_t n, int32_t words, int32_t n_branches, const uint32_t* d_state,
                           const uint32_t* d_next_state, const uint8_t* d_target, const int32_t* d_action,
                           const float* d_reward, const uint8_t* d_flags, uint32_t term_mask, uint32_t done_mask,
                           int64_t capacity_p, int64_t* d_pos_p, int64_t* d_size_p, uint32_t* d_ring_state_p,
                           uint32_t* d_ring_next_state_p, uint8_t* d_ring_target_p, int32_t* d_ring_action_p,
                           float* d_ring_reward_p, uint8_t* d_ring_done_p, int64_t capacity_n, int64_t* d_pos_n,
                           int64_t* d_size_n, uint32_t* d_ring_state_n, uint32_t* d_ring_next_state_n,
                           uint8_t* d_ring_target_n, int32_t* d_ring_action_n, float* d_ring_reward_n,
                           uint8_t* d_ring_done_n, int32_t* d_work, int64_t* d_counts, void* stream);

/*
 * The ControlGBDQ agent's tail (control_gbdq_model/network.py:43-78, control_gbdq_model/__init__.py:
 * 64-86; DESIGN.md "ControlGBDQ"): Linear(N N, 256) + ReLU, two Linear(256, 256) + ReLU, a
 * Linear(256, 1) value head and C = n_ctrl Linear(256, 2) advantage heads, in one MFMA launch
 * (csrc/pbn_cgbdq.hip; parameter order, image layout and LDS carving: csrc/cgbdq_tail.h).  Additive
 * exports (the ABI version is unchanged).  N = the net's nodes (at most 128), n_ctrl 1..128.
 *
 * pbn_cgbdq_pack builds the image (pbn_cgbdq_image_floats floats, 16-byte aligned) from
 *   d_tail   in  float, flat, torch's (out, in) layout, in this order: model.0 weight [256][N N] and
 *                bias [256], model.2 and model.4 weight [256][256] and bias [256], value_head weight
 *                [256] and bias [1], then for head k = 0 .. C - 1 its weight [2][256] and bias [2]
 * Every dense layer is stored as v_mfma_f32_16x16x4_f32 A fragments (a tile's four operands of 16
 * inputs are one contiguous 1 KiB), the inputs beyond N N and the head rows beyond 1 + 2 C zero; the
 * head rows are stacked, the value head first, then (head k, output a) at row 1 + 2 k + a.
 *
 * pbn_cgbdq_heads (for tests, as pbn_qnet_heads):
 *   d_front  in   float [n][N N]: pbn_gbdq_front's output
 *   d_heads  out  float [n][1 + 2 C]: the raw value and advantage outputs, rows as stacked above
 *
 * pbn_cgbdq_flipmask: the same layers by the same code (heads bit-equal to pbn_cgbdq_heads'), then per
 * env and head k: mean = (adv_0 + adv_1) / 2, q_a = (v + adv_a) - mean, action = torch.argmax's (1 iff
 * q_1 > q_0 or q_1 is NaN and q_0 is not); epsilon-greedy by the EXPLORE law (explore iff word 0 <
 * floor(epsilon 2^32)): explore_mode 0 gives every head the value 0, 1 gives head k the value
 * (word_{k + 1} 2) >> 32, words numbered across the stream's calls; then the control flip mask
 *   d_ctrl_nodes in   int32 [C]: head k's node; an entry outside [0, N) keeps its head and sets no bit
 *   d_state      in   uint32 [W][n]: the envs' packed states
 *   d_flipmask   out  uint32 [W][n]: (state XOR values) AND control bits, values = OR of a_k << c_k
 *   d_actions    out  int32 [n][C] (nullable): the chosen values
 * d_step / d_epsilon: optional device pointers read when the kernel runs, as pbn_heads_to_flipmask's.
 * No head output goes to HBM.  Every sum has a fixed order: two runs give the same bits.
 * n_envs and env_offset multiples of 32, n_envs N N < 2^31; d_image 16-byte aligned.
 */
int pbn_cgbdq_image_floats(const pbn_net* net, int32_t n_ctrl, int64_t* n_floats);
int pbn_cgbdq_pack(const pbn_net* net, const float* d_tail, int32_t n_ctrl, float* d_image, void* stream);
int pbn_cgbdq_heads(const pbn_net* net, int64_t n_envs, const float* d_front, const float* d_image, int32_t n_ctrl,
                    float* d_heads, void* stream);
int pbn_cgbdq_flipmask(const pbn_net* net, uint64_t seed, uint64_t step, const uint64_t* d_step, uint64_t env_offset,
                       int64_t n_envs, const float* d_front, const float* d_image, int32_t n_ctrl,
                       const int32_t* d_ctrl_nodes, int32_t explore_mode, float epsilon, const float* d_epsilon,
                       const uint32_t* d_state, uint32_t* d_flipmask, int32_t* d_actions, void* stream);

const char* pbn_last_error(void);
int pbn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PBN_ENV_H */
