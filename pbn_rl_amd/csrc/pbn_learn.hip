// pbn_learn.hip -- the BDQ learner's update_policy step (bdq_model/__init__.py:100-139) as three
// HIP launches over one flat parameter buffer (SURVEY.md 8(f) #3, config 5's training frame).
//
// The reference's update is a PyTorch program: np.stack of 256 sampled transitions, two forwards
// of the online network and one of the target network, the double-DQN target, the MSE, autograd,
// a per-tensor gradient clamp and Adam (:100-131).  On the GPU that is ~100 kernels of a few
// microseconds each, and the frame waits on their launch latency, not on arithmetic (the whole
// update is ~0.3 GFLOP).  Here it is three launches, one header each: learn_fwd.h, learn_bwd.h,
// learn_apply.h, over learn_args.h (their arguments) and bdq_layout.h (the network's shape, the
// layouts and the LDS carvings).  This file is the host side: the entry points and the launches.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/pbn_env.h"
#include "host_check.h"
#include "net_view.h"
// (the kernels in this order: a listing numbers its functions, tools/listing_diff.py)
#include "learn_fwd.h"
#include "learn_bwd.h"
#include "learn_apply.h"
#include "bdq_pack.h"

namespace {

#ifdef PBN_STAMPS
unsigned long long* g_lstamps = nullptr;   // pbn_debug_set_learn_stamps
#endif

int check_branches(int n_branches) {
  if (n_branches < 1 || n_branches > 7) return pbn::set_error(PBN_EINVAL, "fused BDQ update: n_branches 1..7");
  return PBN_OK;
}

int check_shape(int N, int n_branches) {
  if (N < 1 || N > 127) return pbn::set_error(PBN_EINVAL, "fused BDQ update: 1 <= n_nodes <= 127");
  return check_branches(n_branches);
}

int check_batch(int64_t batch) {
  if (batch < kRows || batch % kRows || batch > (1 << 20))
    return pbn::set_error(PBN_EINVAL, "fused BDQ update: batch a multiple of 16, 16..2^20");
  return PBN_OK;
}

}  // namespace

extern "C" {

#ifdef PBN_STAMPS
// diagnostic builds: the learner kernels' phase clocks go to d_buf (uint64 [3][1024][8][32]), or
// nowhere when null
int pbn_debug_set_learn_stamps(unsigned long long* d_buf) {
  g_lstamps = d_buf;
  return PBN_OK;
}
#endif

int pbn_bdq_layout(int32_t n_nodes, int32_t n_branches, int64_t* offsets) {
  int rc = check_shape(n_nodes, n_branches);
  if (rc) return rc;
  if (!offsets) return pbn::set_error(PBN_EINVAL, "null offsets");
  make_layout(n_nodes, n_branches + 1, offsets);
  return PBN_OK;
}

int pbn_bdq_learn_workspace(int32_t n_nodes, int32_t n_branches, int64_t batch, int64_t* bytes) {
  int rc = check_shape(n_nodes, n_branches);
  if (rc) return rc;
  if (!bytes) return pbn::set_error(PBN_EINVAL, "null bytes");
  if ((rc = check_batch(batch))) return rc;
  if (BwdLds(n_branches + 1, apad(n_nodes), n_branches).bytes() > kLdsBytes)
    return pbn::set_error(PBN_EINVAL, "fused BDQ update: (n_branches + 1) x (n_nodes + 1) too large for one block's LDS");
  *bytes = make_work(n_nodes, n_branches + 1, batch).total * (int64_t)sizeof(float);
  return PBN_OK;
}

int pbn_bdq_image_floats(const pbn_net* net, int32_t n_branches, int64_t* floats) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = check_shape(v.n_nodes, n_branches))) return rc;
  if (!floats) return pbn::set_error(PBN_EINVAL, "null floats");
  ImageLayout im;
  make_image(v.n_nodes, n_branches + 1, v.n_attr, &im);
  *floats = im.total;
  return PBN_OK;
}

int pbn_bdq_pack(const pbn_net* net, int32_t n_branches, const float* d_params, float* d_Tq, void* stream) {
  pbn::NetView v;
  int rc = pbn::net_view(net, &v);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  if ((rc = check_shape(v.n_nodes, n_branches))) return rc;
  if (!d_params || !d_Tq) return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!pbn::aligned(d_params, 16) || !pbn::aligned(d_Tq, 16)) return pbn::set_error(PBN_EINVAL, "buffers: 16-byte aligned");
  const int N = v.n_nodes;
  LearnArgs a{};   // (pack_tiles_kernel reads the shape, the offsets and Tq)
  const ImageLayout im = set_shape(a, N, v.W, v.n_attr, v.att_first, n_branches);
  a.Tq = d_Tq;
  const hipStream_t s = (hipStream_t)stream;
  if (v.n_attr > 0) {
    hipLaunchKernelGGL(pack_kernel, dim3(v.n_attr * N), dim3(256), 0, s, d_params, a.off[BIL_W], N, v.W, v.att_first,
                       d_Tq);
    if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "pack_kernel launch failed");
  }
  const int64_t n4 = (im.total - im.fwd[0]) / 4;
  hipLaunchKernelGGL(pack_tiles_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, d_params, a, n4);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "pack_tiles_kernel launch failed");
  return PBN_OK;
}

}  // extern "C"

namespace {

// pbn_bdq_learn and pbn_bdq_learn_per: the argument checks, the LearnArgs fill and the three
// launches.  per: the rows carry importance weights (learn_bwd_kernel<true>); its own arguments and
// the shape arguments that need no net are checked first, before the net is looked at.
int learn_launch(bool per, const pbn_net* net, int64_t batch, const int64_t* d_idx, int64_t capacity,
                 const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                 const int32_t* d_action, int32_t n_branches, const float* d_reward, const uint8_t* d_done,
                 float* d_params, float* d_Tq, const float* d_target_params, const float* d_target_Tq, float* d_adam_m,
                 float* d_adam_v, float* d_adam_step, float lr, float beta1, float beta2, float eps, float gamma,
                 float grad_clamp, float slope, void* d_workspace, int64_t workspace_bytes, float* d_loss,
                 float* d_grad, const float* d_weights, float replay_constant, float* d_priority,
                 const pbn_frame_advance* advance, void* stream) {
  int rc;
  if (per) {
    if (!d_weights) return pbn::set_error(PBN_EINVAL, "pbn_bdq_learn_per: null d_weights");
    if (!d_priority) return pbn::set_error(PBN_EINVAL, "pbn_bdq_learn_per: null d_priority");
    if (!pbn::aligned(d_weights, 4)) return pbn::set_error(PBN_EINVAL, "pbn_bdq_learn_per: d_weights must be 4-byte aligned");
    if (!pbn::aligned(d_priority, 4)) return pbn::set_error(PBN_EINVAL, "pbn_bdq_learn_per: d_priority must be 4-byte aligned");
    if ((rc = check_branches(n_branches))) return rc;
    if ((rc = check_batch(batch))) return rc;
  }
  pbn::NetView nv;
  rc = pbn::net_view(net, &nv);
  if (rc) return rc;
  if ((rc = pbn::check_device(net))) return rc;
  const int N = nv.n_nodes;
  if ((rc = check_shape(N, n_branches))) return rc;
  int64_t need = 0;
  if ((rc = pbn_bdq_learn_workspace(N, n_branches, batch, &need))) return rc;
  if (capacity < 1) return pbn::set_error(PBN_EINVAL, "capacity >= 1");
  if (workspace_bytes < need) return pbn::set_error(PBN_EINVAL, "workspace too small (pbn_bdq_learn_workspace)");
  if (!d_idx || !d_state || !d_next_state || !d_target || !d_action || !d_reward || !d_done || !d_params ||
      !d_target_params || !d_adam_m || !d_adam_v || !d_adam_step || !d_workspace || !d_loss)
    return pbn::set_error(PBN_EINVAL, "null buffer");
  if (!d_Tq || !d_target_Tq) return pbn::set_error(PBN_EINVAL, "null network image");
  for (const void* p : {(const void*)d_params, (const void*)d_target_params, (const void*)d_adam_m,
                        (const void*)d_adam_v, (const void*)d_workspace, (const void*)d_Tq, (const void*)d_target_Tq})
    if (!pbn::aligned(p, 16)) return pbn::set_error(PBN_EINVAL, "parameter, table and workspace buffers: 16-byte aligned");
  LearnArgs a;
  a.idx = d_idx;
  a.B = (int)batch;
  a.cap = capacity;
  a.st = d_state;
  a.nst = d_next_state;
  a.tgt = d_target;
  a.act = d_action;
  a.rew = d_reward;
  a.done = d_done;
  set_shape(a, N, nv.W, nv.n_attr, nv.att_first, n_branches);
  a.P = d_params;
  a.Tq = d_Tq;
  a.PT = d_target_params;
  a.TqT = d_target_Tq;
  a.m = d_adam_m;
  a.v = d_adam_v;
  a.step = d_adam_step;
  a.lr = lr;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.gamma = gamma;
  a.clampv = grad_clamp;
  a.slope = slope;
  set_workspace(a, d_workspace, make_work(N, a.H, batch));
  a.loss = d_loss;
  a.grad = d_grad;
  a.wts = per ? d_weights : nullptr;
  a.prio = per ? d_priority : nullptr;
  a.rconst = per ? replay_constant : 0.f;
  a.stamps = nullptr;
#ifdef PBN_STAMPS
  a.stamps = g_lstamps;
#endif
  a.adv_on = 0;
  a.adv = pbn_frame_advance{};
  if (advance) {
    if (const char* msg = pbn::frame_advance_error(*advance, d_idx, batch)) return pbn::set_error(PBN_EINVAL, msg);
    a.adv_on = 1;
    a.adv = *advance;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)(batch / kRows);
  const size_t lds_f = FwdLds(a.H, a.A).bytes();
  if (lds_f > 64 * 1024 && hipFuncSetAttribute((const void*)learn_fwd_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f) != hipSuccess)
    return pbn::set_error(PBN_EDEVICE, "hipFuncSetAttribute failed");
  hipLaunchKernelGGL(learn_fwd_kernel, dim3(3 * tiles), dim3(kThreads), lds_f, s, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "learn_fwd_kernel launch failed");
  const size_t lds_b = BwdLds(a.H, a.Apad, a.K).bytes();
  void (*const bwd)(LearnArgs) = per ? learn_bwd_kernel<true> : learn_bwd_kernel<false>;
  if (lds_b > 64 * 1024 && hipFuncSetAttribute((const void*)bwd,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b) != hipSuccess)
    return pbn::set_error(PBN_EDEVICE, "hipFuncSetAttribute failed");
  hipLaunchKernelGGL(bwd, dim3(tiles), dim3(kThreads), lds_b, s, a);
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "learn_bwd_kernel launch failed");
  const dim3 grid(apply_blocks(N, a.H, a.Apad / 16) + (a.adv_on ? 1 : 0)), blk(64 * kApplyWaves);
  switch (bil_col_tiles(N)) {
    case 1: hipLaunchKernelGGL(learn_apply_kernel<1>, grid, blk, 0, s, a); break;
    case 2: hipLaunchKernelGGL(learn_apply_kernel<2>, grid, blk, 0, s, a); break;
    case 3: hipLaunchKernelGGL(learn_apply_kernel<3>, grid, blk, 0, s, a); break;
    case 4: hipLaunchKernelGGL(learn_apply_kernel<4>, grid, blk, 0, s, a); break;
    case 5: hipLaunchKernelGGL(learn_apply_kernel<5>, grid, blk, 0, s, a); break;
    case 6: hipLaunchKernelGGL(learn_apply_kernel<6>, grid, blk, 0, s, a); break;
    case 7: hipLaunchKernelGGL(learn_apply_kernel<7>, grid, blk, 0, s, a); break;
    default: hipLaunchKernelGGL(learn_apply_kernel<8>, grid, blk, 0, s, a); break;
  }
  if (hipGetLastError() != hipSuccess) return pbn::set_error(PBN_EDEVICE, "learn_apply_kernel launch failed");
  return PBN_OK;
}

}  // namespace

extern "C" {

int pbn_bdq_learn(const pbn_net* net, int64_t batch, const int64_t* d_idx, int64_t capacity, const uint32_t* d_state,
                  const uint32_t* d_next_state, const uint8_t* d_target, const int32_t* d_action, int32_t n_branches,
                  const float* d_reward, const uint8_t* d_done, float* d_params, float* d_Tq,
                  const float* d_target_params, const float* d_target_Tq, float* d_adam_m, float* d_adam_v,
                  float* d_adam_step, float lr, float beta1, float beta2, float eps, float gamma, float grad_clamp,
                  float slope, void* d_workspace, int64_t workspace_bytes, float* d_loss, float* d_grad,
                  const pbn_frame_advance* advance, void* stream) {
  return learn_launch(false, net, batch, d_idx, capacity, d_state, d_next_state, d_target, d_action, n_branches,
                      d_reward, d_done, d_params, d_Tq, d_target_params, d_target_Tq, d_adam_m, d_adam_v, d_adam_step,
                      lr, beta1, beta2, eps, gamma, grad_clamp, slope, d_workspace, workspace_bytes, d_loss, d_grad,
                      nullptr, 0.f, nullptr, advance, stream);
}

int pbn_bdq_learn_per(const pbn_net* net, int64_t batch, const int64_t* d_idx, int64_t capacity,
                      const uint32_t* d_state, const uint32_t* d_next_state, const uint8_t* d_target,
                      const int32_t* d_action, int32_t n_branches, const float* d_reward, const uint8_t* d_done,
                      float* d_params, float* d_Tq, const float* d_target_params, const float* d_target_Tq,
                      float* d_adam_m, float* d_adam_v, float* d_adam_step, float lr, float beta1, float beta2,
                      float eps, float gamma, float grad_clamp, float slope, void* d_workspace, int64_t workspace_bytes,
                      float* d_loss, float* d_grad, const float* d_weights, float replay_constant, float* d_priority,
                      const pbn_frame_advance* advance, void* stream) {
  return learn_launch(true, net, batch, d_idx, capacity, d_state, d_next_state, d_target, d_action, n_branches,
                      d_reward, d_done, d_params, d_Tq, d_target_params, d_target_Tq, d_adam_m, d_adam_v, d_adam_step,
                      lr, beta1, beta2, eps, gamma, grad_clamp, slope, d_workspace, workspace_bytes, d_loss, d_grad,
                      d_weights, replay_constant, d_priority, advance, stream);
}

}  // extern "C"
