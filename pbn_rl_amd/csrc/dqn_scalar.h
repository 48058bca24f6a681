// dqn_scalar.h -- the scalar laws of the DDQN kernels (dqn_forward.h, pbn_ddqn.hip), stated once for
// the device and for a host program (tests/dqn_scalar_check.cpp) that holds them to PyTorch: the
// ReLU, the Huber loss and its derivative, clip_grad_norm_'s coefficient and Adam's first step on one
// element bit for bit, Adam's later steps within tests/adam_reference.py's bounds (torch orders the
// sums of m and v differently once they are not zero).  Each keeps a NaN and treats an infinity as
// PyTorch does (DESIGN.md "Non-finite values"): fmaxf / fminf return their other operand for a NaN,
// so none of these is written with them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pbn {

// F.relu: x < 0 -> 0, anything else unchanged: NaN and -0.0 pass, -inf gives 0
__host__ __device__ __forceinline__ float relu(float x) { return x < 0.f ? 0.f : x; }

// F.huber_loss at delta = 1 of the TD error d: d^2 / 2 inside (-1, 1), |d| - 1/2 outside; NaN -> NaN
__host__ __device__ __forceinline__ float huber(float d) {
  const float ad = fabsf(d);
  return ad < 1.f ? 0.5f * d * d : ad - 0.5f;
}

// its derivative (huber_loss's backward): -1 below -1, 1 above 1, else d itself, so a NaN stays
__host__ __device__ __forceinline__ float huber_grad(float d) { return d < -1.f ? -1.f : (d > 1.f ? 1.f : d); }

// clip_grad_norm_: coef = max_norm / (total + 1e-6) as PyTorch evaluates a scalar over a tensor
// (the reciprocal times the scalar), then torch.clamp(max = 1): a NaN norm gives a NaN coefficient
__host__ __device__ __forceinline__ float clip_coef(float total, float max_norm) {
  const float c = (1.f / (total + 1e-6f)) * max_norm;
  return c > 1.f ? 1.f : c;
}

// torch.optim.Adam on one element: bc1 = 1 - b1^t, bc2s = sqrt(1 - b2^t)
struct AdamElement {
  float p, m, v;
};
__host__ __device__ __forceinline__ AdamElement adam_element(float p, float m, float v, float g, float lr, float b1,
                                                             float b2, float eps, float bc1, float bc2s) {
  const float mm = b1 * m + (1.f - b1) * g;
  const float vv = b2 * v + (1.f - b2) * g * g;
  const float denom = sqrtf(vv) / bc2s + eps;
  return AdamElement{p - (lr / bc1) * mm / denom, mm, vv};
}

}  // namespace pbn
