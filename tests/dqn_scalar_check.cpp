// Stand-alone host check of csrc/dqn_scalar.h (no GPU, no Python): the DDQN kernels' scalar laws as
// dqn_forward.h and pbn_ddqn.hip call them, driven by commands on stdin, one result line per
// command.  Every float goes in and out as the decimal value of its 32 bits, so NaN, the infinities
// and -0.0 pass unchanged.  tests/test_nonfinite_host.py compiles it (host side only) and compares
// the lines with PyTorch on the CPU.
//   relu x                              relu(x)
//   hub d                               huber(d) huber_grad(d)
//   clip total max_norm                 clip_coef(total, max_norm)
//   adam p m v g lr b1 b2 eps t         p' m' v' of adam_element at step count t (a float), the bias
//                                       corrections as ddqn_adam_kernel takes them
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dqn_scalar.h"

namespace {

float as_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
uint32_t as_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

}  // namespace

int main() {
  char line[512];
  while (fgets(line, (int)sizeof line, stdin)) {
    char cmd[8] = {0};
    int used = 0;
    if (sscanf(line, "%7s%n", cmd, &used) != 1) continue;
    float x[9];
    int n = 0;
    for (char* p = line + used; n < 9; ++n) {
      char* end;
      const unsigned long long u = strtoull(p, &end, 10);
      if (end == p) break;
      x[n] = as_float((uint32_t)u);
      p = end;
    }
    if (!strcmp(cmd, "relu") && n == 1) {
      printf("relu %u\n", as_bits(pbn::relu(x[0])));
    } else if (!strcmp(cmd, "hub") && n == 1) {
      printf("hub %u %u\n", as_bits(pbn::huber(x[0])), as_bits(pbn::huber_grad(x[0])));
    } else if (!strcmp(cmd, "clip") && n == 2) {
      printf("clip %u\n", as_bits(pbn::clip_coef(x[0], x[1])));
    } else if (!strcmp(cmd, "adam") && n == 9) {
      const float b1 = x[5], b2 = x[6], t = x[8];
      const float bc1 = 1.f - powf(b1, t), bc2s = sqrtf(1.f - powf(b2, t));
      const pbn::AdamElement e = pbn::adam_element(x[0], x[1], x[2], x[3], x[4], b1, b2, x[7], bc1, bc2s);
      printf("adam %u %u %u\n", as_bits(e.p), as_bits(e.m), as_bits(e.v));
    } else {
      return 2;
    }
  }
  return 0;
}
