// gbdq_front.h -- the one statement of pbn_gbdq_front's image layout and LDS carving (pbn_gbdq.hip;
// host and device read the same struct).  N = the net's nodes (1..128).
//
// Image (floats; every segment starts at a multiple of 16 floats):
//   m1        [16][N]       layer 1's message table, row = s_i | t_i << 1 | s_j << 2 | t_j << 3
//   bn        [3][2][N]     BatchNorm weight and bias of bn1, bn2, bn3
//   layer 2, then layer 3:
//     wu      [Kp][128]     k-major: column c < 64 = (A - Bm)[c][k], column 64 + c = Bm[c][k], where the
//                           conv model's first Linear is [A | Bm] (x_i and x_j - x_i halves); rows k >= N zero
//     b1      [64]
//     w2t     [64][Np]      the second Linear transposed, [c][o]; columns o >= N zero
//     b2      [N]
//   csr_start int32 [N + 1], csr_src int32 [E]   the edge list by target node (last: E is only there)
// Np = N rounded up to 16 (MFMA tile rows / columns), Kp = N rounded up to 4 (MFMA k-steps).
//
// LDS of one block (floats), one env at a time:
//   act   [Np][NS]   the (N, N) activations between layers; NS >= Kp, NS % 32 == 4 (an MFMA A read
//                    takes 16 rows x 4 consecutive k: row stride 4 mod 32 spreads them over the banks);
//                    rows >= N and columns >= N stay zero: padding contributes exact zeros
//   u     [Np][68]   u_i = (A - Bm) a_i + b1, then in place S_i = sum_e relu(u_i + v_j)
//   v     [Np][68]   v_j = Bm a_j
//   m1    [16][N]    the table, staged once per block
//   code  int [N]    s_i | t_i << 1 of the env
#pragma once
#include <stdint.h>

namespace pbn {

constexpr int kGbdqHidden = 64;      // the conv models' hidden width
constexpr int kGbdqUS = 68;          // row stride of u and v
constexpr int kGbdqThreads = 256;    // four waves
constexpr int kGbdqMaxLds = 160 * 1024;

struct GbdqLayout {
  int N, Np, Kp, NS;
  int64_t m1, bn, wu[2], b1[2], w2t[2], b2[2], csr_start, csr_src;   // float offsets into the image
  int64_t lds_act, lds_u, lds_v, lds_m1, lds_code, lds_floats;       // float offsets into LDS
};

__host__ __device__ inline int64_t gbdq_al16(int64_t x) { return (x + 15) & ~int64_t(15); }

// the number of image floats is csr_src + al16(E)
__host__ __device__ inline GbdqLayout gbdq_layout(int N) {
  GbdqLayout L;
  L.N = N;
  L.Np = (N + 15) & ~15;
  L.Kp = (N + 3) & ~3;
  L.NS = L.Kp + ((4 - L.Kp % 32) + 32) % 32;
  int64_t o = 0;
  L.m1 = o, o += gbdq_al16(16 * (int64_t)N);
  L.bn = o, o += gbdq_al16(6 * (int64_t)N);
  for (int l = 0; l < 2; ++l) {
    L.wu[l] = o, o += gbdq_al16((int64_t)L.Kp * 2 * kGbdqHidden);
    L.b1[l] = o, o += kGbdqHidden;
    L.w2t[l] = o, o += gbdq_al16((int64_t)kGbdqHidden * L.Np);
    L.b2[l] = o, o += gbdq_al16(N);
  }
  L.csr_start = o, o += gbdq_al16(N + 1);
  L.csr_src = o;
  int64_t s = 0;
  L.lds_act = s, s += (int64_t)L.Np * L.NS;
  L.lds_u = s, s += (int64_t)L.Np * kGbdqUS;
  L.lds_v = s, s += (int64_t)L.Np * kGbdqUS;
  L.lds_m1 = s, s += gbdq_al16(16 * (int64_t)N);
  L.lds_code = s, s += gbdq_al16(N);
  L.lds_floats = s;
  return L;
}

// float offsets of d_conv's segments (pbn_gbdq_pack): layer l = 0, 1, 2
struct GbdqConv {
  int64_t w1[3], b1[3], w2[3], b2[3], bn;
};

__host__ __device__ inline GbdqConv gbdq_conv(int N) {
  GbdqConv C;
  int64_t o = 0;
  for (int l = 0; l < 3; ++l) {
    const int in = l == 0 ? 4 : 2 * N;
    C.w1[l] = o, o += (int64_t)kGbdqHidden * in;
    C.b1[l] = o, o += kGbdqHidden;
    C.w2[l] = o, o += (int64_t)N * kGbdqHidden;
    C.b2[l] = o, o += N;
  }
  C.bn = o;
  return C;
}

}  // namespace pbn
