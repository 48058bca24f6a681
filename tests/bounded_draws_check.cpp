// Stand-alone host check of the bounded draws in csrc/step_law.h (no GPU, no Python): the action
// digits from two divisions and gap 2's uniform from the running X, as the env loops take them,
// with the magics net_image.h's finish_scalars gives the kernels, against the three-division
// forms they replaced (restated here), against plain integer division, and against hi32(X * x_mult).  One line per check: "<name> <cases> <mismatches>";
// tests/test_bounded_draws_host.py compiles it (host side only) and reads the lines.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "net_image.h"
#include "step_law.h"

namespace {

pbn::NetImage net_of(int N, int A) {
  pbn::NetImage im;
  im.n_nodes = N;
  im.n_attr = A;
  im.n_states = A;
  im.W = (N + 31) / 32;
  im.lq = 1;
  pbn::image::finish_scalars(&im);
  return im;
}

// ---- the forms before: three multiply-highs by ceil(2^32 / (N + 1))
uint32_t old_actions_mask31(uint32_t c, uint32_t n1, uint32_t magic, uint32_t vmask) {
  uint32_t m = 0;
  for (int q = 0; q < 3; ++q) {
    const uint32_t qt = pbn::mulhi32(c, magic);
    m |= 1u << ((c - qt * n1 - 1u) & 31u);
    c = qt;
  }
  return m & vmask;
}
template <int W>
void old_actions_from_draw(uint32_t c, int N, uint32_t magic, uint32_t (&m)[W]) {
  const uint32_t n1 = (uint32_t)(N + 1);
  for (int q = 0; q < 3; ++q) {
    const uint32_t qt = pbn::mulhi32(c, magic);
    const int act = (int)(c - qt * n1);
    c = qt;
    for (int w = 0; w < W; ++w)
      if (act > 0 && ((act - 1) >> 5) == w) m[w] |= 1u << ((act - 1) & 31);
  }
}

void mask31() {
  unsigned long long n = 0, bad = 0;
  for (uint32_t n1 = 2; n1 <= 32; ++n1) {
    const pbn::NetImage im = net_of((int)n1 - 1, 0);
    const uint32_t vmask = pbn::valid_word_mask((int)n1 - 1, 0);
    for (uint32_t c = 0; c < n1 * n1 * n1; ++c, ++n) {
      const uint32_t got = pbn::actions_mask31(c, n1, im.n1_magic, vmask);
      uint32_t want = 0;   // integer division, apart from the old form
      for (uint32_t q = c, k = 0; k < 3; ++k, q /= n1)
        if (q % n1) want |= 1u << (q % n1 - 1);
      bad += got != old_actions_mask31(c, n1, im.n1_magic, vmask) || got != want;
    }
  }
  std::printf("mask31 %llu %llu\n", n, bad);
}

template <int W>
void from_draw_at(int N, uint32_t stride, unsigned long long* n, unsigned long long* bad) {
  const pbn::NetImage im = net_of(N, 0);
  const uint32_t n1 = (uint32_t)N + 1u, top = n1 * n1 * n1;
  auto one = [&](uint32_t c) {
    uint32_t got[W], old[W], want[W];
    for (int w = 0; w < W; ++w) got[w] = old[w] = want[w] = 0;
    pbn::actions_from_draw<W>(c, N, im.n1_magic, got);
    old_actions_from_draw<W>(c, N, im.n1_magic, old);
    for (uint32_t q = c, k = 0; k < 3; ++k, q /= n1)
      if (q % n1) want[(q % n1 - 1) >> 5] |= 1u << ((q % n1 - 1) & 31);
    ++*n;
    *bad += std::memcmp(got, old, sizeof got) != 0 || std::memcmp(got, want, sizeof got) != 0;
  };
  for (uint32_t c = 0; c < top; c += stride) one(c);
  for (uint32_t c = top - n1; c < top; ++c) one(c);
}

void from_draw(uint32_t stride) {
  unsigned long long n = 0, bad = 0;
  const int Ns[5] = {32, 33, 64, 96, 128};
  for (int N : Ns) {
    if (N <= 32) from_draw_at<1>(N, stride, &n, &bad);
    if (N <= 64) from_draw_at<2>(N, stride, &n, &bad);
    if (N <= 96) from_draw_at<3>(N, stride, &n, &bad);
    from_draw_at<4>(N, stride, &n, &bad);
  }
  std::printf("from_draw %llu %llu\n", n, bad);
}

void pairs() {
  unsigned long long n = 0, bad = 0;
  const int As[3] = {2, 3, 255};   // (A - 1 == 1: the no-divide arm; the largest magic; the largest draws)
  for (int Ai : As) {
    const pbn::NetImage im = net_of(7, Ai);
    const uint32_t A = (uint32_t)Ai;
    for (uint32_t c = 0; c < A * (A - 1); ++c, ++n) {
      const uint32_t as = pbn::pair_start(c, im.am1_magic), rt = pbn::pair_target(c, as, A);
      const uint32_t qs = c / (A - 1), r = c % (A - 1);
      bad += as != qs || rt != r + (r >= qs ? 1u : 0u);
      // pair_draw: the smallest X whose draw over the A(A-1) pairs is c, X = ceil(c * 2^64 / K)
      const unsigned __int128 K = (unsigned __int128)A * (A - 1);
      const uint64_t X = (uint64_t)((((unsigned __int128)c << 64) + K - 1) / K);
      uint32_t xh = (uint32_t)(X >> 32), xl = (uint32_t)X, as2, rt2;
      pbn::pair_draw(xh, xl, A, im.am1_magic, as2, rt2);
      bad += as2 != as || rt2 != rt;
    }
  }
  std::printf("pairs %llu %llu\n", n, bad);
}

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// gap 2's uniform: the running X's top word after the action and pair draws, against the one
// product hi32(X * x_mult) the fast loops took off the chain before
void u2() {
  unsigned long long n = 0, bad = 0;
  const int nets[3][2] = {{2, 2}, {29, 14}, {32, 255}};   // (n1, A)
  for (const auto& na : nets) {
    const pbn::NetImage im = net_of(na[0] - 1, na[1]);
    const uint32_t n1 = (uint32_t)na[0], A = (uint32_t)na[1];
    uint64_t seed = 0x5EEDull * n1 + A;
    for (int i = 0; i < 10005; ++i, ++n) {
      const uint64_t edge[5] = {0ull, 1ull, 0xFFFFFFFFull, 1ull << 32, ~0ull};
      const uint64_t X = i < 5 ? edge[i] : splitmix(&seed);
      uint32_t xhi = (uint32_t)(X >> 32), xlo = (uint32_t)X;
      pbn::ext64(xhi, xlo, n1 * n1 * n1);
      pbn::ext64(xhi, xlo, A * (A - 1));
      bad += xhi != (uint32_t)((X * im.x_mult) >> 32);
    }
  }
  std::printf("u2 %llu %llu\n", n, bad);
}

}  // namespace

int main(int argc, char** argv) {
  const uint32_t stride = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
  if (stride == 0) return 2;
  mask31();
  from_draw(stride);
  pairs();
  u2();
  return 0;
}
