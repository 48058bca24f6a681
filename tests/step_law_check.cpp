// Stand-alone host check of csrc/step_law.h (no GPU, no Python): the per-env law's helpers as the
// step kernels call them, driven by commands on stdin, one result line per command.
// tests/test_step_law_host.py compiles it (host side only) and compares the lines with
// oracle/pyoracle.py.  The magics are net_image.h's (finish_scalars), as the kernels get them.
//   div                         the magic divides, exhaustively (the loops are here, not in Python)
//   net N A first[0..A]         the net of the commands below (A = 0: no attractors, no table)
//   cdf c[0..N)                 its perturbation CDF
//   draw xhi xlo                the ENV draws from X: c_act, as, rt, row, X's top word afterwards,
//                               and the top word of X * x_mult (* size)
//   rst c0 c1 c3 k0 k1          the random reset state (4 words) and its target
//   pert k c0 c1 c3 k0 k1       update k's perturbation mask (4 words), gaps drawn, Philox calls of
//                               the tail; k >= 1 also through the tail alone (settle_updates' form)
//   out att target t horizon autoreset pert open    flags, t, term wrong trunc reset, reward slot
#include <cstdio>
#include <cstring>
#include <vector>

#include "net_image.h"
#include "step_law.h"

namespace {

constexpr int W4 = 4;   // state words of the widest network (128 nodes)

pbn::NetImage g_net;
std::vector<int32_t> g_first;
std::vector<uint32_t> g_cdf;

void set_net(int N, int A, int n_states) {
  g_net = pbn::NetImage();
  g_net.n_nodes = N;
  g_net.n_attr = A;
  g_net.n_states = n_states;
  g_net.W = (N + 31) / 32;
  g_net.lq = 1;
  pbn::image::finish_scalars(&g_net);
}

// oracle/pbn_oracle.c gap_of: min{m in 1..N : u < C[m-1]}, N + 1 if none
int gap_of(uint32_t u) {
  const int N = (int)g_cdf.size();
  for (int m = 1; m <= N; ++m)
    if (u < g_cdf[m - 1]) return m;
  return N + 1;
}

// the ENV call's draws from X = (xhi:xlo) in the kernels' order; returns X's top word afterwards
struct EnvDraws {
  uint32_t c_act, as, rt, row, top, xr_top;
};
EnvDraws env_draws(uint32_t xhi, uint32_t xlo) {
  EnvDraws d{};
  const uint32_t n1 = (uint32_t)g_net.n_nodes + 1u;
  uint64_t xr = (((uint64_t)xhi << 32) | xlo) * g_net.x_mult;
  d.c_act = pbn::ext64(xhi, xlo, n1 * n1 * n1);
  if (g_net.n_attr >= 1) {
    pbn::pair_draw(xhi, xlo, (uint32_t)g_net.n_attr, g_net.am1_magic, d.as, d.rt);
    d.row = pbn::start_pick(xhi, xlo, d.as, g_net.att_single != 0, [](uint32_t i) { return g_first[i]; }, xr);
  }
  d.top = xhi;
  d.xr_top = (uint32_t)(xr >> 32);
  return d;
}

int divides() {
  unsigned long long n_pair = 0, bad_pair = 0, n_act = 0, bad_act = 0, n_m31 = 0, bad_m31 = 0;
  for (int A = 2; A <= 255; ++A) {
    set_net(7, A, A);
    for (uint32_t c = 0; c < (uint32_t)A * (uint32_t)(A - 1); ++c, ++n_pair) {
      const uint32_t as = pbn::pair_start(c, g_net.am1_magic), rt = pbn::pair_target(c, as, (uint32_t)A);
      const uint32_t qs = c / (uint32_t)(A - 1), r = c % (uint32_t)(A - 1);
      if (as != qs || rt != r + (r >= qs ? 1u : 0u)) ++bad_pair;
    }
  }
  const int Ns[8] = {1, 7, 28, 31, 32, 70, 127, 128};
  for (int N : Ns) {
    set_net(N, 0, 0);
    const uint32_t n1 = (uint32_t)N + 1u;
    for (uint32_t c = 0; c < n1 * n1 * n1; ++c, ++n_act) {
      uint32_t m[W4] = {0, 0, 0, 0}, want[W4] = {0, 0, 0, 0};
      pbn::actions_from_draw<W4>(c, N, g_net.n1_magic, m);
      uint32_t q = c;
      for (int k = 0; k < 3; ++k) {
        const uint32_t act = q % n1;
        q /= n1;
        if (act > 0) want[(act - 1) >> 5] |= 1u << ((act - 1) & 31);
      }
      if (std::memcmp(m, want, sizeof m) != 0) ++bad_act;
      if (N <= 31) {
        uint32_t m1[1] = {0};
        pbn::actions_from_draw<1>(c, N, g_net.n1_magic, m1);
        ++n_m31;
        if (pbn::actions_mask31(c, n1, g_net.n1_magic, pbn::valid_word_mask(N, 0)) != m1[0] || m1[0] != want[0])
          ++bad_m31;
      }
    }
  }
  std::printf("div %llu %llu %llu %llu %llu %llu\n", n_pair, bad_pair, n_act, bad_act, n_m31, bad_m31);
  return 0;
}

void pert(uint32_t k, uint32_t c0, uint32_t c1, uint32_t c3, uint32_t k0, uint32_t k1) {
  const int N = g_net.n_nodes;
  const uint32_t c2 = k == 0 ? (pbn::kStreamEnv << 28) : ((pbn::kStreamSettleEnv << 28) | ((k - 1) << 8));
  const pbn::Word4 E = pbn::philox(c0, c1, c2, c3, k0, k1);
  const uint32_t u2 = k == 0 ? env_draws(E.w, E.z).top : E.z;
  int n_gaps = 3, n_calls = 0;
  auto call = [&](int jj) {
    ++n_calls;
    return pbn::philox(c0, c1, pbn::gap_call_c2(k, jj), c3, k0, k1);
  };
  auto gap = [&](uint32_t u) {
    ++n_gaps;
    return gap_of(u);
  };
  uint32_t gam[W4] = {0, 0, 0, 0};
  const int g0 = gap_of(E.x), g1 = gap_of(E.y), g2 = gap_of(u2);
  const int p2 = pbn::first_gaps_mask<W4>(g0, g1, g2, N, gam);
  int same31 = 1;   // the one-word form of the first three gaps (N <= 31)
  if (N <= 31) {
    uint32_t g31 = 0;
    same31 = pbn::first_gaps_mask31(g0, g1, g2, pbn::valid_word_mask(N, 0), g31) == p2 && g31 == gam[0];
  }
  if (p2 < N - 1) pbn::gap_tail<W4>(k, 3, p2, N, E, call, gap, gam);
  // updates k >= 1 as settle_updates draws them: every gap through the tail
  uint32_t alone[W4] = {0, 0, 0, 0};
  if (k >= 1) {
    int calls2 = 0;
    pbn::gap_tail<W4>(
        k, 0, -1, N, pbn::Word4{0, 0, 0, 0},
        [&](int jj) {
          ++calls2;
          return pbn::philox(c0, c1, pbn::gap_call_c2(k, jj), c3, k0, k1);
        },
        [&](uint32_t u) { return gap_of(u); }, alone);
  } else {
    std::memcpy(alone, gam, sizeof alone);
  }
  std::printf("pert %08x %08x %08x %08x %d %d %d %d\n", gam[0], gam[1], gam[2], gam[3], n_gaps, n_calls, same31,
              std::memcmp(alone, gam, sizeof gam) == 0 ? 1 : 0);
}

}  // namespace

int main() {
  char cmd[16];
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "div")) {
      divides();
    } else if (!std::strcmp(cmd, "net")) {
      int N, A;
      if (std::scanf("%d %d", &N, &A) != 2) return 2;
      g_first.assign(A >= 1 ? (size_t)A + 1 : 0, 0);
      for (auto& f : g_first)
        if (std::scanf("%d", &f) != 1) return 2;
      set_net(N, A, A >= 1 ? g_first.back() : 0);
      std::printf("net %u %u %llu %d\n", g_net.n1_magic, g_net.am1_magic, (unsigned long long)g_net.x_mult,
                  g_net.att_single);
    } else if (!std::strcmp(cmd, "cdf")) {
      g_cdf.assign((size_t)g_net.n_nodes, 0u);
      for (auto& c : g_cdf)
        if (std::scanf("%u", &c) != 1) return 2;
      std::printf("cdf %zu\n", g_cdf.size());
    } else if (!std::strcmp(cmd, "draw")) {
      uint32_t xhi, xlo;
      if (std::scanf("%u %u", &xhi, &xlo) != 2) return 2;
      const EnvDraws d = env_draws(xhi, xlo);
      std::printf("draw %u %u %u %u %u %u\n", d.c_act, d.as, d.rt, d.row, d.top, d.xr_top);
    } else if (!std::strcmp(cmd, "rst")) {
      uint32_t v[5], s[W4] = {0, 0, 0, 0};
      for (auto& x : v)
        if (std::scanf("%u", &x) != 1) return 2;
      const uint32_t nt = pbn::random_reset_state<W4>(v[0], v[1], v[2], v[3], v[4], g_net.n_nodes, s);
      std::printf("rst %08x %08x %08x %08x %u\n", s[0], s[1], s[2], s[3], nt);
    } else if (!std::strcmp(cmd, "pert")) {
      uint32_t v[6];
      for (auto& x : v)
        if (std::scanf("%u", &x) != 1) return 2;
      pert(v[0], v[1], v[2], v[3], v[4], v[5]);
    } else if (!std::strcmp(cmd, "out")) {
      int att, horizon, autoreset, pt, open;
      uint32_t target, t;
      if (std::scanf("%d %u %u %d %d %d %d", &att, &target, &t, &horizon, &autoreset, &pt, &open) != 7) return 2;
      const pbn::StepOutcome o =
          pbn::step_outcome(att, target, t, horizon, autoreset != 0, pt != 0, open != 0);
      std::printf("out %u %u %d %d %d %d %d\n", o.flags, o.t, (int)o.term, (int)o.wrong, (int)o.trunc, (int)o.reset,
                  pbn::reward_slot(o));
    } else {
      return 2;
    }
  }
  return 0;
}
