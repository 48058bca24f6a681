// Stand-alone host check of the rare fourth-flip tail as pbn_rollout_pipe's env_fast takes it (no
// GPU, no Python): the PERT call's Philox prefix (csrc/philox.h philox_prefix_sibling: its own A,
// E, d3 beside the ENV prefix's B, D) with philox_tail against the whole philox call, and
// csrc/step_law.h's gap_tail_split (the fourth gap in line, the further ones behind a second
// branch, with and without its early no-flip test) against pbn::gap_tail.  One line per check:
// "<name> <cases> <mismatches>"; tests/test_gap_tail_host.py compiles it (host side only, with the
// address and undefined-behaviour sanitizers) and reads the lines.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "philox.h"
#include "step_law.h"

namespace {

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

bool same(const pbn::Word4& a, const pbn::Word4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// the PERT call 0 of a lane from the prefix the loop pins, against the whole call; c1 is the
// step's low word (0 and 0xFFFFFFFF: the launches around the wrap), c3 the high halves
void pert_prefix() {
  unsigned long long n = 0, bad = 0;
  uint64_t seed = 0x9A7A11ull;
  const uint32_t env_c2 = pbn::kStreamEnv << 28, pert_c2 = pbn::kStreamPert << 28;
  for (int i = 0; i < 20000; ++i) {
    const uint64_t a = splitmix(&seed), b = splitmix(&seed), k = splitmix(&seed);
    const uint32_t c0 = i < 2 ? (i ? 0xFFFFFFFFu : 0u) : (uint32_t)a, c3 = i < 4 ? (i & 1 ? 0xFFFFFFFFu : 0u) : (uint32_t)b;
    const uint32_t k0 = (uint32_t)k, k1 = (uint32_t)(k >> 32);
    uint32_t rk0[pbn::kPhiloxRounds], rk1[pbn::kPhiloxRounds];
    pbn::philox_round_keys(k0, k1, rk0, rk1);
    const pbn::PhiloxPrefix env = pbn::philox_prefix(c0, env_c2, c3, rk0, rk1);
    const pbn::PhiloxPrefix own = pbn::philox_prefix(c0, pert_c2, c3, rk0, rk1);
    const pbn::PhiloxPrefix sib = pbn::philox_prefix_sibling(env, c0, pert_c2, c3, rk0, rk1);
    bad += sib.B != own.B || sib.D != own.D || sib.A != own.A || sib.E != own.E || sib.d3 != own.d3;
    const uint32_t c1s[4] = {0u, 0xFFFFFFFFu, (uint32_t)(a >> 32), (uint32_t)(b >> 32)};
    for (uint32_t c1 : c1s) {
      const pbn::Word4 want = pbn::philox(c0, c1, pert_c2, c3, k0, k1);
      bad += !same(pbn::philox_tail(sib, c1, rk0, rk1), want);
      bad += !same(pbn::philox_rk(c0, c1, pert_c2, c3, rk0, rk1), want);
      // the ENV prefix is left as it was
      bad += !same(pbn::philox_tail(env, c1, rk0, rk1), pbn::philox(c0, c1, env_c2, c3, k0, k1));
      ++n;
    }
  }
  std::printf("pert_prefix %llu %llu\n", n, bad);
}

// A word stream whose word is its own gap: call(jj) hands out words 4 * (jj >> 2) .. + 3 and
// records which calls were made
struct Stream {
  std::vector<uint32_t> words;   // a multiple of 4
  std::vector<int> calls;
  pbn::Word4 call(int jj) {
    calls.push_back(jj);
    const size_t c = (size_t)(jj >> 2) * 4;
    return pbn::Word4{words.at(c), words.at(c + 1), words.at(c + 2), words.at(c + 3)};
  }
};

// `landing` gaps of 1 (each lands while a node is left), then gaps past the network
std::vector<uint32_t> words_landing(int landing, int N) {
  std::vector<uint32_t> w(16, (uint32_t)N + 1u);
  for (int i = 0; i < landing; ++i) w[(size_t)i] = 1u;
  return w;
}

void one_split(const std::vector<uint32_t>& words, int p2, int N, unsigned long long* n, unsigned long long* bad,
               unsigned long long* landed_max) {
  auto gap = [](uint32_t u) { return (int)u; };
  Stream a{words, {}}, b{words, {}}, c{words, {}};
  uint32_t want[1] = {0}, got[1] = {0}, got_past[1] = {0};
  const uint32_t before = 0;
  if (p2 < N - 1) {   // the callers' condition
    pbn::gap_tail<1>(0u, 3, p2, N, pbn::Word4{0, 0, 0, 0}, [&](int jj) { return a.call(jj); }, gap, want);
    // the loop's in-line PERT call 0, then the split: without the early test, and with one that
    // is exact here (the word is its gap)
    pbn::gap_tail_split<1>(p2, N, b.call(0), [&](int jj) { return b.call(jj); }, gap, [](uint32_t) { return false; }, got);
    pbn::gap_tail_split<1>(p2, N, c.call(0), [&](int jj) { return c.call(jj); }, gap,
                           [N](uint32_t u) { return u > (uint32_t)N; }, got_past);
  }
  ++*n;
  *bad += got[0] != want[0] || a.calls != b.calls || (got[0] & ~pbn::valid_word_mask(N, 0)) != 0;
  *bad += got_past[0] != want[0] || a.calls != c.calls;
  const unsigned long long landed = (unsigned long long)__builtin_popcount(want[0] & ~before);
  if (landed > *landed_max) *landed_max = landed;
}

void split() {
  unsigned long long n = 0, bad = 0, landed_max = 0, calls2 = 0;
  const int Ns[4] = {7, 10, 28, 31};
  const int landing[5] = {0, 1, 4, 5, 9};
  uint64_t seed = 0x6A9ull;
  for (int N : Ns)
    for (int p2 = -1; p2 <= N - 1; ++p2) {
      for (int l : landing) one_split(words_landing(l, N), p2, N, &n, &bad, &landed_max);
      for (int r = 0; r < 50; ++r) {   // mixed gaps of 1..4, and some past the network
        std::vector<uint32_t> w(16);
        for (auto& x : w) {
          const uint64_t z = splitmix(&seed);
          x = (z & 15) == 0 ? (uint32_t)N + 1u : 1u + (uint32_t)((z >> 8) & 3);
        }
        w.resize(48, 1u);   // (N = 31 from -1 at gaps of 1: 31 words; never run off the stream)
        one_split(w, p2, N, &n, &bad, &landed_max);
      }
    }
  // the cases cross PERT calls 1 and 2: nine landed gaps of 1 read words 0..9
  {
    Stream s{words_landing(9, 28), {}};
    uint32_t g[1] = {0};
    pbn::gap_tail_split<1>(2, 28, s.call(0), [&](int jj) { return s.call(jj); }, [](uint32_t u) { return (int)u; },
                           [](uint32_t u) { return u > 28u; }, g);
    calls2 = s.calls.size() == 3 && s.calls[1] == 4 && s.calls[2] == 8 && g[0] == 0xFF8u ? 1 : 0;
  }
  std::printf("split %llu %llu\n", n, bad);
  std::printf("split_landed_max %llu 0\n", landed_max);
  std::printf("split_calls_1_and_2 %llu 0\n", calls2);
}

}  // namespace

int main() {
  pert_prefix();
  split();
  return 0;
}
