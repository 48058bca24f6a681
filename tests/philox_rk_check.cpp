// Stand-alone host check of csrc/philox.h's philox_rk (no GPU, no Python): reads lines
// "c0 c1 c2 c3 k0 k1" (hex) from stdin and prints, per line, philox_rk<7>, philox<7>,
// philox_rk<10> and philox<10> of that counter and key (16 hex words), the _rk forms with the
// round keys of philox_round_keys.  tests/test_philox_round_keys.py compiles it (host side only)
// and compares the words with each other, with the C oracle and with the known answers.
#include <cstdio>

#include "philox.h"

template <int R>
static void both(const unsigned (&v)[6]) {
  uint32_t rk0[R], rk1[R];
  pbn::philox_round_keys<R>(v[4], v[5], rk0, rk1);
  const pbn::Word4 a = pbn::philox_rk<R>(v[0], v[1], v[2], v[3], rk0, rk1);
  const pbn::Word4 b = pbn::philox<R>(v[0], v[1], v[2], v[3], v[4], v[5]);
  std::printf("%08x %08x %08x %08x %08x %08x %08x %08x ", a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}

int main() {
  unsigned v[6];
  while (std::scanf("%x %x %x %x %x %x", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
    both<7>(v);
    both<10>(v);
    std::printf("\n");
  }
  return 0;
}
