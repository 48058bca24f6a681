// Stand-alone host check of csrc/philox.h's philox_prefix / philox_tail (no GPU, no Python): reads
// lines "c0 c1 c2 c3 k0 k1" (hex) from stdin and prints, per line, for R = 7 and R = 10 and for
// XM = 0 and XM = kXM: philox_tail<R, XM>(philox_prefix<R>(c0, c2, c3)) at c1, then
// philox<R, XM> of the same counter and key (8 groups of 4 hex words), then the prefix's words
// A B D E d3 for R = 7 and for R = 10 (10 hex words).  tests/test_philox_prefix.py compiles it
// (host side only) and compares the words.
#include <cstdio>

#include "philox.h"

constexpr uint32_t kXM = 0x80008000u;

template <int R, uint32_t XM>
static pbn::PhiloxPrefix both(const unsigned (&v)[6]) {
  uint32_t rk0[R], rk1[R];
  pbn::philox_round_keys<R>(v[4], v[5], rk0, rk1);
  const pbn::PhiloxPrefix pre = pbn::philox_prefix<R>(v[0], v[2], v[3], rk0, rk1);
  const pbn::Word4 a = pbn::philox_tail<R, XM>(pre, v[1], rk0, rk1);
  const pbn::Word4 b = pbn::philox<R, XM>(v[0], v[1], v[2], v[3], v[4], v[5]);
  std::printf("%08x %08x %08x %08x %08x %08x %08x %08x ", a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
  return pre;
}

int main() {
  unsigned v[6];
  while (std::scanf("%x %x %x %x %x %x", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
    const pbn::PhiloxPrefix p7 = both<7, 0u>(v);
    both<7, kXM>(v);
    const pbn::PhiloxPrefix p10 = both<10, 0u>(v);
    both<10, kXM>(v);
    std::printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", p7.A, p7.B, p7.D, p7.E, p7.d3, p10.A, p10.B,
                p10.D, p10.E, p10.d3);
  }
  return 0;
}
