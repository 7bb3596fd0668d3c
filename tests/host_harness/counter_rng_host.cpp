// counter_rng_host.cpp -- csrc/neo_counter_rng.hpp compiled by the host compiler (-ffp-contract=off), for
// tests/test_jitter_cpu.py: one line of stdin is one call, one line of stdout its result as hexadecimal bit patterns.
//
//   B c0 c1 c2 c3 k0 k1          philox4x32_10                        -> four 32-bit words
//   U wa wb                      counter_uniform, counter_probit      -> u, z (64-bit patterns)
//   L bits                       counter_log of the double `bits`     -> 64-bit pattern
//   S seed id a b domain e       counter_normal                       -> 64-bit pattern
//
// Numbers are read with strtoull, base 0 (decimal or 0x...).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "neo_counter_rng.hpp"

int main() {
  std::vector<char> line(512);
  while (std::fgets(line.data(), (int)line.size(), stdin)) {
    char *p = line.data();
    while (*p == ' ') ++p;
    const char op = *p;
    if (op == '\n' || op == '\0') continue;
    ++p;
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    const int want = op == 'B' ? 6 : op == 'U' ? 2 : op == 'L' ? 1 : op == 'S' ? 6 : -1;
    if (want < 0) {
      std::fprintf(stderr, "unknown operation '%c'\n", op);
      return 2;
    }
    for (int i = 0; i < want; ++i) {
      char *end = nullptr;
      v[i] = std::strtoull(p, &end, 0);
      if (end == p) {
        std::fprintf(stderr, "operation '%c' takes %d numbers\n", op, want);
        return 2;
      }
      p = end;
    }
    if (op == 'B') {
      const neo::Philox4 o = neo::philox4x32_10((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3],
                                                (uint32_t)v[4], (uint32_t)v[5]);
      std::printf("%08x %08x %08x %08x\n", o.w[0], o.w[1], o.w[2], o.w[3]);
    } else if (op == 'U') {
      const double u = neo::counter_uniform((uint32_t)v[0], (uint32_t)v[1]);
      std::printf("%016llx %016llx\n", (unsigned long long)neo::counter_bits(u),
                  (unsigned long long)neo::counter_bits(neo::counter_probit(u)));
    } else if (op == 'L') {
      std::printf("%016llx\n", (unsigned long long)neo::counter_bits(neo::counter_log(neo::counter_from_bits((uint64_t)v[0]))));
    } else {
      const double z = neo::counter_normal((uint64_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4],
                                           (uint32_t)v[5]);
      std::printf("%016llx\n", (unsigned long long)neo::counter_bits(z));
    }
  }
  return 0;
}
