// flight_host.cpp -- the flight model of csrc/neo_flight.hpp compiled by the host compiler (-ffp-contract=off), for
// tests/test_flight_cpu.py: one line of stdin is one call, one line of stdout its result; doubles travel as hexadecimal
// 64-bit patterns, integers as decimals.
//
//   M h kp kv a_max alpha drag rho scale gust_every seed     sets the model -> "ok"
//   F id cap cmd_len cmd_index flown_len step ahead first settle reach gx gy s0 .. s7 rows...
//                                      one launch for one mission: min(cmd_len, cap) command rows of 6 doubles follow
//                                      -> idx fut flown_len saturated cmd_full, the 8 state doubles, the 4 head doubles
//                                         (position and velocity of command row fut), then all cap flown rows (6 doubles
//                                         each; a row the launch did not write holds the canary 0x7ff8dead00000000)
//                                      -> "skip" for a mission with cmd_len < 1 (the kernel leaves it alone)
//
// Numbers are read with strtoull, base 0 (decimal or 0x...).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "neo_flight.hpp"

static double from_bits(unsigned long long b) {
  double x;
  std::memcpy(&x, &b, sizeof x);
  return x;
}
static unsigned long long bits(double x) {
  unsigned long long b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

int main() {
  std::vector<char> line(1 << 20);
  neo::FlightParams m{};
  bool have = false;
  while (std::fgets(line.data(), (int)line.size(), stdin)) {
    char *p = line.data();
    while (*p == ' ') ++p;
    const char op = *p;
    if (op == '\n' || op == '\0') continue;
    ++p;
    std::vector<unsigned long long> a;
    for (;;) {
      char *end = nullptr;
      const unsigned long long x = std::strtoull(p, &end, 0);
      if (end == p) break;
      a.push_back(x);
      p = end;
    }
    if (op == 'M') {
      if (a.size() != 10) {
        std::fprintf(stderr, "M takes 8 doubles, gust_every and the seed\n");
        return 2;
      }
      m = {from_bits(a[0]), from_bits(a[1]), from_bits(a[2]), from_bits(a[3]), from_bits(a[4]), from_bits(a[5]),
           from_bits(a[6]), from_bits(a[7]), (int)a[8], a[9]};
      have = true;
      std::printf("ok\n");
    } else if (op == 'F') {
      if (!have || a.size() < 20) {
        std::fprintf(stderr, "F takes 20 values and the command rows, after a model\n");
        return 2;
      }
      const int cap = (int)a[1], cmd_len = (int)(long long)a[2];
      const int len = cmd_len > cap ? cap : cmd_len;
      if (cap < 1 || a.size() != 20 + 6 * (size_t)(len > 0 ? len : 0)) {
        std::fprintf(stderr, "F: cap >= 1 and min(cmd_len, cap) rows of 6 doubles\n");
        return 2;
      }
      if (len < 1) {
        std::printf("skip\n");
        continue;
      }
      const neo::FlightLaunch l = {cap, (int)a[5], (int)a[6], (int)a[7], (int)a[8], from_bits(a[9])};
      const double goal[2] = {from_bits(a[10]), from_bits(a[11])};
      double s[neo::kFlyState];
      for (int q = 0; q < neo::kFlyState; ++q) s[q] = from_bits(a[12 + q]);
      std::vector<double> rows(6 * (size_t)len), flown(6 * (size_t)cap, from_bits(0x7ff8dead00000000ull));
      for (size_t i = 0; i < rows.size(); ++i) rows[i] = from_bits(a[20 + i]);
      neo::FlightRowsMem at;
      at.rows = rows.data();
      at.last = len - 1;
      const neo::FlightWords w = neo::flight_fly(m, l, (uint32_t)a[0], len, (int)(long long)a[3], (int)(long long)a[4], goal,
                                                 rows.data() + 6 * (size_t)(len - 1), s, flown.data(), at);
      std::printf("%d %d %d %d %d", w.idx, w.fut, w.flown_len, w.saturated, w.cmd_full);
      for (int q = 0; q < neo::kFlyState; ++q) std::printf(" %016llx", bits(s[q]));
      for (int q = 0; q < 4; ++q) std::printf(" %016llx", bits(rows[6 * (size_t)w.fut + q]));
      for (double v : flown) std::printf(" %016llx", bits(v));
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown operation '%c'\n", op);
      return 2;
    }
  }
  return 0;
}
