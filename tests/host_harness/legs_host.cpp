// legs_host.cpp -- the goal model of csrc/neo_legs.hpp compiled by the host compiler (-ffp-contract=off), for
// tests/test_legs_cpu.py: one line of stdin is one call, one line of stdout its result as hexadecimal bit patterns.
//
//   S B n_goals begin_0 .. begin_B x0 y0 x1 y1 ...   sets a table (coordinates as 64-bit patterns) -> B counts (decimal)
//   F legs seed x_even x_odd y_scale y_shift         sets a flap campaign (seed decimal or 0x..., the rest 64-bit patterns)
//                                                    -> "ok"
//   I n id_0 .. id_{n-1}                             the flap's mission ids (none given: the mission's index) -> "ok"
//   G b k                                            goal k of mission b -> "1 x y", or "0" where there is none
//   U id k                                           the flap's uniform of (seed, id, k) -> u
//
// Numbers are read with strtoull, base 0 (decimal or 0x...).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "neo_legs.hpp"

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
  std::vector<char> line(1 << 16);
  std::vector<double> goals;
  std::vector<int> begin, ids;
  neo::LegSequences seq{};
  int B = 0;
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
    if (op == 'S') {
      if (a.size() < 2 || a.size() != 2 + (a[0] + 1) + 2 * a[1]) {
        std::fprintf(stderr, "S takes B, n_goals, B + 1 begins and 2 n_goals coordinates\n");
        return 2;
      }
      B = (int)a[0];
      begin.resize((size_t)B + 1);
      goals.resize(2 * (size_t)a[1]);
      for (int b = 0; b <= B; ++b) begin[b] = (int)(long long)a[2 + b];
      for (size_t i = 0; i < goals.size(); ++i) goals[i] = from_bits(a[3 + B + i]);
      seq = neo::LegSequences{};
      seq.kind = 0;
      seq.goals = goals.data();
      seq.n_goals = (int)a[1];
      seq.seq_begin = begin.data();
      for (int b = 0; b < B; ++b) std::printf(b ? " %d" : "%d", neo::leg_count(seq, b));
      std::printf("\n");
    } else if (op == 'F') {
      if (a.size() != 6) {
        std::fprintf(stderr, "F takes legs, seed, x_even, x_odd, y_scale, y_shift\n");
        return 2;
      }
      seq = neo::LegSequences{};
      seq.kind = 1;
      seq.legs = (int)(long long)a[0];
      seq.seed = a[1];
      seq.x_pair[0] = from_bits(a[2]);
      seq.x_pair[1] = from_bits(a[3]);
      seq.y_scale = from_bits(a[4]);
      seq.y_shift = from_bits(a[5]);
      ids.clear();
      B = 1 << 30;
      std::printf("ok\n");
    } else if (op == 'I') {
      if (a.empty() || a.size() != 1 + a[0]) {
        std::fprintf(stderr, "I takes n and n ids\n");
        return 2;
      }
      ids.resize((size_t)a[0]);
      for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int)a[1 + i];
      seq.mission_ids = ids.data();
      B = (int)ids.size();
      std::printf("ok\n");
    } else if (op == 'G') {
      if (a.size() != 2 || (long long)a[0] < 0 || (long long)a[0] >= B) {
        std::fprintf(stderr, "G takes a mission in 0 .. B - 1 and a leg\n");
        return 2;
      }
      double g[2];
      if (neo::leg_goal(seq, (int)a[0], (int)(long long)a[1], g))
        std::printf("1 %016llx %016llx\n", bits(g[0]), bits(g[1]));
      else
        std::printf("0\n");
    } else if (op == 'U') {
      if (a.size() != 2) {
        std::fprintf(stderr, "U takes an id and a leg\n");
        return 2;
      }
      std::printf("%016llx\n", bits(neo::leg_flap_uniform(seq.seed, (uint32_t)a[0], (uint32_t)a[1])));
    } else {
      std::fprintf(stderr, "unknown operation '%c'\n", op);
      return 2;
    }
  }
  return 0;
}
