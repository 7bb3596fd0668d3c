// track_host.cpp -- the route model of csrc/neo_track.hpp compiled by the host compiler (-ffp-contract=off), for
// tests/test_track_cpu.py: one line of stdin is one call, one line of stdout its result as hexadecimal bit patterns.
//
//   R n closed speed x0 y0 x1 y1 ...   sets the route (n vertices; speed and coordinates as 64-bit patterns)
//                                      -> cum_0 .. cum_segments (route_cum)
//   T t                                the route's point at time t (a 64-bit pattern)
//                                      -> x y of route_point, then x y of route_point_cum
//
// Numbers are read with strtoull, base 0 (decimal or 0x...).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "neo_track.hpp"

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
  std::vector<char> line(32768);
  std::vector<double> v, cum;
  int n = 0, closed = 0;
  double speed = 0.0;
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
    if (op == 'R') {
      if (a.size() < 3 || a[0] < 2 || a[0] > (unsigned long long)neo::kRouteMax || a.size() != 3 + 2 * a[0]) {
        std::fprintf(stderr, "R takes n, closed, speed and 2 n coordinates, 2 <= n <= %d\n", neo::kRouteMax);
        return 2;
      }
      n = (int)a[0];
      closed = a[1] != 0;
      speed = from_bits(a[2]);
      v.resize(2 * (size_t)n);
      for (size_t i = 0; i < v.size(); ++i) v[i] = from_bits(a[3 + i]);
      const int nseg = neo::route_segments(n, closed);
      cum.assign((size_t)nseg + 1, 0.0);
      neo::route_cum(v.data(), n, closed, cum.data());
      for (int k = 0; k <= nseg; ++k) std::printf(k ? " %016llx" : "%016llx", bits(cum[k]));
      std::printf("\n");
    } else if (op == 'T') {
      if (n < 2 || a.size() != 1) {
        std::fprintf(stderr, "T takes one time, after a route\n");
        return 2;
      }
      double o1[2], o2[2];
      neo::route_point(v.data(), n, closed, speed, from_bits(a[0]), o1);
      neo::route_point_cum(v.data(), cum.data(), n, closed, speed, from_bits(a[0]), o2);
      std::printf("%016llx %016llx %016llx %016llx\n", bits(o1[0]), bits(o1[1]), bits(o2[0]), bits(o2[1]));
    } else {
      std::fprintf(stderr, "unknown operation '%c'\n", op);
      return 2;
    }
  }
  return 0;
}
