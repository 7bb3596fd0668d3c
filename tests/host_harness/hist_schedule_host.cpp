// hist_schedule_host.cpp -- the walk of the all-fp32 backend's paired two-loop recursion over a memory of exactly COL pairs
// (hist_walk_full of csrc/neo_lbfgs_dir.hpp, the control flow DevBackend::direction_full runs on the device for COL = m),
// compiled for the host with a visitor that prints what the walk asks of it, for tests/test_hist_schedule_cpu.py:
//
//     hist_schedule_host            for every COL in 1 .. 10 and head in 0 .. 9 (m = 10) a line "walk COL head", then one
//                                   line an event:  "read K slot"               the reads of pair K issued (from `slot`)
//                                                   "pair1 KA KB slotA slotB"   a pair step of loop 1 (pair2: of loop 2)
//                                                   "single1 K slot"            a single-pair step (single2: of loop 2)
//                                                   "seam"                      q /= theta
#include <cstdio>

#include "neo_lbfgs.hpp"

struct Printer {
  template <int K> void read(int slot) { printf("read %d %d\n", K, slot); }
  template <int KA, int KB> void pair1(int A, int B) { printf("pair1 %d %d %d %d\n", KA, KB, A, B); }
  template <int KA, int KB> void pair2(int A, int B) { printf("pair2 %d %d %d %d\n", KA, KB, A, B); }
  template <int K> void single1(int A) { printf("single1 %d %d\n", K, A); }
  template <int K> void single2(int A) { printf("single2 %d %d\n", K, A); }
  void seam() { printf("seam\n"); }
};

template <int COL>
void walks(int m) {
  Printer p;
  for (int head = 0; head < m; ++head) {
    printf("walk %d %d\n", COL, head);
    neo::hist_walk_full<COL>(head, m, p);
  }
  if constexpr (COL > 1) walks<COL - 1>(m);
}

int main() {
  walks<10>(10);
  return 0;
}
