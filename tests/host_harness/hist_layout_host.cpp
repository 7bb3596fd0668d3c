// hist_layout_host.cpp -- where the optimiser kernels keep their L-BFGS pairs (hist_index, hist_index_rows of
// csrc/neo_lbfgs_dir.hpp, the one place every device backend takes its LDS positions from), compiled for the host for
// tests/test_hist_layout_cpu.py:
//
//     hist_layout_host M N_MAX      for every n in 1 .. N_MAX a line "n n", then one line a (slot, element):
//                                   "slot e index_of_s index_of_y record rows_index_of_s rows_index_of_y"
//                                   (fp32 pairs: records; fp64 pairs: rows)
#include <cstdio>
#include <cstdlib>

#include "neo_lbfgs.hpp"

int main(int argc, char **argv) {
  const int m = argc > 1 ? atoi(argv[1]) : 10, n_max = argc > 2 ? atoi(argv[2]) : 128;
  for (int n = 1; n <= n_max; ++n) {
    printf("n %d\n", n);
    for (int slot = 0; slot < m; ++slot)
      for (int e = 0; e < n; ++e)
        printf("%d %d %d %d %d %d %d\n", slot, e, neo::hist_index(slot, e, n, 0), neo::hist_index(slot, e, n, 1), neo::hist_record(slot, e, n),
               neo::hist_index_rows(slot, e, n, m, 0), neo::hist_index_rows(slot, e, n, m, 1));
  }
  return 0;
}
