// opt_plan_host.cpp -- the dynamic LDS of an all-fp32 optimize_kernel launch and the launcher's decision whether it may
// run the fixed plan (opt_lds_plan and opt_plan_fixed of csrc/neo_launch_opt.hpp), for tests/test_hist_layout_cpu.py.  Host
// code of a HIP header: compiled with hipcc for the host alone (no kernel is instantiated, nothing is launched).
//
//     opt_plan_host                 for D = 2, 3 and every M the members with a fixed plan serve (lane = (piece,
//                                   dimension): D M <= 64; one or two FLAT slots), without and with the velocity stash:
//                                   "D M NS stash stage pcr_off dyn over_read_elems fixed"
#include <cstdio>

#include "neo_launch_opt.hpp"

namespace neo {

template <int D, int NS>
void line(int M, int stash) {
  using LG = WaveLanesPD<D>;
  static_assert(!opt_plan_t<NS, LG, float, false>::dynamic, "a member with a fixed plan");
  const OptLds l = opt_lds_plan<D, NS, float, 2, LG, float>(M, 0, stash);
  const int n = D * (M - 1) + M;
  printf("%d %d %d %d %d %d %zu %d %d\n", D, M, NS, stash, l.stage, l.pcr_off, l.dyn, hist_over_read_elems(n, NS * kWave),
         (int)opt_plan_fixed<D, NS, LG, float>(l, M, stash, true));
}

template <int D>
void shapes() {
  for (int M = 1; lane_piece_dim(D, M, 0); ++M)
    for (int stash : {0, velocity_stash_bytes(D)})
      switch (slots_for(M, D)) {
        case 1: line<D, 1>(M, stash); break;
        case 2: line<D, 2>(M, stash); break;
        default: break;  // (three FLAT slots and more: lane = piece, no fixed plan)
      }
}

}  // namespace neo

int main() {
  neo::shapes<2>();
  neo::shapes<3>();
  return 0;
}
