// neo_lbfgs_dir.hpp -- the L-BFGS search direction d = -H g from the stored (s, y) pairs, shared by both forms of the
// run (neo_lbfgs.hpp, neo_lbfgs_sm.hpp): the two-loop recursion (Nocedal 1980) with H0 = I / theta.  2*col dot
// products, each depending on the one before -- on the GPU 2*col dependent LDS reads + wavefront reductions per
// iteration.  This is the form pinned to SciPy's iterates (tests/test_lbfgs_host.py).
//
// (A compact-representation variant -- Byrd, Nocedal, Schnabel 1994: 2*col independent dot products + O(col^2) scalar
//  work -- was built and measured in round 2: 24.3 us per evaluation against 21.7 us at cfg2, slower on the MI355X.  It
//  was a build option until round 3 and is gone from the tree; DESIGN.md section 5 keeps the numbers.)
#pragma once
#include <type_traits>

namespace neo {

// a backend may bring its own form of the recursion (`static constexpr bool kOwnDirection = true` and
// `direction(g, d, col, head, m, theta)`): the all-fp32 device backend walks the pairs two at a time (neo_kernels.hpp)
template <class Backend, class = void>
struct has_own_direction { static constexpr bool value = false; };
template <class Backend>
struct has_own_direction<Backend, std::enable_if_t<Backend::kOwnDirection>> { static constexpr bool value = true; };

// ---- the paired recursion of the all-fp32 device backend (DevBackend::direction, neo_kernels.hpp) for a memory of exactly
// COL pairs, written out step by step at compile time (Plan::hist_ahead: the form the fixed-plan kernels take once the
// memory is full, col = m, which is where a run spends its iterations).  The control flow alone, host and device, with the
// backend's work behind a visitor: tests/test_hist_schedule_cpu.py walks every COL in 1 .. 10 and every head with a visitor
// that keeps books, DevBackend::direction_full with the one that computes (COL = m).
// Loop 1 takes the pairs (k, k - 1) for k = COL - 1, COL - 3, ... and, for odd COL, ends on the single pair 0; then q is
// scaled by 1 / theta; loop 2 takes (k, k + 1) for k = 0, 2, ... and, for odd COL, ends on the single pair COL - 1.  Pair
// k lives in slot (head + k) mod m.  With every k a constant, every pair has registers of its own: a pair is read from
// LDS ONCE, one step ahead of its use in loop 1, with no condition around any read, and loop 2 finds all of them where
// loop 1 left them.
//   V: template <int K> void read(int slot)                          issue the reads of pair K
//      template <int KA, int KB> void pair1(int slotA, int slotB)    a loop 1 step on the pairs KA, KB (slots: the scalars)
//      template <int KA, int KB> void pair2(int slotA, int slotB)    a loop 2 step
//      template <int K> void single1(int slot), single2(int slot)    the single-pair steps
//      void seam()                                                   q /= theta
NEO_HD int hist_slot(int head, int k, int m) { return head + k < m ? head + k : head + k - m; }

// ---- where the pairs live (every device backend; tests/test_hist_layout_cpu.py).  The region holds 2 m n elements.  fp32
// pairs: the m pairs one after the other, and within a pair element e of s next to element e of y -- the two-element record (s_e, y_e).
// A lane that holds element e of a FLAT slot fetches both with ONE access of twice the width, and the records of the FLAT
// slots of a pair lie a compile-time distance apart (64 records): one address a pair.
NEO_HD int hist_record(int slot, int e, int n) { return slot * n + e; }                                    // in records
NEO_HD int hist_index(int slot, int e, int n, int which) { return hist_record(slot, e, n) * 2 + which; }  // which: 0 s, 1 y
// fp64 pairs: the m rows of s, then the m rows of y (a 16-byte record is one read into four consecutive registers, which the
// register-bound members that store fp64 pairs paid in spills and time: DevBackend::kRecords)
NEO_HD int hist_index_rows(int slot, int e, int n, int m, int which) { return (which * m + slot) * n + e; }
// The written-out recursion (hist_walk_full below, DevBackend::DirFull) reads the partly filled last FLAT slot without a
// condition: a lane beyond n reads the records that follow, and behind the last pair that is memory behind the region --
// so many elements of it (`lanes` = 64 * FLAT slots).  The launcher admits the form only where they lie inside the launch's
// own dynamic LDS (neo_launch_opt.hpp); the values are replaced by zeros before any use.
NEO_HD int hist_over_read_elems(int n, int lanes) { return (lanes - n) * 2; }
template <int K, class V>
NEO_HD void hist_full_read1(int head, int m, V &v) {  // the pairs of the loop 1 step whose pair A is K (none: K < 0)
  if constexpr (K >= 0) v.template read<K>(hist_slot(head, K, m));
  if constexpr (K >= 1) v.template read<K - 1>(hist_slot(head, K - 1, m));
}
template <int K, class V>
NEO_HD void hist_full_loop1(int head, int m, V &v) {
  if constexpr (K >= 0) hist_full_read1<K - 2>(head, m, v);
  if constexpr (K >= 1) {
    v.template pair1<K, K - 1>(hist_slot(head, K, m), hist_slot(head, K - 1, m));
    hist_full_loop1<K - 2>(head, m, v);
  } else if constexpr (K == 0) {
    v.template single1<0>(hist_slot(head, 0, m));
  }
}
template <int COL, int K, class V>
NEO_HD void hist_full_loop2(int head, int m, V &v) {
  if constexpr (K + 1 < COL) {
    v.template pair2<K, K + 1>(hist_slot(head, K, m), hist_slot(head, K + 1, m));
    hist_full_loop2<COL, K + 2>(head, m, v);
  } else if constexpr (K < COL) {
    v.template single2<K>(hist_slot(head, K, m));
  }
}
template <int COL, class V>
NEO_HD void hist_walk_full(int head, int m, V &v) {
  static_assert(COL >= 1, "at least one pair");
  hist_full_read1<COL - 1>(head, m, v);
  hist_full_loop1<COL - 1>(head, m, v);
  v.seam();
  hist_full_loop2<COL, 0>(head, m, v);
}

// d = -H g.  `scratch` vectors are the caller's (tmp, tmp2 of the run).
template <class Backend>
NEO_HD void lbfgs_direction(Backend &be, const typename Backend::Vec &g, typename Backend::Vec &d,
                            typename Backend::Vec &tmp, typename Backend::Vec &tmp2, int col, int head, int m,
                            double theta) {
  if constexpr (has_own_direction<Backend>::value) {
    be.direction(g, d, col, head, m, theta);
    return;
  }
  if (col == 0) {
    be.neg(d, g);
    return;
  }
  be.copy(d, g);  // d plays q of the two-loop recursion
  for (int k = col - 1; k >= 0; --k) {
    const int slot = head + k < m ? head + k : head + k - m;  // (head + k) % m without the division
    be.hist_get_sy(slot, tmp, tmp2);  // (y issued with the read of s: its latency hides behind the reduction)
    const double a = be.rho_dot(slot, tmp, d);  // rho * s'q
    be.sput(m + slot, a);
    be.axpy(-a, tmp2, d);
  }
  be.scale(d, 1.0 / theta);
  for (int k = 0; k < col; ++k) {
    const int slot = head + k < m ? head + k : head + k - m;
    be.hist_get_sy(slot, tmp2, tmp);
    const double b = be.rho_dot(slot, tmp, d);
    be.axpy(be.sdiff(m + slot, b), tmp2, d);
  }
  be.scale(d, -1.0);
}

}  // namespace neo
