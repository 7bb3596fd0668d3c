// neo_kernels.hpp -- the fused kernels of libneo_planner_hip.so as templates (gfx950 only); every translation
// unit of the library instantiates the family it dispatches to (neo_disp_*.hip), so that the families compile in parallel.
//
//   eval_kernel      get_cost + get_grad for a batch            (expert_planner.py:539-585)
//   optimize_kernel  plan_once: the whole L-BFGS-B run on-chip  (expert_planner.py:205-237)
//   sample_kernel    add_sampled_cost + add_sampled_grad_CT     (expert_planner.py:392-466)
//
// x0 / x: the start points are read from x0 and the results written to x; the two may be the same buffer (every lane reads
// its own elements before it writes them), which is the in-place form of neo_optimize_batch_dev.
// One 64-lane workgroup (= one wavefront) per trajectory: the optimiser never leaves the chip,
// finished trajectories free their slot for the next ones, no host round trips.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "../../include/neo_planner.h"
#ifndef NEO_FUSED_U
#define NEO_FUSED_U (sizeof(Real) == 4 ? 4 : 2)
#endif
#ifndef NEO_W2_U
// one sample per lane in the blocked sample loop: no VGPR spills.  2: cfg2's all-fp32 member spills 7 registers (32 B of
// scratch) on the current tree and was not timed again; the last timing of the blocked form, with 13 spilled, read 1.437 M
// against 1.513 M traj/s.  What overlaps a round's gathers with arithmetic in that member is the gather-ahead loop
// (neo_device.hpp Plan::gather_ahead), which keeps U = 1: +2.0 %, HISTORY.md
#define NEO_W2_U 1
#endif
#ifndef NEO_W2_OCC
#define NEO_W2_OCC 2  // wavefronts per SIMD the throughput variant is allocated for (experiments: 3)
#endif
#ifndef NEO_X_OCC
// all-fp32 kernels (Num = float) with up to two FLAT slots (n <= 128; four slots -- cfg5 -- spill 167 registers at that
// budget and stay at two per SIMD): allocated for THREE wavefronts per SIMD (168 registers; the cfg2 instantiation
// spills 25 of them, built with -amdgpu-use-amdgpu-trackers: neo_planner_amd/build.py) -- measured 933 k traj/s against
// 889 k at two per SIMD without spills; LDS: fp32 pairs + staging = 12.6 KB of the 13.3 KB a twelfth of a CU has
#define NEO_X_OCC 3
#endif
#include "neo_device.hpp"
#include "neo_lbfgs.hpp"
#include "neo_lbfgs_sm.hpp"

namespace neo {

// the type of the optimiser's scalars and of the line-search state: fp32 where everything else is (Num = float) and the
// run is the state machine (the straight-line form of the four-slot kernels keeps fp64 scalars)
template <typename Num, int NS>
using opt_scalar_t = std::conditional_t<sizeof(Num) == 4 && (NS <= NEO_SM_MAX_SLOTS), float, double>;

// doubles of LDS staging a wavefront needs: NS * 64 for the FLAT <-> PIECE exchange, 64 rows of [D][8] Reals for the
// per-piece fold of the sampled partials (the two uses never overlap)
template <int D, int NS, typename Real>
__host__ __device__ constexpr int stage_doubles() {
  constexpr int fold = sizeof(Real) == 4 ? kWave * 8 * D * (int)sizeof(Real) : 0;  // (fp32 sampling only)
  return (NS * kWave * 8 > fold ? NS * kWave * 8 : fold) / 8;
}

constexpr int kSlCacheInts = kWave / 4 + kWave + 4;  // DevBackend::sl_cache: a key byte and an assignment word a lane, three uniform ints

// ------------------------------------------------------------------ device backend of the optimiser
// SU: samples per lane in flight in the sample loop (minco_sample)
// LG: lane layout of the PIECE-layout phases -- WaveLanes (lane = piece) or WaveLanesPD<D> (lane = (piece, dimension))
// Storage of the L-BFGS pairs.  fp64, except in the two-waves fp32-sampling kernels with four FLAT slots (n > 128,
// cfg5): their 2 * 10 * n doubles (25.8 KB at n = 161) leave room for six wavefronts per CU, in fp32 for eight -- measured
// at cfg5: 119 k traj/s with one wavefront per SIMD, 105 k with two and fp64 pairs, 155 k with two and fp32 pairs,
// mean nfev 336.7 against 337.5 and the same status histogram (the rounding of the pairs is well below what the fp32
// gradient already carries).
template <typename Real, int NS, int WAVES>
__host__ __device__ constexpr bool pairs_in_f32() {
  return sizeof(Real) == 4 && WAVES == 2 && NS > 2;
}
// PAIRS32: the L-BFGS pairs are stored in fp32
// Num: arithmetic of the coefficient solve, the adjoint and the optimiser vectors (double; float = the all-fp32 mode)
// Plan: the launch plan as compile-time constants (neo_device.hpp), or PlanDynamic: the members below decide at run time
template <int D, int NS, typename Real, class MapT, class LookupT, int SU = NEO_FUSED_U, class LG = WaveLanes,
          bool PAIRS32 = false, typename Num = double, class Plan = PlanDynamic>
struct DevBackend {
  static constexpr int DL = LG::dl(D);
  static constexpr int kSlotsN = NS;  // FLAT slots of a Vec
  // joint systems by parallel cyclic reduction in the all-fp32 mode (neo_device.hpp pcr_solve).  Block Thomas wherever the
  // solve is fp64: the parity mode's recorded runs are pinned to its rounding, and in the mixed mode the reduction was
  // measured SLOWER (fp64: 744 k against 778 k traj/s at cfg2, 142 k against 156 k at cfg5 -- five levels of 63 fp64
  // instructions with ~60 live doubles spill where block Thomas does not)
  // (measured again after the spills had gone: in the lane = (piece, dimension) kernel the fp64 reduction fits the
  // registers -- 251 of 256, no spills -- and changes nothing: 774 k traj/s either way)
  static constexpr bool kPcr = sizeof(Num) == 4 && LG::W == kWave;
  // the sample loop runs in its gather-ahead form (minco_sample): a plan's constant, for the lookups that have the form
  static constexpr bool kAhead = !Plan::dynamic && Plan::gather_ahead && LookupT::gather_ahead && SU == 1 && sizeof(Real) == 4;
  // FLAT layout with NS slots: n <= 64 * NS
  struct Vec {
    Num v[NS];
  };
  Traj<D, DL, Num> t;
  const DevParams &prm;
  const MapT &map;
  double *xs;    // LDS [kStage]: FLAT <-> PIECE staging; between scatter_x and the gradient gather the same memory
                 // holds the lane assignment's segment table, the gather-ahead loop's velocity stash and the rows or
                 // accumulators of the per-piece fold, one after the other (minco_sample)
  static constexpr int kStage = stage_doubles<D, NS, Real>();
  // LDS [kSlCacheInts] or nullptr: the lane assignment of the last evaluation (a key byte and a word a lane + three wave-uniform ints).
  // The assignment depends on the pieces' sample counts int(T / delta_t) alone, and along a run 58 % of consecutive
  // iterates have the same counts in every piece (line-search trial points more often still): a hit costs a compare, a
  // ballot and two LDS reads instead of the ~140 vector instructions of balanced_sample_lanes.  Same assignment, same bits.
  int *sl_cache = nullptr;
  bool fold_rows = true;  // xs has all kStage doubles (false: only NS * 64, the fold stays in registers)
  bool fold_acc = false;  // xs holds [M][fold_acc_stride(D)] per-piece accumulators instead of the rows (minco_sample; the kernels that keep
                          // the cyclic reduction's multipliers in LDS: launch_opt)
  // the optimiser's scalars (f, step, g . d, theta) and the line-search state: fp32 in the all-fp32 kernels that run the
  // state machine (round 5: dcsrch / dcstep were ~150 wave-uniform fp64 instructions, eight divisions and a square root
  // among them, on the dependent chain of every evaluation), fp64 otherwise
  using Scalar = opt_scalar_t<Num, NS>;
  LineSearchT<Scalar> *lsp;  // LDS: line-search state (wave-uniform)
  double *cst;      // LDS [12]: cost terms of the last evaluation / current x / previous x
  // LDS: the stored (s, y) pairs of this trajectory -- fp32 pairs [m][n][2], element by element (neo_lbfgs_dir.hpp
  // hist_index), fp64 pairs [2][m][n] (hist_index_rows)
  using Hist = std::conditional_t<PAIRS32, float, double>;
  Hist *hist;
  int npad, m;
  double *coeff_out;  // optional [6M][D] (eval kernel)
  long long samples = 0;  // quadrature samples visited so far (lane-uniform), for the bench's byte count
  int last_ns = 0;        // samples of the last evaluation
  double *trace = nullptr;  // optional [trace_cap][4] of this trajectory: (f, step, samples, iteration) per evaluation
  double *trace_xg = nullptr;  // optional [trace_cap][2][n]: the evaluated point and its gradient
  int trace_cap = 0;

  __device__ DevBackend(const DevParams &p, const MapT &mp) : prm(p), map(mp) {}

  __device__ __forceinline__ double dot(const Vec &a, const Vec &b) const {
    Num s = Num(0);
#pragma unroll
    for (int k = 0; k < NS; ++k) s += a.v[k] * b.v[k];
    return uni((double)wave_sum(s));
  }
  // a wave-uniform scalar back into scalar registers (two v_readfirstlane): the optimiser's scalar state then costs
  // no vector registers
  __device__ __forceinline__ double uni(double v) const { return uniform(v); }
  __device__ __forceinline__ float uni(float v) const { return uniform(v); }
  __device__ __forceinline__ double amax(const Vec &a) const {
    Num s = Num(0);
#pragma unroll
    for (int k = 0; k < NS; ++k) s = fmax(s, fabs(a.v[k]));
    return wave_max_nonneg(s);
  }
  __device__ __forceinline__ void copy(Vec &d, const Vec &s) const {
#pragma unroll
    for (int k = 0; k < NS; ++k) d.v[k] = s.v[k];
  }
  __device__ __forceinline__ void neg(Vec &d, const Vec &s) const {
#pragma unroll
    for (int k = 0; k < NS; ++k) d.v[k] = -s.v[k];
  }
  __device__ __forceinline__ void axpy(double a, const Vec &x, Vec &y) const {
#pragma unroll
    for (int k = 0; k < NS; ++k) y.v[k] += (Num)a * x.v[k];
  }
  __device__ __forceinline__ void lincomb(Vec &o, const Vec &a, double s, const Vec &b) const {
#pragma unroll
    for (int k = 0; k < NS; ++k) o.v[k] = a.v[k] + (Num)s * b.v[k];
  }
  __device__ __forceinline__ void scale(Vec &v, double s) const {
#pragma unroll
    for (int k = 0; k < NS; ++k) v.v[k] *= (Num)s;
  }
  // element k * 64 + lane of a FLAT vector exists.  The kernel with NS slots is launched for kFull * 64 < n <= NS * 64
  // (slots_for: kFull = 0, 1, 2, 2 for NS = 1, 2, 3, 4), so the first kFull slots are full in every lane: no exec masking
  // around their LDS accesses.
  static constexpr int kFull = NS == 3 ? 2 : NS / 2;
  __device__ __forceinline__ bool in_range(int k, int lane) const { return k < kFull || k * kWave + lane < t.n; }
  // fp32 pairs lie in records (s_e, y_e) (neo_lbfgs_dir.hpp hist_index): a lane moves s and y of its element with one
  // 8-byte access.  fp64 pairs keep the rows [2][m][n] (hist_index_rows) and their two 8-byte accesses: a record of doubles is
  // one 16-byte read into four consecutive registers, and the members that have fp64 pairs fill their 256 registers --
  // built and measured, they spilled more and cfg2 ran 0.6 - 0.8 % slower in the f32 and f64 modes (HISTORY.md).
  static constexpr bool kRecords = sizeof(Hist) == 4;
  typedef Hist HistPair __attribute__((ext_vector_type(2)));
  __device__ __forceinline__ HistPair *hist_rec(int slot, int e) const {
    return reinterpret_cast<HistPair *>(hist) + hist_record(slot, e, t.n);
  }
  __device__ __forceinline__ void hist_put(int slot, const Vec &s, const Vec &y) {
    const int lane = lane_id();
    if constexpr (kRecords) {
      HistPair *p = hist_rec(slot, lane);
      // (opaque: a record built straight from two elements of the caller's vectors is turned into a two-element LOAD of the
      //  vector object plus an insert -- which then keeps that object, a vector of the optimiser's state, in private memory)
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (in_range(k, lane)) p[k * kWave] = HistPair{(Hist)opaque(s.v[k]), (Hist)opaque(y.v[k])};
    } else {
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (in_range(k, lane)) {
          hist[hist_index_rows(slot, k * kWave + lane, t.n, m, 0)] = (Hist)s.v[k];
          hist[hist_index_rows(slot, k * kWave + lane, t.n, m, 1)] = (Hist)y.v[k];
        }
    }
    lds_wave_sync();
  }
  template <int WHICH>
  __device__ __forceinline__ void hist_get(int slot, Vec &v) const {
    const int lane = lane_id();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int e = k * kWave + lane;
      v.v[k] = in_range(k, lane) ? (Num)hist[kRecords ? hist_index(slot, e, t.n, WHICH) : hist_index_rows(slot, e, t.n, m, WHICH)] : Num(0);
    }
  }
  __device__ __forceinline__ void hist_get_s(int slot, Vec &v) const { hist_get<0>(slot, v); }
  __device__ __forceinline__ void hist_get_y(int slot, Vec &v) const { hist_get<1>(slot, v); }
  // s and y of one pair together.  fp32 pairs: one record a FLAT slot; in the all-fp32 members no read has a condition -- a
  // lane without an element in the partly filled last slot reads record 0 of the pair (inside the region, whatever lies
  // behind it) and takes zeros.  The members with fp64 arithmetic fill the register file, and the two-waves ones with three
  // FLAT slots (cfg5's) pay the address select and its selects to zero in spilled registers (57 and 63 -> 74): they read
  // the record under the lane's mask (57 and 63); with four slots the select is the better one (47 and 80 -> 43;
  // profiles/hist_pairs_kernel_resource_usage.txt).  fp64 pairs: the partly filled last slot of both rows under ONE exec mask.
  static constexpr bool kMaskedRead = sizeof(Num) == 8 && NS == 3;
  __device__ __forceinline__ void hist_get_sy(int slot, Vec &s, Vec &y) const {
    const int lane = lane_id();
    if constexpr (kRecords) {
      const HistPair *p = hist_rec(slot, 0);
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const bool in = in_range(k, lane);
        if constexpr (kMaskedRead) {
          s.v[k] = Num(0);
          y.v[k] = Num(0);
          if (in) {
            const HistPair r = p[k * kWave + lane];
            s.v[k] = (Num)r.x;
            y.v[k] = (Num)r.y;
          }
        } else {
          const HistPair r = p[in ? k * kWave + lane : 0];
          s.v[k] = in ? (Num)r.x : Num(0);
          y.v[k] = in ? (Num)r.y : Num(0);
        }
      }
    } else {
      const Hist *ps = hist + hist_index_rows(slot, lane, t.n, m, 0), *py = hist + hist_index_rows(slot, lane, t.n, m, 1);
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        s.v[k] = Num(0);
        y.v[k] = Num(0);
        if (in_range(k, lane)) {
          s.v[k] = (Num)ps[k * kWave];
          y.v[k] = (Num)py[k * kWave];
        }
      }
    }
  }
  // the 2m wave-uniform scalars of the two-loop recursion (rho, alpha): entry i lives in lane i of one register
  // pair, written with a select and read back with v_readlane -- no LDS round trip on the recursion's dependent chain
  Num sreg = Num(0);
  __device__ __forceinline__ void sput(int i, double v) { sreg = (lane_id() == i) ? (Num)v : sreg; }
  __device__ __forceinline__ double sget(int i) const { return (double)rdlane(sreg, i); }
  // scalar i minus b, in the backend's arithmetic (alpha_k - beta of the two-loop recursion's second loop)
  __device__ __forceinline__ double sdiff(int i, double b) const { return (double)(rdlane(sreg, i) - (Num)b); }
  // rho_slot * (a . b) in the backend's arithmetic (the two-loop recursion's coefficient)
  __device__ __forceinline__ double rho_dot(int slot, const Vec &a, const Vec &b) const {
    Num s = Num(0);
#pragma unroll
    for (int k = 0; k < NS; ++k) s += a.v[k] * b.v[k];
    return (double)(rdlane(sreg, slot) * wave_sum(s));
  }
  // ---- the two-loop recursion two pairs at a time (all-fp32 mode; round 5).  The textbook recursion is 2 * col DEPENDENT
  // steps "read (s, y), dot, wave-wide sum, axpy": a_k = rho_k s_k . q_k needs q_k = q_{k+1} - a_{k+1} y_{k+1}.  Written out for
  // two steps, a_{k-1} = rho_{k-1} (s_{k-1} . q_k - a_k s_{k-1} . y_k): the three dots s_k . q, s_{k-1} . q, s_{k-1} . y_k do not
  // depend on each other, go through ONE batched reduction (wave_sum4) and give both coefficients; likewise the second
  // loop with y_k . r, y_{k+1} . r, y_{k+1} . s_k.  col dependent reductions instead of 2 * col, ~35 vector instructions a
  // pair of steps instead of ~90.  Same mathematics, another rounding (the fp64 modes keep the textbook form: their
  // iterates are pinned to SciPy's, tests/test_lbfgs_host.py).
  static constexpr bool kOwnDirection = sizeof(Num) == 4;
  // the three dots of a pair of steps through one batched reduction
  __device__ __forceinline__ void dot3(const Vec &a0, const Vec &b0, const Vec &a1, const Vec &b1, const Vec &a2, const Vec &b2,
                                       Num &t0, Num &t1, Num &t2) const {
    Num p0 = Num(0), p1 = Num(0), p2 = Num(0);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      p0 += a0.v[k] * b0.v[k];
      p1 += a1.v[k] * b1.v[k];
      p2 += a2.v[k] * b2.v[k];
    }
    Num unused;
    wave_sum4((float)p0, (float)p1, (float)p2, 0.0f, t0, t1, t2, unused);
  }
  __device__ __forceinline__ void direction(const Vec &g, Vec &d, int col, int head, int mm, Num theta) {
    if (col == 0) {
      neg(d, g);
      return;
    }
    if constexpr (!Plan::dynamic && Plan::hist_ahead) {
      if (col == NEO_LBFGS_M) {  // (mm is NEO_LBFGS_M: optimize_body)
        direction_full(g, d, head, mm, theta);
        return;
      }
    }
    auto slot_of = [&](int k) { return head + k < mm ? head + k : head + k - mm; };
    copy(d, g);  // d plays q of the recursion
    Vec sA, yA, sB, yB;
    int k = col - 1;
    for (; k >= 1; k -= 2) {
      const int A = slot_of(k), B = slot_of(k - 1);
      hist_get_sy(A, sA, yA);
      hist_get_sy(B, sB, yB);
      Num t0, t1, t2;
      dot3(sA, d, sB, d, sB, yA, t0, t1, t2);
      const Num aA = rdlane(sreg, A) * t0;
      const Num aB = rdlane(sreg, B) * (t1 - aA * t2);
      sput(mm + A, (double)aA);
      sput(mm + B, (double)aB);
#pragma unroll
      for (int q = 0; q < NS; ++q) d.v[q] = (d.v[q] - aA * yA.v[q]) - aB * yB.v[q];
    }
    if (k == 0) {
      const int A = slot_of(0);
      hist_get_sy(A, sA, yA);
      const Num aA = (Num)rho_dot(A, sA, d);
      sput(mm + A, (double)aA);
      axpy(-(double)aA, yA, d);
    }
    scale(d, (double)(Num(1) / theta));
    k = 0;
    for (; k + 1 < col; k += 2) {
      const int A = slot_of(k), B = slot_of(k + 1);
      hist_get_sy(A, sA, yA);
      hist_get_sy(B, sB, yB);
      Num t0, t1, t2;
      dot3(yA, d, yB, d, yB, sA, t0, t1, t2);
      const Num cA = rdlane(sreg, mm + A) - rdlane(sreg, A) * t0;              // alpha_k - beta_k
      const Num cB = rdlane(sreg, mm + B) - rdlane(sreg, B) * (t1 + cA * t2);
#pragma unroll
      for (int q = 0; q < NS; ++q) d.v[q] = (d.v[q] + cA * sA.v[q]) + cB * sB.v[q];
    }
    if (k < col) {
      const int A = slot_of(k);
      hist_get_sy(A, sA, yA);
      const double b = rho_dot(A, yA, d);
      axpy(sdiff(mm + A, b), sA, d);
    }
    scale(d, -1.0);
  }
  // ---- the same recursion for a full memory (col = m), written out step by step (a fixed plan's constant, Plan::hist_ahead).
  // Above, every step begins with the LDS reads of its pairs and waits for them at once: the reduction, the coefficients and
  // the axpy all follow that wait, 10 LDS round trips in series an iteration, and loop 2 reads every pair again.  The
  // addresses depend on head and the lane alone, not on the recursion.  With col a constant every pair has registers of its
  // own (4 NS a pair): each is read ONCE, one step ahead of its use in loop 1, and loop 2 reads nothing; alpha_k stays in a
  // register between the loops instead of a lane of sreg; 1 / theta is formed ahead of the steps, off the chain between the
  // loops.  The control flow is hist_walk_full (neo_lbfgs_dir.hpp), this struct its visitor.  Same pairs in the same order
  // through the same expressions: the same bits as above (which optimize_dyn_kernel and the budgeted members keep for every
  // col, and these kernels while the memory fills; tests/test_gpu_hist_ahead.py compares the two).
  // No read has a condition around it -- a wait in front of a step's dots is a counted one, and one path into it that
  // reads less makes it a wait for everything: the partly filled FLAT slot is read without an exec mask and without an
  // address of its own (a lane beyond n reads the records that follow: the next pair's, behind the last pair
  // hist_over_read_elems elements of whatever lies there -- the launcher admits this kernel only where that is the launch's
  // own LDS, neo_launch_opt.hpp opt_plan_fixed) and `settle` puts the zeros of hist_get_sy there before the values are used.
  template <int COL>
  struct DirFull {
    DevBackend &be;
    Vec &d;
    const Num inv_theta;
    Vec s[COL], y[COL];
    Num alpha[COL];
    __device__ __forceinline__ void settle(Vec &sv, Vec &yv) const {
#pragma unroll
      for (int k = kFull; k < NS; ++k)
        if (lane_ge(be.t.n - k * kWave)) {
          sv.v[k] = Num(0);
          yv.v[k] = Num(0);
        }
    }
    template <int K>
    __device__ __forceinline__ void read(int slot) {
      // one address a pair: record `lane` of the slot, the next FLAT slot 64 records on (a compile-time offset)
      const HistPair *p = be.hist_rec(slot, lane_id());
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const HistPair r = p[k * kWave];
        s[K].v[k] = (Num)r.x;
        y[K].v[k] = (Num)r.y;
      }
    }
    template <int KA, int KB>
    __device__ __forceinline__ void pair1(int A, int B) {
      settle(s[KA], y[KA]);
      settle(s[KB], y[KB]);
      Num t0, t1, t2;
      be.dot3(s[KA], d, s[KB], d, s[KB], y[KA], t0, t1, t2);
      const Num aA = rdlane(be.sreg, A) * t0;
      const Num aB = rdlane(be.sreg, B) * (t1 - aA * t2);
      alpha[KA] = aA;
      alpha[KB] = aB;
#pragma unroll
      for (int q = 0; q < NS; ++q) d.v[q] = (d.v[q] - aA * y[KA].v[q]) - aB * y[KB].v[q];
    }
    template <int KA, int KB>
    __device__ __forceinline__ void pair2(int A, int B) {
      Num t0, t1, t2;
      be.dot3(y[KA], d, y[KB], d, y[KB], s[KA], t0, t1, t2);
      const Num cA = alpha[KA] - rdlane(be.sreg, A) * t0;              // alpha_k - beta_k
      const Num cB = alpha[KB] - rdlane(be.sreg, B) * (t1 + cA * t2);
#pragma unroll
      for (int q = 0; q < NS; ++q) d.v[q] = (d.v[q] + cA * s[KA].v[q]) + cB * s[KB].v[q];
    }
    template <int K>
    __device__ __forceinline__ void single1(int A) {
      settle(s[K], y[K]);
      const Num aA = (Num)be.rho_dot(A, s[K], d);
      alpha[K] = aA;
      be.axpy(-(double)aA, y[K], d);
    }
    template <int K>
    __device__ __forceinline__ void single2(int A) {
      const double b = be.rho_dot(A, y[K], d);
      be.axpy((double)(alpha[K] - (Num)b), s[K], d);
    }
    __device__ __forceinline__ void seam() { be.scale(d, (double)inv_theta); }
  };
  __device__ __forceinline__ void direction_full(const Vec &g, Vec &d, int head, int mm, Num theta) {
    copy(d, g);  // d plays q of the recursion
    DirFull<NEO_LBFGS_M> w{*this, d, Num(1) / theta};
    hist_walk_full<NEO_LBFGS_M>(head, mm, w);
    scale(d, -1.0);
  }

  // (line-search state and cost terms in LDS: in registers they spill, measured 14.0 against 15.5 ms at cfg2)
  __device__ __forceinline__ LineSearchT<Scalar> &ls() { return *lsp; }
  __device__ __forceinline__ double *cost_store() { return cst; }

  // diagnostics (neo_optimize_trace / neo_optimize_trace_xg): one record per counted evaluation -- (f, step, samples,
  // iteration) and, when asked for, the evaluated point and its gradient (replay tests: every evaluation of a run is laid
  // beside the CPU oracle's at the same point)
  __device__ __forceinline__ void note_eval(int nfev, int iter, double stp, double f, const Vec &x, const Vec &g) {
    // (trace_cap is 0 when neither buffer was given: ONE scalar test in the product path -- the two pointers tested
    //  here were four spilled scalar registers re-read at every evaluation)
    if constexpr (!Plan::dynamic && !Plan::trace) return;  // (a plan without trace buffers: no hook at all)
    if (nfev > trace_cap) return;
    if (trace != nullptr && lane_id() == 0) {
      double *r = trace + (size_t)(nfev - 1) * 4;
      r[0] = f;
      r[1] = stp;
      r[2] = (double)last_ns;
      r[3] = (double)iter;
    }
    if (trace_xg != nullptr) {
      const int lane = lane_id();
      double *r = trace_xg + (size_t)(nfev - 1) * 2 * t.n;
#pragma unroll
      for (int k = 0; k < NS; ++k)
        if (k * kWave + lane < t.n) {
          r[k * kWave + lane] = (double)x.v[k];
          r[t.n + k * kWave + lane] = (double)g.v[k];
        }
    }
  }

  // FLAT x -> PIECE inputs
  __device__ __forceinline__ void scatter_x(const Vec &x) {
    // (opaque: the LDS addresses below are loop invariant -- hoisted out of the optimiser loop they become nine registers
    // that live across everything and are spilled; formed here they cost one instruction each)
    const int lane = opaque(lane_id());
    lds_wave_sync();
    Num *xn = reinterpret_cast<Num *>(xs);  // (the staging holds Num values)
#pragma unroll
    for (int k = 0; k < NS; ++k)
      if (in_range(k, lane)) xn[k * kWave + lane] = x.v[k];
    lds_wave_sync();
    const int M = t.M;
    const int p = opaque(LG::piece());
    const bool act = p < M;
    t.tau = act ? xn[t.nq + p] : Num(0);
#pragma unroll
    for (int d = 0; d < DL; ++d) {
      const int dg = LG::dim0() + d;  // the dimension: compile-time when the lane holds all of them
      t.P0[d] = (p == 0 || !act) ? bstate<D, LG, false>(t, 0, d) : xn[dg * (M - 1) + (p > 0 ? p - 1 : 0)];
      t.P1[d] = (p >= M - 1) ? bstate<D, LG, true>(t, 0, d) : xn[dg * (M - 1) + p];
    }
  }

  // one evaluation of cost and gradient (get_cost + get_grad, :539-585)
  __device__ __forceinline__ int eval(const Vec &x, double &f, Vec &g, double *costs) {
    const int lane = lane_id();
    const int p = LG::piece();
    NEO_MARK("eval_begin");
    // Lane masks such as `piece < M` are loop invariant: hoisted out of the optimiser loop they are scalar register PAIRS
    // that live across everything, the allocator spills them to lanes of a vector register, and every use inside the
    // loop pays two v_readlane on the vector pipe (round 4: ~120 of them an evaluation).  The piece count is re-read
    // through an opaque copy at the head of every phase, so the masks are compared where they are used (one v_cmp).
    const int M_all = t.M;
    t.M = opaque_uniform(M_all);
    scatter_x(x);
    NEO_MARK("scatter_done");
    Num *xn = reinterpret_cast<Num *>(xs);
    double energy, tsum;
    const int st = minco_forward<D, LG, Num, kPcr, Plan>(t, prm, energy, tsum);
    NEO_MARK("forward_done");
    if (st != 0) {
      f = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) costs[k] = 0.0;
      return st;
    }
    if (plan_pick<Plan, Plan::coeff_out>(coeff_out != nullptr) && p < t.M) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int d = 0; d < DL; ++d) coeff_out[(size_t)(6 * p + k) * D + LG::dim0() + d] = (double)t.c[k][d];
    }
    Num gC[6][DL], gT = Num(0);
    double cf, ck;
    {
      Real cr[6][DL], gCr[6][DL], gTr;
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int d = 0; d < DL; ++d) cr[k][d] = (Real)t.c[k][d];
      LookupT lk(map);
      // lanes in proportion to the pieces' sample counts (xs is free between scatter_x and the gradient gather);
      // the assignment wants the sample count of piece l in lane l
      int ns_by_piece = t.ns;
      if constexpr (LG::S > 1) ns_by_piece = __shfl(t.ns, min(LG::S * lane, kWave - 1), kWave);
      NEO_MARK("assign_begin");
      t.M = opaque_uniform(M_all);
      SampleLanes sl;
      bool cached = false;
      const int ns_key = lane < t.M ? ns_by_piece : 0;  // (what balanced_sample_lanes sees of this lane)
      const bool have_cache = plan_pick<Plan, Plan::sl_cache>(sl_cache != nullptr);
      if (have_cache) cached = __ballot(ns_key == (int)reinterpret_cast<const unsigned char *>(sl_cache)[lane]) == ~0ull;
      if (cached) {
        const unsigned pk = (unsigned)sl_cache[kWave / 4 + lane];
        sl.piece = pk & 63;
        sl.r = (pk >> 6) & 63;
        sl.L = (pk >> 12) & 127;
        sl.act = ((pk >> 19) & 1) != 0;
        sl.first = (pk >> 20) & 63;
        sl.Lp = pk >> 26;  // (<= 32 here: Lp = 64 means a single piece, which has no entry -- see the store)
        sl.rounds = __builtin_amdgcn_readfirstlane(sl_cache[kWave / 4 + kWave]);
        sl.lmax = __builtin_amdgcn_readfirstlane(sl_cache[kWave / 4 + kWave + 1]);
        sl.total = __builtin_amdgcn_readfirstlane(sl_cache[kWave / 4 + kWave + 2]);
      } else {
        sl = balanced_sample_lanes<kAhead>(t.M, ns_by_piece, reinterpret_cast<int *>(xs));
        if (have_cache) {
          // one byte a lane for the key (sample counts stay below T_max / delta_t; 255 = never equal), one word for the
          // assignment; a piece with more than 63 lanes (M = 1) does not fit the word's six bits: not cached
          const bool fits = sl.lmax < 64 && ns_key < 255;
          reinterpret_cast<unsigned char *>(sl_cache)[lane] = (unsigned char)(__ballot(!fits) == 0 ? ns_key : 255);
          sl_cache[kWave / 4 + lane] = (int)((unsigned)sl.piece | ((unsigned)sl.r << 6) | ((unsigned)sl.L << 12) |
                                             ((sl.act ? 1u : 0u) << 19) | ((unsigned)sl.first << 20) | ((unsigned)sl.Lp << 26));
          if (lane == 0) {
            sl_cache[kWave / 4 + kWave] = sl.rounds;
            sl_cache[kWave / 4 + kWave + 1] = sl.lmax;
            sl_cache[kWave / 4 + kWave + 2] = sl.total;
          }
          lds_wave_sync();
        }
      }
      last_ns = sl.total;  // (the lane assignment has summed the sample counts already)
      samples += (long long)last_ns;
      NEO_MARK("assign_done");
      minco_sample<Real, D, LookupT, SU, false, LG, Plan>(
          t.M, sl, t.ns, cr, prm, lk, gCr, gTr, cf, ck,
          plan_pick<Plan, Plan::fold_rows>(fold_rows) ? reinterpret_cast<Real *>(xs) : nullptr, fold_acc);
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int d = 0; d < DL; ++d) gC[k][d] = (Num)gCr[k][d];
      gT = (Num)gTr;
    }
    costs[0] = uniform(energy);
    costs[1] = uniform(tsum);
    costs[2] = uniform(cf);
    costs[3] = uniform(ck);
    f = uniform(costs[0] * prm.w[0] + costs[1] * prm.w[1] + costs[2] * prm.w[2] + costs[3] * prm.w[3]);
    Num gq[DL], gtau;
    NEO_MARK("sample_done");
    t.M = opaque_uniform(M_all);
    if constexpr (kAhead && sizeof(Num) == 4) {
      // the powers of 1 / T are formed again for the adjoint by minco_forward's expressions (the same bits) instead of
      // being held across the sample phase: three registers for the round the sample loop keeps in flight
      const Num i1 = opaque(t.i1);
      t.i2 = i1 * i1;
      t.i3 = t.i2 * i1;
      t.i4 = t.i2 * t.i2;
    }
    const int bst = minco_backward<D, LG, Num, kPcr, Plan>(t, prm, gC, gT, gq, gtau);
    NEO_MARK("backward_done");
    if (bst != 0) return bst;
    // PIECE -> FLAT (addresses formed here, as in scatter_x)
    lds_wave_sync();
    const int pg = opaque(p), lg = opaque(lane);
    if (pg >= 1 && pg < t.M) {
#pragma unroll
      for (int d = 0; d < DL; ++d) xn[(LG::dim0() + d) * (t.M - 1) + pg - 1] = gq[d];
    }
    if (pg < t.M && LG::dim0() == opaque_uniform(0)) xn[t.nq + pg] = gtau;
    lds_wave_sync();
#pragma unroll
    for (int k = 0; k < NS; ++k) g.v[k] = in_range(k, lg) ? xn[k * kWave + lg] : Num(0);
    NEO_MARK("gather_done");
    return 0;
  }
};

// ------------------------------------------------------------------ suspended runs (neo_optimize_batch_budget_dev)
// A launch with an evaluation budget stops a run that needs more: everything the optimiser carries between two
// evaluations -- the machine's vectors and scalars, the line search, the stored pairs and their rho, the cost terms --
// goes to `st` (doubles: every fp32 value converts exactly both ways) and a later launch picks the run up at the very
// evaluation it was about to make.  Layout: [64 scalars | x g t r d (n each) | rho / alpha lanes (64) | pairs (2 m n)].
// The pairs are the LDS region as it stands, element for element (hist_index / hist_index_rows decide where a value lies,
// here as there: a state is read by the build that wrote it).  Its size is opt_state_doubles (neo_host.hpp).

template <class BE, class Mach>
__device__ __forceinline__ void save_run(BE &be, const Mach &mc, double *st) {
  const int lane = lane_id(), n = be.t.n;
  lds_wave_sync();
  if (lane == 0) {
    const int iv[9] = {mc.phase, mc.status, mc.nfev, mc.nit, mc.iter, mc.col, mc.head, mc.task, mc.ifun};
#pragma unroll
    for (int k = 0; k < 9; ++k) st[k] = (double)iv[k];
    const double dv[7] = {(double)mc.f, (double)mc.fold, (double)mc.stp, (double)mc.gd, (double)mc.gdold, (double)mc.theta,
                          (double)mc.stp_evaluated};
#pragma unroll
    for (int k = 0; k < 7; ++k) st[9 + k] = dv[k];
    st[16] = (double)be.samples;
    st[17] = (double)be.last_ns;
    const auto &L = *be.lsp;
    const double lv[20] = {(double)L.ftol, (double)L.gtol, (double)L.xtol, (double)L.stpmin, (double)L.stpmax, (double)L.brackt,
                           (double)L.stage, (double)L.ginit, (double)L.gtest, (double)L.gx, (double)L.gy, (double)L.finit,
                           (double)L.fx, (double)L.fy, (double)L.stx, (double)L.sty, (double)L.stmin, (double)L.stmax,
                           (double)L.width, (double)L.width1};
#pragma unroll
    for (int k = 0; k < 20; ++k) st[20 + k] = lv[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) st[40 + k] = be.cst[k];
  }
  double *v = st + 64;
#pragma unroll
  for (int k = 0; k < BE::kSlotsN; ++k)
    if (k * kWave + lane < n) {
      const int e = k * kWave + lane;
      v[e] = (double)mc.x.v[k];
      v[n + e] = (double)mc.g.v[k];
      v[2 * n + e] = (double)mc.t.v[k];
      v[3 * n + e] = (double)mc.r.v[k];
      v[4 * n + e] = (double)mc.d.v[k];
    }
  v[5 * n + lane] = (double)be.sreg;
  double *h = v + 5 * n + kWave;
  for (int i = lane; i < 2 * be.m * n; i += kWave) h[i] = (double)be.hist[i];
}

template <class BE, class Mach>
__device__ __forceinline__ void load_run(BE &be, Mach &mc, const double *st) {
  using Num = decltype(be.sreg);
  const int lane = lane_id(), n = be.t.n;
  auto iu = [&](int k) { return (int)uniform(st[k]); };
  mc.phase = iu(0); mc.status = iu(1); mc.nfev = iu(2); mc.nit = iu(3); mc.iter = iu(4);
  mc.col = iu(5); mc.head = iu(6); mc.task = iu(7); mc.ifun = iu(8);
  using S = typename Mach::S;  // (every fp32 scalar went to the state as a double: exact both ways)
  mc.f = (S)uniform(st[9]); mc.fold = (S)uniform(st[10]); mc.stp = (S)uniform(st[11]); mc.gd = (S)uniform(st[12]);
  mc.gdold = (S)uniform(st[13]); mc.theta = (S)uniform(st[14]); mc.stp_evaluated = (S)uniform(st[15]);
  be.samples = (long long)uniform(st[16]);
  be.last_ns = iu(17);
  if (lane == 0) {
    auto &L = *be.lsp;
    L.ftol = (S)st[20]; L.gtol = (S)st[21]; L.xtol = (S)st[22]; L.stpmin = (S)st[23]; L.stpmax = (S)st[24];
    L.brackt = (int)st[25]; L.stage = (int)st[26];
    L.ginit = (S)st[27]; L.gtest = (S)st[28]; L.gx = (S)st[29]; L.gy = (S)st[30]; L.finit = (S)st[31]; L.fx = (S)st[32];
    L.fy = (S)st[33]; L.stx = (S)st[34]; L.sty = (S)st[35]; L.stmin = (S)st[36]; L.stmax = (S)st[37]; L.width = (S)st[38];
    L.width1 = (S)st[39];
#pragma unroll
    for (int k = 0; k < 12; ++k) be.cst[k] = st[40 + k];
  }
  const double *v = st + 64;
#pragma unroll
  for (int k = 0; k < BE::kSlotsN; ++k) {
    const int e = k * kWave + lane;
    const bool in = e < n;
    mc.x.v[k] = in ? (Num)v[e] : Num(0);
    mc.g.v[k] = in ? (Num)v[n + e] : Num(0);
    mc.t.v[k] = in ? (Num)v[2 * n + e] : Num(0);
    mc.r.v[k] = in ? (Num)v[3 * n + e] : Num(0);
    mc.d.v[k] = in ? (Num)v[4 * n + e] : Num(0);
  }
  be.sreg = (Num)v[5 * n + lane];
  const double *h = v + 5 * n + kWave;
  for (int i = lane; i < 2 * be.m * n; i += kWave) be.hist[i] = (typename BE::Hist)h[i];
  lds_wave_sync();
}

struct MapTable {
  const void *maps;  // array of MapT indexed by scene slot
};

// ------------------------------------------------------------------ kernels
template <int D, int NS, typename Real, class MapT, class LookupT, class LG = WaveLanes, typename Num = double>
__global__ __launch_bounds__(kWave) void eval_kernel(int B, int M, DevParams prm, MapT map,
                                                      const double *__restrict__ x,
                                                      const double *__restrict__ head,
                                                      const double *__restrict__ tail,
                                                      double *__restrict__ cost, double *__restrict__ costs4,
                                                      double *__restrict__ grad, double *__restrict__ coeffs,
                                                      int *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) double xs[stage_doubles<D, NS, Real>()];
  __shared__ LineSearchT<opt_scalar_t<Num, NS>> lsm;
  __shared__ double cst[12];
  __shared__ Num bnd[6 * D];
  // all-fp32 mode, lane = (piece, dimension): the cyclic reduction's multipliers stay in LDS for the adjoint pass
  constexpr bool kKeep = sizeof(Num) == 4 && LG::S > 1;
  __shared__ __attribute__((aligned(16))) Num mult_s[kKeep ? (5 * 8 + 4) * (kWave / LG::S + 1) : 4];
  const int b = blockIdx.x;
  if (b >= B) return;
  using BE = DevBackend<D, NS, Real, MapT, LookupT, NEO_FUSED_U, LG, false, Num>;
  BE be(prm, map);
  if constexpr (kKeep) be.t.pcr_mult = mult_s;
  be.xs = xs;
  if constexpr (sizeof(Num) == 4 && LG::W == kWave)   // (the staging doubles as the cyclic reduction's exchange table)
    if (pcr_xch_elems(M, LG::dl(D)) * (int)sizeof(Num) <= stage_doubles<D, NS, Real>() * 8) be.t.pcr_xch = reinterpret_cast<Num *>(xs);
  be.lsp = &lsm;
  be.cst = cst;
  be.hist = nullptr;
  be.m = NEO_LBFGS_M;
  load_boundary<LG>(be.t, head + (size_t)b * 3 * D, tail + (size_t)b * 3 * D, M, bnd);
  const int n = be.t.n;
  be.npad = NS * kWave;
  be.coeff_out = coeffs ? coeffs + (size_t)b * 6 * M * D : nullptr;
  const int lane = lane_id();
  typename BE::Vec xv, gv;
#pragma unroll
  for (int k = 0; k < NS; ++k) xv.v[k] = (k * kWave + lane < n) ? x[(size_t)b * n + k * kWave + lane] : 0.0;
  double f;
  double *costs = cst;
  const int st = be.eval(xv, f, gv, costs);
#pragma unroll
  for (int k = 0; k < NS; ++k)
    if (k * kWave + lane < n) grad[(size_t)b * n + k * kWave + lane] = gv.v[k];
  if (lane == 0) {
    cost[b] = f;
#pragma unroll
    for (int k = 0; k < 4; ++k) costs4[(size_t)b * 4 + k] = costs[k];
    if (status) status[b] = st;
  }
}

// WAVES = wavefronts per SIMD the register allocation aims at.  1: the whole file (256 VGPRs + AGPRs) for one
// trajectory -- the shortest evaluation, for batches that leave SIMDs to spare.  2: half the file (the cfg2
// instantiation fits it without spills) -- each evaluation is slower, but two trajectories share a SIMD's issue
// slots, which wins once the batch queues for the 1024 SIMDs anyway.  Same source, same arithmetic, bit-identical
// results.
// Dynamic LDS (launch parameter): `stage` doubles of staging (DevBackend::xs) followed by the 2 * maxcor * n doubles of
// the L-BFGS pairs.  The launcher gives the staging its full size (room for the rows of the per-piece fold) unless that
// would cost a wavefront of occupancy -- then NS * 64 doubles, and the fold runs in registers.
// BUDGET (neo_optimize_batch_budget_dev; instantiated in neo_disp_opt3d_b.hip only): a run that has not terminated after
// `budget` evaluations in this launch is suspended -- its state to `state`, status NEO_TRAJ_SUSPENDED -- and a launch
// with `resume` set continues the suspended runs of its trajectories (the others it leaves untouched).
// The kernel is compiled once per launch plan (neo_device.hpp PlanDynamic / PlanFixedX): optimize_body is the whole run,
// optimize_kernel and optimize_dyn_kernel below are its two wrappers.
template <class Plan, int D, int NS, typename Real, class MapT, class LookupT, int WAVES, class LG, typename Num, bool BUDGET>
__device__ __forceinline__ void optimize_body(int B, int M, const DevParams &prm, const MapT *maps,
                                              const int *__restrict__ scene_slot, int nmaps, const double *x0, double *x,
                                              const double *__restrict__ head, const double *__restrict__ tail,
                                              double *__restrict__ costs4, double *__restrict__ costs4_last,
                                              int *__restrict__ nit, int *__restrict__ nfev, int *__restrict__ status,
                                              long long *__restrict__ nsamples, const int *__restrict__ order,
                                              double *__restrict__ trace, double *__restrict__ trace_xg, int trace_cap, int stage,
                                              int pcr_off, double *state, int state_doubles, int budget, int resume,
                                              int traj_total) {
  extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
  __shared__ LineSearchT<opt_scalar_t<Num, NS>> lsm;
  __shared__ double cst[12];
  __shared__ Num bnd[6 * D];
  // the all-fp32 kernels keep the last lane assignment (DevBackend::sl_cache; launch_opt counts its 336 bytes)
  constexpr bool kSlCache = sizeof(Num) == 4;
  __shared__ __attribute__((aligned(8))) int slc[kSlCache ? kSlCacheInts : 2];
  if ((int)blockIdx.x >= B) return;
  // workgroups are dispatched in index order: `order` lets the caller start the runs it expects to
  // be long first (list scheduling: a long run that starts last sets the duration of the launch)
  const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
  if constexpr (BUDGET)  // (a subset launch names its trajectories: an entry outside the arrays is skipped)
    if (b < 0 || b >= traj_total) return;
  // the two-waves variant has half the registers: two samples per lane in flight instead of four (with the lean
  // Horner form, cfg2 with three batches in flight: 414 k -> 541 k traj/s; scratch 640 -> 336 B per lane)
  using BE = DevBackend<D, NS, Real, MapT, LookupT, (WAVES == 2 ? NEO_W2_U : NEO_FUSED_U), LG,
                        pairs_in_f32<Real, NS, WAVES>() || sizeof(Num) == 4, Num, Plan>;
  // a slot outside the table (a stale or foreign slot array): the trajectory is left untouched and flagged
  const int slot = scene_slot ? scene_slot[b] : 0;
  if (slot < 0 || slot >= nmaps) {
    if (lane_id() == 0) {
      status[b] = NEO_TRAJ_BAD_SCENE;
      nit[b] = 0;
      nfev[b] = 0;
      if constexpr (!BUDGET)  // (the progress counter counts every trajectory of the launch: below)
        if (state != nullptr) __hip_atomic_fetch_add(reinterpret_cast<int *>(state), 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  const MapT map = maps[slot];
  BE be(prm, map);
  be.xs = dyn_lds;
  be.fold_rows = stage >= stage_doubles<D, NS, Real>();
  // pcr_off != 0 (all-fp32 mode, lane = (piece, dimension), launch_opt): the multipliers of the forward cyclic reduction
  // live at dyn_lds + pcr_off (doubles) for the adjoint pass, and the staging holds per-piece accumulators for the fold
  if constexpr (sizeof(Num) == 4 && LG::S > 1) {
    if (plan_pick<Plan, Plan::pcr_mult>(pcr_off != 0)) {
      be.t.pcr_mult = reinterpret_cast<Num *>(dyn_lds + pcr_off);
      be.fold_rows = true;
      be.fold_acc = true;
    }
  }
  if constexpr (sizeof(Num) == 4 && LG::W == kWave)   // (the staging doubles as the cyclic reduction's exchange table)
    if (plan_pick<Plan, Plan::pcr_xch>(be.fold_rows && pcr_xch_elems(M, LG::dl(D)) * (int)sizeof(Num) <= stage * 8))
      be.t.pcr_xch = reinterpret_cast<Num *>(dyn_lds);
  be.lsp = &lsm;
  be.cst = cst;
  be.m = NEO_LBFGS_M;
  be.coeff_out = nullptr;
  if constexpr (kSlCache) {
    if (lane_id() < kWave / 4) slc[lane_id()] = -1;  // (key bytes 255: the first evaluation misses)
    be.sl_cache = slc;
  }
  if constexpr (Plan::dynamic || Plan::trace) {
    be.trace = trace ? trace + (size_t)b * trace_cap * 4 : nullptr;
    be.trace_cap = (trace != nullptr || trace_xg != nullptr) ? trace_cap : 0;
    be.trace_xg = trace_xg ? trace_xg + (size_t)b * trace_cap * 2 * (D * (M - 1) + M) : nullptr;
  }
  load_boundary<LG>(be.t, head + (size_t)b * 3 * D, tail + (size_t)b * 3 * D, M, bnd);
  const int n = be.t.n;
  be.npad = NS * kWave;
  be.hist = reinterpret_cast<typename BE::Hist *>(dyn_lds + stage);
  const int lane = lane_id();
  typename BE::Vec xv;
#pragma unroll
  for (int k = 0; k < NS; ++k) xv.v[k] = (k * kWave + lane < n) ? x0[(size_t)b * n + k * kWave + lane] : 0.0;
  LbfgsOpts o{prm.ftol, prm.gtol, prm.maxls, prm.maxiter, prm.maxfun, NEO_LBFGS_M};
  LbfgsResult res;
  // n <= 128: the run as "evaluate, then advance" (neo_lbfgs_sm.hpp: the same arithmetic and decisions as
  // lbfgs_minimize) -- ONE inlined copy of the evaluation instead of two: 36 % less code and no spills in the cfg2
  // two-waves kernel.  Four FLAT slots (n > 128, cfg5): the compiler keeps the machine's vectors in private memory
  // (1 KB of scratch, 3x slower), so those instantiations run the straight-line form.
  bool suspended = false;
  // (round 5, measured and dropped: wavefronts raising their own issue priority -- s_setprio -- as their evaluations pass
  //  128 / 256 / 384: 1.444 - 1.451 M traj/s against 1.439 - 1.440 M, a single batch unchanged: HISTORY.md)
  if constexpr (NS <= NEO_SM_MAX_SLOTS) {
    LbfgsMachine<BE> mach(be, o);
    if constexpr (BUDGET) {
      double *st = state + (size_t)b * (size_t)state_doubles;
      if (resume) {
        if (status[b] != NEO_TRAJ_SUSPENDED) return;  // (finished in an earlier launch: its results stay as they are)
        load_run(be, mach, st);
      } else {
        mach.x = xv;
        mach.begin();
      }
      int evals = 0;
      while (mach.need_eval()) {
        if (evals >= budget) {
          save_run(be, mach, st);
          suspended = true;
          break;
        }
        double fe;
        const int est = be.eval(mach.x, fe, mach.g, mach.costs());
        mach.f = (typename BE::Scalar)fe;
        mach.advance(est);
        ++evals;
      }
    } else {
      mach.x = xv;
      mach.begin();
      while (mach.need_eval()) {
        double fe;
        const int est = be.eval(mach.x, fe, mach.g, mach.costs());
        mach.f = (typename BE::Scalar)fe;
        mach.advance(est);
      }
    }
    mach.result(res);
    xv = mach.x;
  } else {
    lbfgs_minimize<BE>(be, xv, o, res);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k)
    if (k * kWave + lane < n) x[(size_t)b * n + k * kWave + lane] = xv.v[k];
  if (lane == 0) {
    int st = res.status;
    // weighted collision cost of the last evaluated x against the tolerance (:233-237)
    if (res.costs_last[3] * prm.w[3] > prm.coll_tol) st |= NEO_TRAJ_FLAG_COLLISION;
    if (suspended) st = NEO_TRAJ_SUSPENDED;  // (x = the point the run evaluates next, costs4 = the terms at its last iterate)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      costs4[(size_t)b * 4 + k] = res.costs[k];
      if (costs4_last) costs4_last[(size_t)b * 4 + k] = res.costs_last[k];
    }
    nit[b] = res.nit;
    nfev[b] = res.nfev;
    status[b] = st;
    if (nsamples) nsamples[b] = be.samples;
  }
  // Progress counter (neo_optimize_progress_counter, round 6; plain launches only -- their `state` argument carries it): one
  // system-scope release add per finished trajectory, after every lane's result stores.  A host that polls the counter
  // knows how many trajectories are complete while the launch's long runs are still going, and may read x / status of those
  // (status[b] != NEO_TRAJ_RUNNING, preset by the caller) through a copy on another stream.
  if constexpr (!BUDGET) {
    if (state != nullptr && lane == 0)
      __hip_atomic_fetch_add(reinterpret_cast<int *>(state), 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The plan optimize_kernel<...> is compiled for.  The all-fp32 kernels with lane = (piece, dimension) and n <= 128
// variables (cfg2's member among them) always get PlanFixedX from opt_lds_plan unless flags bit 4096 is set: their
// optimize_kernel holds that plan alone, and launch_opt_kernel (neo_launch_opt.hpp) sends every other launch -- comparison
// runs, trace buffers, a plan that is not the fixed one -- to optimize_dyn_kernel.  Every other member, the budgeted ones
// included, has the dynamic plan in optimize_kernel itself.
template <int NS, class LG, typename Num, bool BUDGET>
using opt_plan_t = std::conditional_t<sizeof(Num) == 4 && (LG::S > 1) && NS <= 2 && !BUDGET, PlanFixedX, PlanDynamic>;

// optimize_kernel<...>'s sample loop is the gather-ahead form, which keeps two rounds of velocity in the staging buffer
// (velocity_stash_bytes: the launcher makes the room and sends a launch without it to optimize_dyn_kernel)
template <int D, int NS, typename Real, class MapT, class LookupT, int WAVES, class LG, typename Num, bool BUDGET>
constexpr bool opt_gather_ahead() {
  return DevBackend<D, NS, Real, MapT, LookupT, (WAVES == 2 ? NEO_W2_U : NEO_FUSED_U), LG, false, Num,
                    opt_plan_t<NS, LG, Num, BUDGET>>::kAhead;
}

#define NEO_OPT_LAUNCH_BOUNDS __launch_bounds__(kWave, (WAVES == 2 ? (sizeof(Num) == 4 && NS <= 2 ? NEO_X_OCC : NEO_W2_OCC) : 1))

// the product kernel.  (One argument list for every plan: under a fixed plan the trace arguments are never read -- the
// launcher passes them to optimize_dyn_kernel instead -- and an argument nobody reads is not loaded from the segment.)
template <int D, int NS, typename Real, class MapT, class LookupT, int WAVES, class LG = WaveLanes, typename Num = double,
          bool BUDGET = false>
__global__ NEO_OPT_LAUNCH_BOUNDS void optimize_kernel(int B, int M, DevParams prm, const MapT *maps,
                                                          const int *__restrict__ scene_slot, int nmaps,
                                                          const double *x0, double *x,
                                                          const double *__restrict__ head,
                                                          const double *__restrict__ tail,
                                                          double *__restrict__ costs4,
                                                          double *__restrict__ costs4_last,
                                                          int *__restrict__ nit, int *__restrict__ nfev,
                                                          int *__restrict__ status,
                                                          long long *__restrict__ nsamples,
                                                          const int *__restrict__ order, double *__restrict__ trace,
                                                          double *__restrict__ trace_xg, int trace_cap,
                                                          int stage, int pcr_off,
                                                          double *state, int state_doubles, int budget, int resume,
                                                          int traj_total) {
  optimize_body<opt_plan_t<NS, LG, Num, BUDGET>, D, NS, Real, MapT, LookupT, WAVES, LG, Num, BUDGET>(
      B, M, prm, maps, scene_slot, nmaps, x0, x, head, tail, costs4, costs4_last, nit, nfev, status, nsamples, order, trace,
      trace_xg, trace_cap, stage, pcr_off, state, state_doubles, budget, resume, traj_total);
}

// the same run with every selector of the plan a run-time value: comparison runs (flags bit 4096), launches with a trace
// buffer, and any launch whose plan is not the one optimize_kernel was compiled for.  Same arithmetic, same bits.
template <int D, int NS, typename Real, class MapT, class LookupT, int WAVES, class LG = WaveLanes, typename Num = double,
          bool BUDGET = false>
__global__ NEO_OPT_LAUNCH_BOUNDS void optimize_dyn_kernel(int B, int M, DevParams prm, const MapT *maps,
                                                              const int *__restrict__ scene_slot, int nmaps,
                                                              const double *x0, double *x,
                                                              const double *__restrict__ head,
                                                              const double *__restrict__ tail,
                                                              double *__restrict__ costs4,
                                                              double *__restrict__ costs4_last,
                                                              int *__restrict__ nit, int *__restrict__ nfev,
                                                              int *__restrict__ status,
                                                              long long *__restrict__ nsamples,
                                                              const int *__restrict__ order, double *__restrict__ trace,
                                                              double *__restrict__ trace_xg, int trace_cap,
                                                              int stage, int pcr_off,
                                                              double *state, int state_doubles, int budget, int resume,
                                                              int traj_total) {
  optimize_body<PlanDynamic, D, NS, Real, MapT, LookupT, WAVES, LG, Num, BUDGET>(
      B, M, prm, maps, scene_slot, nmaps, x0, x, head, tail, costs4, costs4_last, nit, nfev, status, nsamples, order, trace,
      trace_xg, trace_cap, stage, pcr_off, state, state_doubles, budget, resume, traj_total);
}
#undef NEO_OPT_LAUNCH_BOUNDS

// add_sampled_cost + add_sampled_grad_CT (expert_planner.py:392-466) as a kernel of its own: the ESDF
// lookup kernel.  Input: polynomial coefficients and durations; output: the two sampled cost terms and
// their partials w.r.t. coefficients and durations.  One wavefront per trajectory; every lane reads the
// coefficients of its piece straight into the SAMPLE layout and the first lane of each piece writes the
// piece's partials.  fp32: <= 128 VGPRs, so four waves per SIMD -- the whole cfg2 batch is resident at once and
// the gathers of different trajectories overlap (one sample per lane in flight is enough then).
#ifndef NEO_SAMPLE_U
#define NEO_SAMPLE_U 1
#endif
#ifndef NEO_SAMPLE_OCC
// waves per SIMD the fp32 instantiations are allocated for.  Round 6: five (94 registers suffice): the launch over a whole
// step's 163 840 requests 921 -> 731 us (more gathers in flight per CU); the 4096 launch, whose wavefronts are all
// resident at four per SIMD anyway, is unchanged (23.9 us either way, same box)
#define NEO_SAMPLE_OCC 5
#endif
// the body of sample_kernel (one wavefront per trajectory, lanes per piece) as a function: also the fallback path of
// sample_chunk_kernel (neo_sample_chunk.hpp)
// (round 5, measured and not adopted -- HISTORY.md: the coefficients loaded in the PIECE layout next to the durations and
//  handed to the sample lanes through an LDS table, to take the coefficient load off the chain "durations -> lane
//  assignment -> coefficients": 28.3 us against 27.9 us per 4096 launch; shared tail lanes, 10 rounds instead of 13 at a
//  fresh guess: 31.1 us, tools/probe/neo_sample_shared.hpp.  Round 6, same verdict -- HISTORY.md round 6 (1): the samples as ONE
//  sequence dealt round-robin to the lanes with a candidate list, tools/probe/seq/; floor / clamp / brick address as single
//  instructions through inline assembly: 8 % FEWER vector instructions and 10 % slower, 26.3 against 23.8 us)
// IO: element type of the coefficient / partials buffers (double: neo_sampled_terms_batch[_dev]; float: the _f32 entry
// points of the fp32 sampling path, round 6: half the operand bytes and no conversions)
template <int D, typename Real, class MapT, class LookupT, typename IO = double>
__device__ __forceinline__ void sample_wave_per_piece(int b, int M, const DevParams &prm, const MapT &map,
                                                      const IO *__restrict__ coeffs, const double *__restrict__ ts,
                                                      double *__restrict__ costs2, IO *__restrict__ grad_C,
                                                      IO *__restrict__ grad_T, int *seg, Real *rows) {
  typedef IO IOPair __attribute__((ext_vector_type(2)));
  const int lane = lane_id();
  // lanes in proportion to the pieces' sample counts, as in the fused kernels
  const double Tp = lane < M ? ts[(size_t)b * M + lane] : 1.0;
  const int ns_p = lane < M ? (int)(Tp / prm.delta_t) : 0;
  const SampleLanes sl = balanced_sample_lanes(M, ns_p, seg);
  const int piece = sl.piece, r = sl.r;
  const bool act = sl.act;
  const double T = act ? ts[(size_t)b * M + piece] : 1.0;
  const int ns = act ? (int)(T / prm.delta_t) : 0;
  Real c[6][D], gC[6][D], gT;
  {
    // the 6*D elements of a piece are contiguous and pair-aligned (6*D is even)
    const IOPair *src = reinterpret_cast<const IOPair *>(coeffs + ((size_t)b * 6 * M + 6 * (act ? piece : 0)) * D);
#pragma unroll
    for (int q = 0; q < 3 * D; ++q) {
      const IOPair v = src[q];
      const int e0 = 2 * q, e1 = 2 * q + 1;
      c[e0 / D][e0 % D] = act ? (Real)v.x : Real(0);
      c[e1 / D][e1 % D] = act ? (Real)v.y : Real(0);
    }
  }
  double cf, ck;
  LookupT lk(map);
  minco_sample<Real, D, LookupT, NEO_SAMPLE_U, true>(M, sl, ns, c, prm, lk, gC, gT, cf, ck, sizeof(Real) == 4 ? rows : nullptr);
  if (act && r == 0) {
    IOPair *dst = reinterpret_cast<IOPair *>(grad_C + ((size_t)b * 6 * M + 6 * piece) * D);
#pragma unroll
    for (int q = 0; q < 3 * D; ++q) {
      const int e0 = 2 * q, e1 = 2 * q + 1;
      dst[q] = IOPair{(IO)gC[e0 / D][e0 % D], (IO)gC[e1 / D][e1 % D]};
    }
    grad_T[(size_t)b * M + piece] = (IO)gT;
  }
  if (lane < M && ns_p == 0) {
    // a piece shorter than delta_t has no sample and no sample lane: its partials are zeros (the planner's durations
    // never are -- T > T_min = 5 delta_t --, a caller of neo_sampled_terms_batch may pass any; found by
    // tests/test_gpu_parity.py::test_sampled_terms_on_ragged_durations: the rows were left as the caller's buffer had them)
    IOPair *dst = reinterpret_cast<IOPair *>(grad_C + ((size_t)b * 6 * M + 6 * lane) * D);
#pragma unroll
    for (int q = 0; q < 3 * D; ++q) dst[q] = IOPair{IO(0), IO(0)};
    grad_T[(size_t)b * M + lane] = IO(0);
  }
  if (lane == 0) {
    costs2[(size_t)b * 2 + 0] = cf;
    costs2[(size_t)b * 2 + 1] = ck;
  }
}

template <int D, typename Real, class MapT, class LookupT, typename IO = double>
__global__ __launch_bounds__(kWave, sizeof(Real) == 4 ? NEO_SAMPLE_OCC : 2) void sample_kernel(int B, int M, DevParams prm, MapT map,
                                                                                  const IO *__restrict__ coeffs,
                                                                                  const double *__restrict__ ts,
                                                                                  double *__restrict__ costs2,
                                                                                  IO *__restrict__ grad_C,
                                                                                  IO *__restrict__ grad_T,
                                                                                  const int *__restrict__ order) {
  if ((int)blockIdx.x >= B) return;
  // workgroup i runs on XCD i mod 8 (round-robin dispatch) and each XCD has its own 4 MB L2: `order` lets the caller
  // hand every XCD requests that fly through the same part of the field (BatchPlanner.spatial_order); results stay in
  // the caller's order
  const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
  __shared__ int seg[kWave];
  // rows of the per-piece fold (fp32 sampling, minco_sample)
  __shared__ __attribute__((aligned(16))) Real rows[sizeof(Real) == 4 ? kWave * 8 * D : 4];
  sample_wave_per_piece<D, Real, MapT, LookupT, IO>(b, M, prm, map, coeffs, ts, costs2, grad_C, grad_T, seg, rows);
}

}  // namespace neo
