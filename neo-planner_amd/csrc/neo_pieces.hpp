// neo_pieces.hpp -- the piece table: a packed trajectory x as coefficients per piece and cumulative piece times, and the
// sample rows read off it.  One wavefront per trajectory.  What get_full_state_cmd (traj_utils.py:85-195) does, for
//
//   traj_state_kernel    the rows themselves (neo_eval_traj_batch)                    below, launched from neo_disp_audit.hip
//   audit_kernel         the flight metric over the rows                              neo_audit.hpp
//   fleet_splice_kernel  the rows into a mission's command array                      neo_fleet.hpp
//
// The three compute the same bits: one solve, one sample count, one set of row expressions (compiled with the units'
// -ffp-contract=on and no pragma: a multiply-add is fused where the expression has one, whoever calls).  Nothing of the
// optimiser is included: the solve is minco_forward on a Traj of its own (neo_device.hpp).
#pragma once
#include "neo_device.hpp"

namespace neo {

// the wavefront's LDS: a __shared__ object of the kernel, declared with NEO_PIECE_LDS.  16-byte aligned with the
// coefficients first: the row expressions read them with 16-byte LDS accesses whose immediate offsets reach a whole piece
// (the alignment is the variable's, not the type's: the type's would pad the odd number of doubles by 8 bytes)
#define NEO_PIECE_LDS(D, name) __shared__ __attribute__((aligned(16))) PieceLds<D> name
template <int D>
struct PieceLds {
  double cs[kWave * 6 * D];   // coefficients [M][6][D]
  double xs[kSlots * kWave];  // staging of x in the FLAT layout
  double tcum[kWave + 1];     // start time of piece p; tcum[M]: the duration
};

template <int D>
struct PieceTable {
  PieceLds<D> &lds;
  const int M;
  double total;  // duration: tcum[M]

  __device__ PieceTable(PieceLds<D> &l, int M_) : lds(l), M(M_) {}

  // x, head and tail of request b -> cs, tcum and total.  Returns minco_forward's status (not 0: nothing here is usable;
  // what a kernel then reports is its own).  Called by the whole wavefront.  x goes from global memory straight into the
  // staging, n <= kSlots * kWave.
  __device__ __forceinline__ int solve(int b, const DevParams &prm, const double *__restrict__ x,
                                       const double *__restrict__ head, const double *__restrict__ tail) {
    Traj<D> t;
    load_boundary(t, head + (size_t)b * 3 * D, tail + (size_t)b * 3 * D, M);
    const int n = t.n, lane = lane_id();
#pragma unroll
    for (int k = 0; k < kSlots; ++k)
      if (k * kWave + lane < n) lds.xs[k * kWave + lane] = x[(size_t)b * n + k * kWave + lane];
    lds_wave_sync();
    // minco_forward's inputs, lane = piece: tau and the positions at the piece's two ends (what DevBackend::scatter_x
    // reads off its staging; shared with it, the call changed an instruction of the fused fp32 kernels, so it is restated)
    const double *xn = lds.xs;
    const int p = opaque(lane);  // (as there; with the plain lane traj_state_kernel<3> takes two registers more)
    // (the selects may read for inactive lanes too: up to element D (M - 1) + 62 of xs, beyond the n written ones -- in
    // bounds because xs has kSlots * kWave elements, whatever n is; those values are discarded)
    const bool act = p < M;
    t.tau = act ? xn[t.nq + p] : 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      t.P0[d] = (p == 0 || !act) ? t.head[d] : xn[d * (M - 1) + (p > 0 ? p - 1 : 0)];
      t.P1[d] = (p >= M - 1) ? t.tail[d] : xn[d * (M - 1) + p];
    }
    double energy, tsum;
    const int st = minco_forward<D>(t, prm, energy, tsum);
    if (st != 0) return st;
    if (lane < M) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int d = 0; d < D; ++d) lds.cs[(lane * 6 + k) * D + d] = t.c[k][d];
    }
    // sequential prefix sums like Python's sum(ts[:k]) (traj_utils.py:98-101)
    if (lane == 0) lds.tcum[0] = 0.0;
    for (int pce = 0; pce < M; ++pce) {
      const double Tp = rdlane(t.T, pce);
      if (lane == 0) lds.tcum[pce + 1] = lds.tcum[pce] + Tp;
    }
    __syncthreads();
    total = lds.tcum[M];
    return 0;
  }

  // len(np.arange(0, total, step)), as a double
  __device__ __forceinline__ double sample_count_d(double step) const { return ceil(total / step); }
  // ... as an int; false for a duration that is not finite (or beyond 2^30 samples)
  __device__ __forceinline__ bool sample_count(double step, int &cnt) const {
    const double cnt_d = sample_count_d(step);
    if (!(cnt_d >= 0.0 && cnt_d <= (double)(1 << 30))) return false;
    cnt = (int)cnt_d;
    return true;
  }
  // time of sample k
  __device__ __forceinline__ double time_of(int k, double step) const {
    const double tt = (double)k * step;
    return tt > total ? total : tt;
  }
  // the piece of time tt, searched forward from pc
  __device__ __forceinline__ int seek(int pc, double tt) const {
    while (pc < M - 1 && lds.tcum[pc + 1] < tt) ++pc;
    return pc;
  }
  // position, velocity and acceleration at time tt of piece pc
  __device__ __forceinline__ void state(int pc, double tt, double (&p)[D], double (&v)[D], double (&a)[D]) const {
    const double *cs = lds.cs;
    const double T = tt - lds.tcum[pc];
    const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double c0 = cs[(pc * 6 + 0) * D + d], c1 = cs[(pc * 6 + 1) * D + d], c2 = cs[(pc * 6 + 2) * D + d];
      const double c3 = cs[(pc * 6 + 3) * D + d], c4 = cs[(pc * 6 + 4) * D + d], c5 = cs[(pc * 6 + 5) * D + d];
      p[d] = c0 + c1 * T + c2 * T2 + c3 * T3 + c4 * T4 + c5 * T5;
      v[d] = c1 + 2.0 * c2 * T + 3.0 * c3 * T2 + 4.0 * c4 * T3 + 5.0 * c5 * T4;
      a[d] = 2.0 * c2 + 6.0 * c3 * T + 12.0 * c4 * T2 + 20.0 * c5 * T3;
    }
  }
};

// get_full_state_cmd (traj_utils.py:85-195): one wavefront per trajectory solves the coefficients, then its lanes walk the
// sample times.  count = -1: the solve failed.
template <int D>
__global__ __launch_bounds__(kWave) void traj_state_kernel(int B, int M, DevParams prm, const double *__restrict__ x,
                                                            const double *__restrict__ head,
                                                            const double *__restrict__ tail, double hz, int K,
                                                            double *__restrict__ state, int *__restrict__ count) {
  NEO_PIECE_LDS(D, lds);
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  PieceTable<D> pt(lds, M);
  if (pt.solve(b, prm, x, head, tail) != 0) {
    if (lane == 0) count[b] = -1;
    return;
  }
  const double step = 1.0 / hz;
  // (not sample_count: this kernel has no refusal for a duration that is not finite -- the conversion saturates, a NaN
  // counts no samples -- and keeps that behaviour)
  const int cnt = (int)pt.sample_count_d(step);
  if (lane == 0) count[b] = cnt;
  for (int k = lane; k < K; k += kWave) {
    double *out = state + ((size_t)b * K + k) * 3 * D;
    if (k >= cnt) {
#pragma unroll
      for (int q = 0; q < 3 * D; ++q) out[q] = 0.0;
      continue;
    }
    const double tt = pt.time_of(k, step);
    const int pc = pt.seek(0, tt);
    double pos[D], vel[D], acc[D];
    pt.state(pc, tt, pos, vel, acc);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      out[0 * D + d] = pos[d];
      out[1 * D + d] = vel[d];
      out[2 * D + d] = acc[d];
    }
  }
}

}  // namespace neo
