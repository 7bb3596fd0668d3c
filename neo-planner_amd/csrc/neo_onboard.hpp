// neo_onboard.hpp -- onboard mapping (include/neo_planner.h: neo_onboard_integrate_batch): the depth images of B missions
// into B 2-D log-odds grids of their own, octomap's scan insertion (hit wins over miss within a scan, clamped log-odds)
// projected to the band [z_lo, z_hi].  tests/onboard_oracle_np.py is the same model in NumPy and the tests compare bit
// for bit: the ray directions are the depth camera's fp32 values (neo_depth.hpp) widened to fp64, everything after
// them is fp64 with every operation rounded on its own (contraction is switched off in the kernel), then integers.
//
// One workgroup of 256 lanes per mission.  Every cell a scan can touch lies in a window of side 2 half + 1 cells around
// the eye's cell (OnboardArgs::half, sized by the host from the camera's widest column); the workgroup keeps two bits a
// cell of it in LDS -- passed, hit -- ORs into them with LDS atomics and then updates the window's log-odds and
// occupancy itself: no global atomics, no pass over the whole grid.
//
// The marks factor: the cell of sample n of a ray depends on (column, n) only, whether the sample lies in the band on
// (row, n) only, and the band's samples of a row are a range [a_i, b_i] because t -> ez + t dz_i is monotone operation
// by operation.  So, per chunk of 64 columns:
//   pixels    wavefront w takes rows w, w + 4, ...; lane = column (256-byte rows of depth_m, coalesced).  A pixel ORs
//             the range [a_i, min(b_i, K - 1)] into its column's coverage bitmap, K = #{n : t_n < min(d, range)} from an
//             fp32 estimate corrected against the t table (exact whatever the estimate), and marks its hit cell.  Both
//             are skipped when they repeat the lane's previous row (a vertical face has one depth per column).
//   samples   (column, n) pairs dealt to the 256 lanes: a covered sample's cell gets its passed bit.
// Then one pass over the window's cells: hit -> min(L0 + hit, hi); passed only -> max(L0 + miss, lo).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/neo_planner.h"
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kOnboardThreads = 256;
constexpr int kOnboardCols = 64;                 // columns a chunk: one per lane
constexpr int kOnboardWaves = kOnboardThreads / kOnboardCols;
constexpr int kOnboardUnknown = -128;            // the log-odds byte of a cell never updated
constexpr size_t kOnboardLds = 64 * 1024 - 64;   // dynamic LDS a workgroup may ask for (the kernel has one static word)

struct OnboardArgs {
  LaunchList list;          // the missions of the launch (neo_launch_list.hpp)
  const float *depth_m;     // [list.n][H][W], by launch position
  const double *pose;       // [list.n][5], by launch position
  int W, H;
  double focal;
  int grid_w, grid_h;
  double res;
  const double *origins;    // [B][2]
  double range, z_lo, z_hi;
  int l_hit, l_miss, l_lo, l_hi;
  int N;                    // samples a ray: ceil(range / (res / 2))
  int half;                 // the window reaches `half` cells from the eye's cell
  int8_t *logodds, *occupancy;  // [B][grid_h][grid_w]
  int *changed;             // [B]
};

// dynamic LDS of a launch, in bytes: the window's marks, the t table, the coverage bitmaps of a chunk, the chunk's
// directions, and per row dz and the band's sample range
__host__ __device__ inline size_t onboard_mark_words(int half) {
  const size_t side = 2 * (size_t)half + 1;
  return (side * side + 15) / 16;
}
__host__ __device__ inline int onboard_cov_words(int N) { return (N + 31) / 32; }
__host__ __device__ inline size_t onboard_lds_bytes(int half, int N, int H) {
  return (size_t)N * 8 + (size_t)kOnboardCols * 16 + (size_t)H * 8 + onboard_mark_words(half) * 4 +
         (size_t)onboard_cov_words(N) * kOnboardCols * 4 + (size_t)H * 4;
}

// flat index of the point's cell in the window, or -1: outside the grid (the model's rule) or outside the window (never
// for a unit heading: the bound of memory safety)
struct OnboardGeom {
  double ox, oy, res;
  int grid_w, grid_h, wx0, wy0, side;
  __device__ __forceinline__ int window_cell(double px, double py) const {
#pragma clang fp contract(off)
    const double rx = px - ox, ry = py - oy;
    const double fx = rx / res, fy = ry / res;
    if (!(fx >= 0.0 && fy >= 0.0 && fx < (double)grid_w && fy < (double)grid_h)) return -1;
    const int lx = (int)fx - wx0, ly = (int)fy - wy0;
    if (lx < 0 || ly < 0 || lx >= side || ly >= side) return -1;
    return ly * side + lx;
  }
};

__device__ __forceinline__ void onboard_mark(unsigned *marks, int cell, unsigned bit) {
  const unsigned m = bit << ((cell & 15) * 2);
  unsigned *w = marks + (cell >> 4);
  if (!(*w & m)) atomicOr(w, m);  // (most marks repeat one already set)
}

__global__ __launch_bounds__(kOnboardThreads) void onboard_integrate_kernel(OnboardArgs a) {
#pragma clang fp contract(off)  // every operation rounded on its own, as the NumPy model's are
  extern __shared__ __attribute__((aligned(16))) unsigned char onboard_lds[];
  __shared__ int s_changed;
  const int t = threadIdx.x, lane = t & (kOnboardCols - 1), wave = t / kOnboardCols;
  const int i_launch = blockIdx.x;
  const int b = a.list.request(i_launch);  // (workgroup-uniform)
  if (b < 0) return;

  const int N = a.N, H = a.H, W = a.W;
  const int side = 2 * a.half + 1;
  const int nmark = (int)onboard_mark_words(a.half), ncw = onboard_cov_words(N);
  double *tt = reinterpret_cast<double *>(onboard_lds);                  // [N] sample distances
  double *cdx = tt + N, *cdy = cdx + kOnboardCols;                       // [64] each: the chunk's directions
  double *rdz = cdy + kOnboardCols;                                      // [H]
  unsigned *marks = reinterpret_cast<unsigned *>(rdz + H);               // [nmark]: 2 bits a window cell
  unsigned *cov = marks + nmark;                                         // [ncw][64] coverage words, lane-minor
  unsigned *rab = cov + (size_t)ncw * kOnboardCols;                      // [H]: a | b << 16, or a > b for none

  const double *ps = a.pose + (size_t)i_launch * 5;
  const double ex = ps[0], ey = ps[1], ez = ps[2];
  const float c = (float)ps[3], s = (float)ps[4];
  OnboardGeom g;
  g.ox = a.origins[(size_t)b * 2], g.oy = a.origins[(size_t)b * 2 + 1], g.res = a.res;
  g.grid_w = a.grid_w, g.grid_h = a.grid_h, g.side = side;
  // the eye's cell (may lie outside the grid); an eye nowhere near the grid, or not a number, marks nothing
  const double erx = ex - g.ox, ery = ey - g.oy;
  const double efx = floor(erx / g.res), efy = floor(ery / g.res);
  const bool eye_ok = fabs(efx) < 1.0e9 && fabs(efy) < 1.0e9;
  g.wx0 = eye_ok ? (int)efx - a.half : 0;
  g.wy0 = eye_ok ? (int)efy - a.half : 0;

  if (t == 0) s_changed = 0;
  for (int k = t; k < nmark; k += kOnboardThreads) marks[k] = 0u;
  const double hstep = a.res / 2.0;
  for (int n = t; n < N; n += kOnboardThreads) tt[n] = (double)n * hstep;
  __syncthreads();
  // ---- rows: dz and the range of samples inside the band
  for (int i = t; i < H; i += kOnboardThreads) {
    const double num = (double)i - (double)(H - 1) / 2.0;
    const float v = (float)(num / a.focal);
    const double dz = (double)(-v);
    int lo = N, hi = -1;
    for (int n = 0; n < N; ++n) {
      const double zt = tt[n] * dz;
      const double z = ez + zt;
      if (a.z_lo <= z && z <= a.z_hi) {
        lo = n < lo ? n : lo;
        hi = n;
      }
    }
    rdz[i] = dz;
    rab[i] = (unsigned)lo | ((unsigned)(hi + 1) << 16);  // [lo, hi + 1): N <= 32767
  }
  const float inv_h = (float)(1.0 / hstep);
  const float *img = a.depth_m + (size_t)i_launch * H * W;

  for (int j0 = 0; eye_ok && j0 < W; j0 += kOnboardCols) {
    __syncthreads();  // the rows' tables; the previous chunk's samples pass
    for (int k = t; k < ncw * kOnboardCols; k += kOnboardThreads) cov[k] = 0u;
    const int j = j0 + lane;
    double dxj = 0.0, dyj = 0.0;
    if (j < W) {
      const double num = (double)j - (double)(W - 1) / 2.0;
      const float u = (float)(num / a.focal);
      const float us = u * s;
      const float dxf = c + us;
      const float uc = u * c;
      const float dyf = s - uc;
      dxj = (double)dxf, dyj = (double)dyf;
    }
    if (wave == 0) cdx[lane] = dxj, cdy[lane] = dyj;
    __syncthreads();
    // ---- pixels
    if (j < W) {
      float d_prev = __builtin_nanf("");
      int K = 0;
      unsigned span_prev = 0xffffffffu;
      int hit_cell = -1;
      for (int i = wave; i < H; i += kOnboardWaves) {
        const float df = img[(size_t)i * W + j];
        if (!(df == df)) continue;  // NaN marks nothing
        const double d = (double)df;
        if (df != d_prev) {
          d_prev = df;
          const double m = d < a.range ? d : a.range;
          // K = #{n : t_n < m}
          const float est = (float)m * inv_h;
          K = est > 0.0f ? (est < (float)N ? (int)est : N) : 0;
          while (K < N && tt[K] < m) ++K;
          while (K > 0 && !(tt[K - 1] < m)) --K;
          const double hx = d * dxj, hy = d * dyj;
          hit_cell = d < a.range ? g.window_cell(ex + hx, ey + hy) : -1;
        }
        const unsigned ab = rab[i];
        const int lo = (int)(ab & 0xffffu);
        int hi = (int)(ab >> 16);  // exclusive
        hi = hi < K ? hi : K;
        if (lo < hi) {
          const unsigned span = (unsigned)lo | ((unsigned)hi << 16);
          if (span != span_prev) {
            span_prev = span;
            for (int w = lo >> 5; w <= (hi - 1) >> 5; ++w) {
              const int f0 = lo - w * 32, f1 = hi - w * 32;  // bits [max(f0, 0), min(f1, 32))
              const unsigned from = f0 > 0 ? (0xffffffffu << f0) : 0xffffffffu;
              const unsigned upto = f1 < 32 ? ((1u << f1) - 1u) : 0xffffffffu;
              const unsigned bits = from & upto;
              unsigned *cw = cov + (size_t)w * kOnboardCols + lane;
              if ((*cw & bits) != bits) atomicOr(cw, bits);
            }
          }
        }
        if (hit_cell >= 0) {
          const double zt = d * rdz[i];
          const double z = ez + zt;
          if (a.z_lo <= z && z <= a.z_hi) onboard_mark(marks, hit_cell, 2u);
        }
      }
    }
    __syncthreads();
    // ---- samples: the covered (column, n) pairs of the chunk
    const int ncol = W - j0 < kOnboardCols ? W - j0 : kOnboardCols;
    if (lane < ncol) {
      const double dxs = cdx[lane], dys = cdy[lane];
      for (int n = wave; n < N; n += kOnboardWaves) {
        if (!((cov[(size_t)(n >> 5) * kOnboardCols + lane] >> (n & 31)) & 1u)) continue;
        const double tn = tt[n];
        const double sx = tn * dxs, sy = tn * dys;
        const int cell = g.window_cell(ex + sx, ey + sy);
        if (cell >= 0) onboard_mark(marks, cell, 1u);
      }
    }
  }
  __syncthreads();
  // ---- the window's cells: log-odds, occupancy, whether the occupied set changed
  int chg = 0;
  const size_t gbase = (size_t)b * a.grid_w * a.grid_h;
  for (int k = t; eye_ok && k < side * side; k += kOnboardThreads) {
    const unsigned mk = (marks[k >> 4] >> ((k & 15) * 2)) & 3u;
    if (!mk) continue;
    const int ly = k / side, lx = k - ly * side;
    const size_t at = gbase + (size_t)(g.wy0 + ly) * a.grid_w + (g.wx0 + lx);  // inside the grid: window_cell checked
    const int L = a.logodds[at];
    const int L0 = L == kOnboardUnknown ? 0 : L;
    int Ln;
    if (mk & 2u) {
      Ln = L0 + a.l_hit;
      Ln = Ln < a.l_hi ? Ln : a.l_hi;
    } else {
      Ln = L0 + a.l_miss;
      Ln = Ln > a.l_lo ? Ln : a.l_lo;
    }
    const bool was = L != kOnboardUnknown && L >= 0, is = Ln >= 0;
    chg |= was != is;
    a.logodds[at] = (int8_t)Ln;
    a.occupancy[at] = (int8_t)(is ? 100 : 0);
  }
  if (chg) s_changed = 1;  // (every writer stores the same value)
  __syncthreads();
  if (t == 0) a.changed[b] = s_changed;
}

}  // namespace neo
