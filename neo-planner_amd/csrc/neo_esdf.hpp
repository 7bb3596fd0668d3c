// neo_esdf.hpp -- the map kernels: building, packing and querying the distance fields
//
//   edt_* / edt2_*_bf, gradient_pack   ESDF.occupancy_map_cb (2-D)    (map_server/esdf.py:11-33)
//   edt3_x / edt3_xv / edt3_line*      the exact 3-D EDT, three separable passes
//   pack2d, pack3d_*                   precomputed fields into the records / the four 3-D layouts
//   query_kernel                       ESDF point lookups              (map_server/esdf.py:53-82)
//
// Launched from neo_disp_esdf.hip; the C ABI (neo_abi.hip) checks arguments and carves the scratch.
#pragma once
#include "neo_wave.hpp"

namespace neo {

// ---- ESDF construction (esdf.py:23-33) ------------------------------------
// exact Euclidean distance transform of the free cells to the nearest occupied cell, two
// separable passes over integer squared distances (Felzenszwalb & Huttenlocher lower envelope),
// then sqrt * resolution and numpy.gradient with unit spacing.
// Every 2-D kernel takes a map dimension in its grid (blockIdx.y of the sweeps and of gradient_pack, blockIdx.z of the
// exhaustive form): map k's occupancy and work arrays lie k maps further on (neo_esdf_build_2d_batch_dev); a launch for
// one map has one block there.
constexpr int kEdtInf = 1 << 28;

__global__ void edt_columns_kernel(const int8_t *__restrict__ occ, int W, int H, int *__restrict__ g) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= W) return;
  occ += (size_t)blockIdx.y * W * H;
  g += (size_t)blockIdx.y * W * H;
  int d = kEdtInf;
  for (int y = 0; y < H; ++y) {
    d = (occ[(size_t)y * W + x] == 100) ? 0 : (d >= kEdtInf ? kEdtInf : d + 1);
    g[(size_t)y * W + x] = d;
  }
  d = kEdtInf;
  for (int y = H - 1; y >= 0; --y) {
    d = (occ[(size_t)y * W + x] == 100) ? 0 : (d >= kEdtInf ? kEdtInf : d + 1);
    const int cur = g[(size_t)y * W + x];
    g[(size_t)y * W + x] = cur < d ? cur : d;
  }
}

// one thread per row; v/z scratch rows live in global memory (W ints / W+1 doubles per row)
__global__ void edt_rows_kernel(const int *__restrict__ g, int W, int H, double res, int *__restrict__ vbuf,
                                double *__restrict__ zbuf, double *__restrict__ dist) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= H) return;
  const size_t map0 = (size_t)blockIdx.y * W * H;
  const int *f = g + map0 + (size_t)y * W;
  int *v = vbuf + map0 + (size_t)y * W;
  double *z = zbuf + (size_t)blockIdx.y * H * (W + 1) + (size_t)y * (W + 1);
  int k = -1;
  for (int q = 0; q < W; ++q) {
    if (f[q] >= kEdtInf) continue;
    const double fq = (double)f[q] * (double)f[q] + (double)q * q;
    double s = 0.0;
    while (k >= 0) {
      const int p = v[k];
      const double fp = (double)f[p] * (double)f[p] + (double)p * p;
      s = (fq - fp) / (2.0 * q - 2.0 * p);
      if (s <= z[k]) {
        --k;
      } else {
        break;
      }
    }
    ++k;
    v[k] = q;
    z[k] = (k == 0) ? -1.0e300 : s;
    z[k + 1] = 1.0e300;
  }
  double *out = dist + map0 + (size_t)y * W;
  if (k < 0) {
    // no occupied cell in the whole map: scipy.ndimage.distance_transform_edt then measures to a
    // virtual background cell at (row -1, column 0); the reference inherits that (esdf.py:29)
    for (int q = 0; q < W; ++q) {
      const long long sq = (long long)(y + 1) * (y + 1) + (long long)q * q;
      out[q] = sqrt((double)sq) * res;
    }
    return;
  }
  int j = 0;
  for (int q = 0; q < W; ++q) {
    while (z[j + 1] < (double)q) ++j;
    const long long p = v[j];
    const long long dq = q - p;
    const long long sq = dq * dq + (long long)f[p] * f[p];
    out[q] = sqrt((double)sq) * res;
  }
}

// Small maps (the reference's 300 x 300): the same two passes by exhaustive minimisation, one thread per cell --
// W*H*(W+H) integer operations (54 M at 300 x 300) instead of a sequential sweep per line.  Exact integer
// squared distances, hence the same doubles as the sweeps above (and as SciPy).
__global__ void edt2_columns_bf_kernel(const int8_t *__restrict__ occ, int W, int H, int *__restrict__ g) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  occ += (size_t)blockIdx.z * W * H;
  g += (size_t)blockIdx.z * W * H;
  int d = kEdtInf;
  for (int q = 0; q < H; ++q) {
    const int dq = q > y ? q - y : y - q;
    if (occ[(size_t)q * W + x] == 100 && dq < d) d = dq;
  }
  g[(size_t)y * W + x] = d;
}
__global__ void edt2_rows_bf_kernel(const int *__restrict__ g, int W, int H, double res, double *__restrict__ dist) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const size_t map0 = (size_t)blockIdx.z * W * H;
  const int *f = g + map0 + (size_t)y * W;
  long long best = -1;
  for (int p = 0; p < W; ++p) {
    const int fp = f[p];
    if (fp >= kEdtInf) continue;
    const long long dq = x - p;
    const long long sq = dq * dq + (long long)fp * fp;
    if (best < 0 || sq < best) best = sq;
  }
  // no occupied cell in the whole map: SciPy's virtual background cell at (row -1, column 0), see edt_rows_kernel
  if (best < 0) best = (long long)(y + 1) * (y + 1) + (long long)x * x;
  dist[map0 + (size_t)y * W + x] = sqrt((double)best) * res;
}

// ---- 3-D exact EDT (north-star scenes): three separable passes over integers, so the result equals
// scipy.ndimage.distance_transform_edt exactly; the final sqrt * resolution is rounded to fp32.
//   pass X  distance in cells to the nearest occupied voxel of the same x-row: one wavefront per row, two wave scans
//           ("last occupied index at or before me" from the left, the mirror image from the right) -> uint16
//   pass Y  squared distance in the (x, y) plane, D(p) = min_q gx(q)^2 + (p - q)^2 along y; pass Z the same along z on
//           the plane distances, then sqrt * res -> fp32.  The (leftmost) minimiser q*(p) never moves left when p
//           moves right (the cost is totally monotone for ANY f), so the line is solved by monotone minima: the two end
//           points by a full scan, then the midpoint of every gap -- its minimiser lies between its neighbours' -- at
//           spacings 2^k .. 1.  Each level visits at most n + (#points) candidates: O(n log n) comparisons for a line,
//           about a dozen per voxel, whatever the distances are (an outward search from q = p, stopped at d^2 >= best,
//           visits as many candidates as the voxel's distance in cells: 4.2 ms for the y pass of a 300^3 forest scene,
//           most of whose volume is far from everything).  A block holds TX x-columns by the whole line in LDS
//           (squared values + minimisers, 6 bytes a voxel); work items (point, column) are dealt to its 256 threads.
// (Round 1-3 form: one thread per line running the lower-envelope sweep with its stacks in global memory -- 0.75 +
//  1.24 + 2.73 ms for 300^3 and 540 MB of scratch; these kernels need none.)  Dimensions up to 4096 per axis.
constexpr int kXInf = 0x7fff;

__global__ __launch_bounds__(256) void edt3_x_kernel(const uint8_t *__restrict__ occ, int nx, size_t rows,
                                                     uint16_t *__restrict__ gx) {
  extern __shared__ uint16_t x_left[];  // [4][nx]
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const uint8_t *o = occ + row * nx;
  uint16_t *left = x_left + (size_t)wave * nx;
  int carry = 0;  // (index + 1) of the last occupied voxel so far, 0 = none
  for (int c0 = 0; c0 < nx; c0 += kWave) {
    const int idx = c0 + lane;
    const int v = (idx < nx && o[idx]) ? idx + 1 : 0;
    const int s = max(wave_scan_max_nonneg(v), carry);
    if (idx < nx) left[idx] = (uint16_t)(s ? min(idx + 1 - s, kXInf) : kXInf);
    carry = rdlane(s, kWave - 1);
  }
  lds_wave_sync();
  carry = 0;  // nx - index of the nearest occupied voxel to the right so far (>= 1), 0 = none
  const int nchunk = (nx + kWave - 1) / kWave;
  for (int c = nchunk - 1; c >= 0; --c) {
    const int idx = c * kWave + (kWave - 1 - lane);  // lanes walk the chunk from its right end
    const int v = (idx < nx && o[idx]) ? nx - idx : 0;
    const int s = max(wave_scan_max_nonneg(v), carry);
    if (idx < nx) {
      const int right = s ? (nx - s) - idx : kXInf;
      gx[row * nx + idx] = (uint16_t)min(min((int)left[idx], right), kXInf);
    }
    carry = rdlane(s, kWave - 1);
  }
}

// The same pass with V = 8 or 16 consecutive voxels per lane (rows of up to 64 V voxels, nx a multiple of four): ONE
// pair of 4-byte loads per lane instead of a byte per lane and chunk, one prefix and one suffix scan per row, the
// distances of the lane's voxels by two sweeps in registers, 8-byte stores (round 4: 69 -> see DESIGN.md at 300^3).
template <int V>
__global__ __launch_bounds__(256) void edt3_xv_kernel(const uint8_t *__restrict__ occ, int nx, size_t rows,
                                                      uint16_t *__restrict__ gx) {
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const uint32_t *o = reinterpret_cast<const uint32_t *>(occ + row * nx);
  const int idx0 = lane * V;
  uint32_t w[V / 4];
#pragma unroll
  for (int k = 0; k < V / 4; ++k) w[k] = idx0 + 4 * k < nx ? o[(idx0 >> 2) + k] : 0u;
  // bit k of m: voxel idx0 + k is occupied
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < V / 4; ++k) {
    const uint32_t nz = (((w[k] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w[k]) & 0x80808080u;  // bit 7 of every non-zero byte
    m |= (((nz >> 7) & 1u) | ((nz >> 14) & 2u) | ((nz >> 21) & 4u) | ((nz >> 28) & 8u)) << (4 * k);
  }
  // nearest occupied voxel before the lane's group (index + 1, 0 = none) and after it (nx - index, 0 = none)
  const int last_in = m ? idx0 + (31 - __clz((int)m)) + 1 : 0;
  const int first_in = m ? nx - (idx0 + __ffs((int)m) - 1) : 0;
  const int pre = wave_scan_max_nonneg(last_in);
  int before = __shfl_up(pre, 1, kWave);
  before = lane == 0 ? 0 : before;
  const int rev = __shfl(first_in, kWave - 1 - lane, kWave);
  const int suf = wave_scan_max_nonneg(rev);  // (in reversed lane order)
  int after = __shfl(suf, kWave - 2 - lane >= 0 ? kWave - 2 - lane : 0, kWave);
  after = lane == kWave - 1 ? 0 : after;
  int left[V];
  int last = before;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if ((m >> k) & 1u) last = idx0 + k + 1;
    left[k] = last ? idx0 + k + 1 - last : kXInf;
  }
  int nxt = after;
  uint16_t out[V];
#pragma unroll
  for (int k = V - 1; k >= 0; --k) {
    if ((m >> k) & 1u) nxt = nx - (idx0 + k);
    const int right = nxt ? (nx - nxt) - (idx0 + k) : kXInf;
    out[k] = (uint16_t)min(min(left[k], right), kXInf);
  }
  uint2 *dst = reinterpret_cast<uint2 *>(gx + row * nx + idx0);
#pragma unroll
  for (int k = 0; k < V / 4; ++k)
    if (idx0 + 4 * k < nx)
      dst[k] = make_uint2((uint32_t)out[4 * k] | ((uint32_t)out[4 * k + 1] << 16), (uint32_t)out[4 * k + 2] | ((uint32_t)out[4 * k + 3] << 16));
}

constexpr int kSqInf = 1 << 28;

// SrcT = uint16_t: plane distances from row distances (squared while the tile is loaded); uint32_t: volume distances
// from plane distances.  `stride_line` = elements between consecutive voxels of a line, `stride_slab` = elements
// between the slabs a block row works on (grid.y), nline = voxels per line.  Dynamic LDS: nline * TX * 4 (uint16 source) or 6 bytes.
constexpr int kEdtThreads = 256;  // threads of a line-pass block
template <typename SrcT, int TX, bool FINAL>
__global__ __launch_bounds__(kEdtThreads) void edt3_line_kernel(const SrcT *__restrict__ src, int nx, int nline, size_t stride_line,
                                                        size_t stride_slab, double res, uint32_t *__restrict__ out_sq,
                                                        float *__restrict__ out_dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tile_raw[];
  // [nline][TX] values: row distances as they are (uint16, squared when read: half the LDS, twice the blocks per CU) or
  // plane distances (already squared); then [nline][TX] minimisers
  using FT = std::conditional_t<sizeof(SrcT) == 2, uint16_t, int>;
  FT *f = reinterpret_cast<FT *>(tile_raw);
  uint16_t *am = reinterpret_cast<uint16_t *>(tile_raw + (size_t)nline * TX * sizeof(FT));
  auto val = [&](int i) -> int {
    const int v = (int)f[i];
    if constexpr (sizeof(SrcT) == 2) return v >= kXInf ? kSqInf : v * v;
    return v;
  };
  const int x0 = blockIdx.x * TX;
  const size_t base = (size_t)blockIdx.y * stride_slab;
  for (int i = threadIdx.x; i < nline * TX; i += kEdtThreads) {
    const int q = i / TX, xl = i - q * TX;
    FT v = sizeof(SrcT) == 2 ? (FT)kXInf : (FT)kSqInf;
    if (x0 + xl < nx) v = (FT)src[base + (size_t)q * stride_line + x0 + xl];
    f[i] = v;
  }
  __syncthreads();
  // One level: `npts` points p = p0 + k * dp, each with the minimiser range of its column taken from the neighbours
  // (or the whole line).  While a level has fewer (point, column) items than the block has threads, G = 2 .. 8 threads
  // share an item -- contiguous parts of its range, combined through `part` (leftmost minimum wins: parts in order,
  // strict comparison) -- so that the coarse levels, few points with long ranges, do not run on a handful of threads.
  // leftmost minimiser of f[q] + (p - q)^2 over a <= q <= b: four candidates' LDS reads in flight at a time, compared in
  // order with a strict "<" (kSqInf + 4095^2 < 2^31)
  auto scan = [&](int p, int xl, int a, int b, int &best, int &arg) {
    int q = a;
    for (; q + 3 <= b; q += 4) {
      const int f0 = val(q * TX + xl), f1 = val((q + 1) * TX + xl), f2 = val((q + 2) * TX + xl), f3 = val((q + 3) * TX + xl);
      const int d0 = p - q, d1 = d0 - 1, d2 = d0 - 2, d3 = d0 - 3;
      const int c0 = f0 + d0 * d0, c1 = f1 + d1 * d1, c2 = f2 + d2 * d2, c3 = f3 + d3 * d3;
      if (c0 < best) { best = c0; arg = q; }
      if (c1 < best) { best = c1; arg = q + 1; }
      if (c2 < best) { best = c2; arg = q + 2; }
      if (c3 < best) { best = c3; arg = q + 3; }
    }
    for (; q <= b; ++q) {
      const int dq = p - q, c = val(q * TX + xl) + dq * dq;
      if (c < best) { best = c; arg = q; }
    }
  };
  __shared__ int part_best[kEdtThreads];
  __shared__ int part_arg[kEdtThreads];
  auto level = [&](int npts, int p0, int dp, int S) {
    int G = 1;
    while (G < 8 && npts * TX * G * 2 <= kEdtThreads) G *= 2;
    const int items = npts * TX * G;
    int p = 0, xl = 0, g = 0;
    const bool mine = (int)threadIdx.x < items || G == 1;
    if (G > 1) {
      if (mine) {
        xl = threadIdx.x % TX;
        g = (threadIdx.x / TX) % G;
        p = min(p0 + (int)(threadIdx.x / (TX * G)) * dp, nline - 1);
        const int lo = S ? am[(p - S) * TX + xl] : 0, hi = S ? am[min(p + S, nline - 1) * TX + xl] : nline - 1;
        const int chunk = (hi - lo + G) / G, a = lo + g * chunk, b = min(hi, a + chunk - 1);
        int best = 0x7fffffff, arg = lo;
        scan(p, xl, a, b, best, arg);
        part_best[threadIdx.x] = best;
        part_arg[threadIdx.x] = arg;
      }
      __syncthreads();
      if (mine && g == 0) {
        int best = part_best[threadIdx.x], arg = part_arg[threadIdx.x];
        for (int j = 1; j < G; ++j) {
          const int c = part_best[threadIdx.x + j * TX];
          if (c < best) { best = c; arg = part_arg[threadIdx.x + j * TX]; }
        }
        am[p * TX + xl] = (uint16_t)arg;
      }
    } else {
      for (int it = threadIdx.x; it < items; it += kEdtThreads) {
        const int k = it / TX;
        xl = it - k * TX;
        p = min(p0 + k * dp, nline - 1);
        const int lo = S ? am[(p - S) * TX + xl] : 0, hi = S ? am[min(p + S, nline - 1) * TX + xl] : nline - 1;
        int best = 0x7fffffff, arg = lo;
        scan(p, xl, lo, hi, best, arg);
        am[p * TX + xl] = (uint16_t)arg;
      }
    }
    __syncthreads();
  };
  level(2, 0, nline - 1, 0);  // the two end points: full scans
  int top = 1;
  while (top < nline - 1) top <<= 1;
  for (int S = top >> 1; S >= 1; S >>= 1)
    level((nline - 1 - S + 2 * S - 1) / (2 * S), S, 2 * S, S);  // points p = S + 2 S k < nline - 1
  for (int i = threadIdx.x; i < nline * TX; i += kEdtThreads) {
    const int p = i / TX, xl = i - p * TX;
    if (x0 + xl >= nx) continue;
    const int q = am[i], dq = p - q;
    const int best = min(val(q * TX + xl) + dq * dq, kSqInf);
    const size_t o = base + (size_t)p * stride_line + x0 + xl;
    if constexpr (FINAL) {
      // no occupied voxel at all: keep a large finite distance (scipy's convention there is an artefact of its
      // virtual background voxel; 3-D scenes always contain the ground slab)
      out_dist[o] = (float)(best >= kSqInf ? 1.0e4 : sqrt((double)best) * res);
    } else {
      out_sq[o] = (uint32_t)best;
    }
  }
}

// The same monotone-minima line pass on PACKED KEYS (round 4), for volumes whose squared diagonal leaves room in 31 bits
// (every scene of BASELINE.json: 300^3 needs 28 bits, 600^3 31).  With h(q) = f(q) + q^2 the cost of candidate q at point
// p is f(q) + (p - q)^2 = h(q) - 2 p q + p^2; the tile holds h(q) << qb (the low qb bits are the slot of the minimiser
// found for POINT q, masked off when q is read as a candidate), and
//     key(p, q) = (h(q) << qb) + q * (1 - (p << (qb + 1)))        [= ((cost - p^2) << qb) | q]
// orders the candidates of one point by (cost, q): the leftmost minimiser is ONE v_mad_i32_i24 and half a v_min3_i32 per
// candidate instead of square / add / compare / two selects (the line passes are bound by vector issue: 4.0 k vector
// instructions a wavefront, 72 % of the SIMDs' cycles, `tools/probe/pmc_edt.sh`).  Unreachable voxels enter as
// `big` = nx^2 + ny^2 + nz^2 + 1, above every real squared distance, so a line's minimum is a real candidate whenever it
// has one.  Same levels, same work distribution, bit-equal results (integers).
template <typename SrcT, int TX, bool FINAL>
__global__ __launch_bounds__(kEdtThreads) void edt3_line_keys_kernel(const SrcT *__restrict__ src, int nx, int nline,
                                                                     size_t stride_line, size_t stride_slab, int nslab, double res,
                                                                     int big, int qb, uint32_t *__restrict__ out_sq,
                                                                     float *__restrict__ out_dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tile_raw[];
  static_assert((TX & (TX - 1)) == 0, "TX is a power of two");
  constexpr int LX = TX == 32 ? 5 : (TX == 16 ? 4 : (TX == 8 ? 3 : (TX == 4 ? 2 : 1)));
  int *hk = reinterpret_cast<int *>(tile_raw);  // [nline][TX] keys (and, in their low bits, the minimisers found)
  // the minimiser found for point p lives in the low qb bits of hk[p] (they hold p itself until then, and a candidate's
  // position is added back from its index): 4 bytes a voxel -- 8 workgroups a CU at 300 voxels a line, 4 at 600 (with a
  // separate 2-byte array: 5 and 2; 600^3 5.1 -> 4.0 ms the build).  A candidate's key is masked when it is read.
  const int himask = ~((1 << qb) - 1);
  auto am_get = [&](int i) { return hk[i] & ~himask; };
  auto am_put = [&](int i, int arg) { hk[i] = (hk[i] & himask) | arg; };
#define NEO_EDT_K(x) ((x) & himask)
#define NEO_EDT_NEGP(p) (1 - ((p) << (qb + 1)))  // per unit of q: -(p << (qb + 1)) for the cost, + 1 for q in the low bits
  // 1-D grid, XCD-aware: workgroup b runs on XCD b mod 8; the tiles of one slab share their rows' 128-byte lines (a row
  // of a 16-column tile is 32 or 64 bytes), so a slab's tiles go to ONE XCD, one after the other, and meet in its L2
  const int ntx = (nx + TX - 1) / TX;
  const int bj = blockIdx.x >> 3, slab = (blockIdx.x & 7) + 8 * (bj / ntx);
  if (slab >= nslab) return;
  const int x0 = (bj % ntx) * TX;
  const size_t base = (size_t)slab * stride_slab;
  const int qmask = (1 << qb) - 1;
  // the tile: several loads in flight per thread (one load per thread and trip left the pass waiting on memory latency:
  // 84 of the y pass's 149 us at 300^3 were this loop and the store loop with the levels switched off) -- four
  // neighbouring columns per load where the rows are aligned for it, eight rows per thread in flight
  auto put = [&](int q, int xl, int v, bool in) {
    int c = big;
    if (in) {
      if constexpr (sizeof(SrcT) == 2)
        c = v >= kXInf ? big : v * v;
      else
        c = v >= kSqInf ? big : v;
    }
    hk[q * TX + xl] = ((c + q * q) << qb) | q;
  };
  if (TX >= 4 && ((nx | stride_line | stride_slab) & 3) == 0) {
    struct alignas(4 * sizeof(SrcT)) Vec4 { SrcT v[4]; };
    constexpr int CPR = TX / 4 > 0 ? TX / 4 : 1, RPP = kEdtThreads / CPR;  // threads a row, rows a pass of the block
    const int xl = (threadIdx.x % CPR) * 4, r0 = threadIdx.x / CPR;
    const bool in = x0 + xl < nx;  // (nx is a multiple of four: the four columns are in or out together)
    constexpr int U = 8;
    for (int qa = r0; qa < nline; qa += U * RPP) {
      Vec4 w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = qa + u * RPP;
        if (q < nline && in) w[u] = *reinterpret_cast<const Vec4 *>(src + base + (size_t)q * stride_line + x0 + xl);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = qa + u * RPP;
        if (q < nline) {
#pragma unroll
          for (int e = 0; e < 4; ++e) put(q, xl + e, in ? (int)w[u].v[e] : 0, in);
        }
      }
    }
  } else {
    constexpr int U = 8;
    for (int ia = threadIdx.x; ia < nline * TX; ia += U * kEdtThreads) {
      int v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = ia + u * kEdtThreads, q = i >> LX, xl = i & (TX - 1);
        v[u] = (i < nline * TX && x0 + xl < nx) ? (int)src[base + (size_t)q * stride_line + x0 + xl] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = ia + u * kEdtThreads, q = i >> LX, xl = i & (TX - 1);
        if (i < nline * TX) put(q, xl, v[u], x0 + xl < nx);
      }
    }
  }
  __syncthreads();
  // smallest key of the candidates a <= q <= b of column xl for the point with negP = -(p << (qb + 1)).  (No unrolling
  // beyond the four written out: most ranges of the fine levels hold one to three candidates, and the kernel is bound
  // by the instructions around the loop.)
  auto scan = [&](int negP, int xl, int a, int b, int &best) {
    int q = a;
    const int *h = hk + a * TX + xl;
    int t = __mul24(q, negP);
#pragma clang loop unroll(disable)
    for (; q + 3 <= b; q += 4, h += 4 * TX, t += 4 * negP) {
      const int k0 = NEO_EDT_K(h[0]), k1 = NEO_EDT_K(h[TX]), k2 = NEO_EDT_K(h[2 * TX]), k3 = NEO_EDT_K(h[3 * TX]);
      best = min(min(best, k0 + t), k1 + t + negP);
      best = min(min(best, k2 + t + 2 * negP), k3 + t + 3 * negP);
    }
#pragma clang loop unroll(disable)
    for (; q <= b; ++q, h += TX, t += negP) best = min(best, NEO_EDT_K(h[0]) + t);
  };
  __shared__ int part_key[kEdtThreads];
  const int my_xl = threadIdx.x & (TX - 1), my_k = threadIdx.x >> LX;
  auto level = [&](int npts, int p0, int dp, int S) {
    int G = 1, lg = 0;
    while (G < 8 && npts * TX * G * 2 <= kEdtThreads) G *= 2, ++lg;
    if (G > 1) {
      const int items = npts * TX * G;
      const bool mine = (int)threadIdx.x < items;
      int p = 0, g = 0;
      const int xl = my_xl;
      if (mine) {
        g = my_k & (G - 1);
        p = min(p0 + (int)(threadIdx.x >> (LX + lg)) * dp, nline - 1);
        const int lo = S ? am_get((p - S) * TX + xl) : 0, hi = S ? am_get(min(p + S, nline - 1) * TX + xl) : nline - 1;
        const int chunk = (hi - lo + G) >> lg, a = lo + g * chunk, b = min(hi, a + chunk - 1);
        int best = 0x7fffffff;
        scan(NEO_EDT_NEGP(p), xl, a, b, best);
        part_key[threadIdx.x] = best;
      }
      __syncthreads();
      if (mine && g == 0) {
        int best = part_key[threadIdx.x];
        for (int j = 1; j < G; ++j) best = min(best, part_key[threadIdx.x + j * TX]);
        am_put(p * TX + xl, best & qmask);
      }
    } else {
      // (every point of these levels has both neighbours: p = S + 2 S k < nline - 1)
      const int xl = my_xl;
      for (int k = my_k; k < npts; k += kEdtThreads / TX) {
        const int p = p0 + k * dp;
        const int lo = am_get((p - S) * TX + xl), hi = am_get(min(p + S, nline - 1) * TX + xl);
        int arg = lo;
        if (lo != hi) {  // (neighbours with the same minimiser: it is this point's too)
          int best = 0x7fffffff;
          scan(NEO_EDT_NEGP(p), xl, lo, hi, best);
          arg = best & qmask;
        }
        am_put(p * TX + xl, arg);
      }
    }
    __syncthreads();
  };
  level(2, 0, nline - 1, 0);  // the two end points: full scans
  int top = 1;
  while (top < nline - 1) top <<= 1;
  for (int S = top >> 1; S >= 1; S >>= 1) level((nline - 1 - S + 2 * S - 1) / (2 * S), S, 2 * S, S);
  auto result = [&](int p, int xl) {  // squared distance of voxel p of column xl (>= big: nothing occupied in reach)
    const int q = am_get(p * TX + xl);
    const int key = NEO_EDT_K(hk[q * TX + xl]) + q * NEO_EDT_NEGP(p);
    return (key >> qb) + p * p;  // (arithmetic shift: the key is ((cost - p^2) << qb) | q)
  };
  auto emit = [&](int c) {
    // (the correctly rounded fp64 root is 7 of the z pass's 157 us at 300^3 -- measured with an fp32 root in its place)
    if constexpr (FINAL) return (float)(c >= big ? 1.0e4 : sqrt((double)c) * res);
    else return c >= big ? (uint32_t)kSqInf : (uint32_t)c;
  };
  using OutT = std::conditional_t<FINAL, float, uint32_t>;
  OutT *out = nullptr;
  if constexpr (FINAL) out = out_dist; else out = out_sq;
  if (TX >= 4 && ((nx | stride_line | stride_slab) & 3) == 0) {
    struct alignas(16) Out4 { OutT v[4]; };
    constexpr int CPR = TX / 4 > 0 ? TX / 4 : 1, RPP = kEdtThreads / CPR;
    const int xl = (threadIdx.x % CPR) * 4;
    if (x0 + xl < nx) {
      for (int p = threadIdx.x / CPR; p < nline; p += RPP) {
        Out4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o.v[e] = emit(result(p, xl + e));
        *reinterpret_cast<Out4 *>(out + base + (size_t)p * stride_line + x0 + xl) = o;
      }
    }
  } else {
    for (int i = threadIdx.x; i < nline * TX; i += kEdtThreads) {
      const int p = i >> LX, xl = i & (TX - 1);
      if (x0 + xl >= nx) continue;
      out[base + (size_t)p * stride_line + x0 + xl] = emit(result(p, xl));
    }
  }
}

#undef NEO_EDT_K
#undef NEO_EDT_NEGP

// numpy.gradient, unit spacing: central differences inside, one-sided at the borders.  `recs` (or NULL): the record
// buffer of each map of a batch, in place of `rec`
__global__ void gradient_pack_kernel(const double *__restrict__ dist, int W, int H, double4 *__restrict__ rec,
                                     double4 *const *__restrict__ recs, double *__restrict__ gx_out,
                                     double *__restrict__ gy_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  dist += (size_t)blockIdx.y * W * H;
  if (recs) rec = recs[blockIdx.y];
  const int y = i / W, x = i - y * W;
  double gx, gy;
  if (W == 1) gx = 0.0;
  else if (x == 0) gx = dist[i + 1] - dist[i];
  else if (x == W - 1) gx = dist[i] - dist[i - 1];
  else gx = (dist[i + 1] - dist[i - 1]) / 2.0;
  if (H == 1) gy = 0.0;
  else if (y == 0) gy = dist[i + W] - dist[i];
  else if (y == H - 1) gy = dist[i] - dist[i - W];
  else gy = (dist[i + W] - dist[i - W]) / 2.0;
  rec[i] = make_double4(dist[i], gx, gy, 0.0);
  if (gx_out) gx_out[i] = gx;
  if (gy_out) gy_out[i] = gy;
}

__global__ void pack2d_kernel(const double *__restrict__ dist, const double *__restrict__ gx,
                              const double *__restrict__ gy, int n, double4 *__restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rec[i] = make_double4(dist[i], gx[i], gy[i], 0.0);
}

// 3-D field: convert element type (linear layout)
template <typename SrcT, typename DstT>
__global__ void pack3d_kernel(const SrcT *__restrict__ src, int nx, int ny, int nz, DstT *__restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)nx * ny * nz;
  if (i >= total) return;
  const float v = (float)src[i];
  if constexpr (sizeof(DstT) == 2)
    dst[i] = __float2half(v);
  else
    dst[i] = (DstT)v;
}

// yz-quad layout: dst[voxel][w] = src at (ix, iy + (w & 1), iz + (w >> 1)), clamped at the upper faces
template <typename SrcT, typename DstT>
__global__ void pack3d_yz4_kernel(const SrcT *__restrict__ src, int nx, int ny, int nz, DstT *__restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)nx * ny * nz;
  if (i >= total) return;
  const int ix = (int)(i % nx), iy = (int)((i / nx) % ny), iz = (int)(i / ((size_t)nx * ny));
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int y = min(iy + (w & 1), ny - 1), z = min(iz + (w >> 1), nz - 1);
    const float v = (float)src[((size_t)z * ny + y) * nx + ix];
    if constexpr (sizeof(DstT) == 2)
      dst[i * 4 + w] = __float2half(v);
    else
      dst[i * 4 + w] = (DstT)v;
  }
}

// cell-packed layout: dst[cell][dz][dy][dx] = src at (ix+dx, iy+dy, iz+dz), clamped at the upper faces
template <typename SrcT, typename DstT>
__global__ void pack3d_cell8_kernel(const SrcT *__restrict__ src, int nx, int ny, int nz, DstT *__restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)nx * ny * nz;
  if (i >= total) return;
  const int ix = (int)(i % nx), iy = (int)((i / nx) % ny), iz = (int)(i / ((size_t)nx * ny));
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const int x = min(ix + (w & 1), nx - 1), y = min(iy + ((w >> 1) & 1), ny - 1), z = min(iz + (w >> 2), nz - 1);
    const float v = (float)src[((size_t)z * ny + y) * nx + x];
    if constexpr (sizeof(DstT) == 2)
      dst[i * 8 + w] = __float2half(v);
    else
      dst[i * 8 + w] = (DstT)v;
  }
}

// corner-brick layout: one 128-byte line per block of 2 x 2 x 2 cells (fp32: 32 elements a line, 27 used) or 4 x 2 x 2
// cells (fp16: 64 elements, 45 used); element ((cz * 3 + cy) * CX + cx) of block (bx, by, bz) = src at the block's corner
// (cx, cy, cz), clamped at the upper faces; the rest of the line is zero.
// A workgroup packs kBrickXB bricks of one (by, bz) row: their nine source rows (3 y x 3 z) come in with coalesced loads
// through LDS, then every thread assembles 16-byte (fp32) / 8-byte (fp16) pieces of the lines.  (Round 4, first form: one
// thread per four stored elements reading its four corners straight from memory -- 153 us at 300^3, bound by the
// address processing of the scattered 4-byte loads.)
constexpr int kBrickXB = 64;  // (32: 145 us at 300^3 against 126)
template <typename SrcT, typename DstT>
__global__ __launch_bounds__(256) void pack3d_brick_kernel(const SrcT *__restrict__ src, int nx, int ny, int nz, int nbx, int nby,
                                                           DstT *__restrict__ dst) {
  constexpr int SHX = sizeof(DstT) == 4 ? 1 : 2, CX = (1 << SHX) + 1, PER = 128 / (int)sizeof(DstT);
  constexpr int NCOL = (kBrickXB << SHX) + 1;  // corners along x the workgroup's bricks touch
  __shared__ float tile[9 * NCOL];
  const int bx0 = blockIdx.x * kBrickXB, by = blockIdx.y, bz = blockIdx.z;
  {
    constexpr int NL = (9 * NCOL + 255) / 256;  // loads a thread, all in flight before the first is stored
    SrcT w[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int i = min((int)threadIdx.x + u * 256, 9 * NCOL - 1), r = i / NCOL, cxl = i - r * NCOL;
      const int x = min((bx0 << SHX) + cxl, nx - 1), y = min(2 * by + r % 3, ny - 1), z = min(2 * bz + r / 3, nz - 1);
      w[u] = src[((size_t)z * ny + y) * nx + x];
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int i = threadIdx.x + u * 256;
      if (i < 9 * NCOL) tile[i] = (float)w[u];
    }
  }
  __syncthreads();
  constexpr int Q = PER / 4;  // four-element pieces a line
  DstT *line0 = dst + ((size_t)((size_t)bz * nby + by) * nbx + bx0) * PER;
  for (int i = threadIdx.x; i < kBrickXB * Q; i += 256) {
    const int bl = i / Q, e0 = (i - bl * Q) * 4;
    if (bx0 + bl >= nbx) break;  // (bl grows with i)
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + k, r = e / CX, cx = e - r * CX;  // r = cz * 3 + cy
      v[k] = e < 9 * CX ? tile[r * NCOL + (bl << SHX) + cx] : 0.0f;
    }
    DstT *o = line0 + (size_t)bl * PER + e0;
    if constexpr (sizeof(DstT) == 2) {
      const __half2 lo = __floats2half2_rn(v[0], v[1]), hi = __floats2half2_rn(v[2], v[3]);
      uint2 u;
      u.x = *reinterpret_cast<const unsigned int *>(&lo);
      u.y = *reinterpret_cast<const unsigned int *>(&hi);
      *reinterpret_cast<uint2 *>(o) = u;
    } else {
      *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

template <typename Real, class MapT, class LookupT, int DM>
__global__ void query_kernel(int n, MapT map, const double *__restrict__ pts, double *__restrict__ dist,
                             double *__restrict__ grad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Real pos[DM], g[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) pos[d] = (Real)pts[(size_t)i * DM + d];
  bool inside;
  LookupT lk(map);
  const Real v = lk.template fetch<DM>(pos, g, inside);
  dist[i] = (double)v;
  if (grad)
#pragma unroll
    for (int d = 0; d < DM; ++d) grad[(size_t)i * DM + d] = (double)g[d];
}

}  // namespace neo
