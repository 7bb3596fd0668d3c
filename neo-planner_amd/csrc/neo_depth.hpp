// neo_depth.hpp -- the batched depth camera (include/neo_planner.h: neo_depth_render_batch): B pinhole images of box
// scenes, the sensor in front of the initializer network.  The arithmetic is initializer.raycast_depth's slab test
// restated in fp32, every product rounded on its own (tests/depth_oracle_np.py is the same text in NumPy, and the tests
// compare bit for bit), so nothing here may fuse, reassociate or approximate:
//
//   u_j, v_i           fp64 on the device, rounded once (depth_uv_kernel; a table per call, not per ray)
//   d = (c + u s, s - u c, -v), inv = 1 / d       correctly rounded divisions, a zero component gives +-inf
//   rel = (float)(corner - eye)                   fp64 subtraction, once per image and box
//   t0 = rel_lo inv, t1 = rel_hi inv, tn = max_axes min(t0, t1), tf = min_axes max(t0, t1)
//   hit: tf >= max(tn, 0) and no NaN among the six products; depth = min(depth, max(tn, 0))
//
// Three kernels: depth_uv_kernel (the two tables), depth_render_kernel (depth_m and the image's maximum) and
// depth_norm_kernel (depth_m -> depth_u8; it needs the whole image's maximum, hence a pass of its own).
//
// depth_render_kernel: one workgroup of 256 lanes per tile of 64 x 64 pixels, rendered as four strips of 16 rows, four
// horizontally adjacent pixels per lane (one 16-byte store of depth_m); a lane keeps its columns' x and y inverses over
// the strips.  The workgroup first cuts its scene's box list down to the boxes its tile can
// see (the cull block below: interval arithmetic on the very operations the rays use, so it drops only boxes every ray of the
// tile misses, or that start beyond max_range) and keeps the survivors' fp32 bounds in LDS; the box loop is then the
// same for every lane -- broadcast LDS reads, no divergence.  NaN (0 x inf: a ray parallel to a face whose plane holds
// the eye) is a miss, as NumPy's minimum / maximum propagate it: a box carries one bit per axis with a zero bound, a ray
// one bit per axis with an infinite inverse, and a hit needs their AND to be empty, so the min / max of the slab test
// only ever see numbers.  The image's maximum is an integer atomicMax on the bits of the non-negative depths (-0 never
// leaves the kernel): independent of order, launch and batch.  A request whose scene index or box range is out of
// range gets NaN everywhere (NaN's bits win the integer maximum) and reads no box.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/neo_planner.h"

namespace neo {

constexpr int kDepthTileW = 64, kDepthStripH = 16;  // a strip: 16 lanes x 4 pixels by 16 rows, one row per lane
constexpr int kDepthStrips = 4;                     // strips a workgroup renders one after the other from one culled list
constexpr int kDepthTileH = kDepthStripH * kDepthStrips;
constexpr int kDepthThreads = 256;
constexpr int kDepthMaxSide = 4096;                // width, height <= this (the tables' size)
constexpr unsigned kDepthNaNBits = 0x7fc00000u;

struct DepthArgs {
  int W, H, n_scenes, B;
  float max_range;
  const double *boxes;     // [NB][6]
  const int *box_begin;    // [n_scenes + 1]
  const int *scene_index;  // [B] or NULL
  const double *pose;      // [B][5]
  const float *u, *v;      // the tables: u padded to a multiple of 4 columns
  float *depth_m;
  unsigned char *depth_u8;  // or NULL
  unsigned *max_bits;       // [B]: the images' maxima as bits (zeroed before the render pass)
  unsigned long long *box_tests;  // optional counter (neo_depth_box_test_counter)
  int vec_m, vec_u8;        // rows of depth_m / images of depth_u8 start 16 / 4-byte aligned: packed stores
};

// a product rounded on its own (never the multiply of a fused multiply-add)
__device__ __forceinline__ float depth_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ bool depth_not_finite(float x) { return !(fabsf(x) < INFINITY); }

__global__ __launch_bounds__(kDepthThreads) void depth_uv_kernel(int W, int H, double focal, float *__restrict__ u,
                                                                 float *__restrict__ v) {
  const int k = blockIdx.x * kDepthThreads + threadIdx.x;
  const int Wp = (W + 3) & ~3;
  if (k < Wp) {
    const double num = (double)k - (double)(W - 1) / 2.0;
    u[k] = (float)(num / focal);
  } else if (k - Wp < H) {
    const double num = (double)(k - Wp) - (double)(H - 1) / 2.0;
    v[k - Wp] = (float)(num / focal);
  }
}

// the range of 1 / d over a tile whose direction component lies in [dmin, dmax]: usable only where the component keeps
// one sign (1 / d is monotone there, and so is its rounding)
struct DepthInvRange {
  float lo, hi;
  bool ok;
};
__device__ __forceinline__ DepthInvRange depth_inv_range(float da, float db) {
  const float dmin = fminf(da, db), dmax = fmaxf(da, db);
  DepthInvRange r;
  r.ok = (dmin > 0.0f || dmax < 0.0f) && da == da && db == db;
  r.lo = 1.0f / dmax;
  r.hi = 1.0f / dmin;
  return r;
}

// bounds of one axis's slab over the tile: every ray's min(t0, t1) >= near_lo and max(t0, t1) <= far_hi, because a
// rounded product is monotone in either factor.  Returns false (no bound from this axis) when a product is NaN.
__device__ __forceinline__ bool depth_axis_bounds(float rl, float rh, const DepthInvRange &r, float &near_lo, float &far_hi) {
  if (!r.ok) return false;
  const float p0 = depth_mul(rl, r.lo), p1 = depth_mul(rl, r.hi), q0 = depth_mul(rh, r.lo), q1 = depth_mul(rh, r.hi);
  if (!(p0 == p0 && p1 == p1 && q0 == q0 && q1 == q1)) return false;
  near_lo = fminf(fminf(p0, p1), fminf(q0, q1));
  far_hi = fmaxf(fmaxf(p0, p1), fmaxf(q0, q1));
  return true;
}

__global__ __launch_bounds__(kDepthThreads) void depth_render_kernel(DepthArgs a, int img0, int tiles_x) {
  __shared__ float4 sbox[2 * NEO_DEPTH_MAX_BOXES];  // per kept box: (rel_lo xyz, mask bits), (rel_hi xyz, -)
  __shared__ int s_n;
  __shared__ unsigned s_max;
  const int b = img0 + (int)blockIdx.y;
  const int t = threadIdx.x;
  const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
  const int jlo = tx * kDepthTileW, ilo = ty * kDepthTileH;
  const int jhi = min(jlo + kDepthTileW, a.W) - 1, ihi = min(ilo + kDepthTileH, a.H) - 1;
  const int j0 = jlo + (t & 15) * 4, i0 = ilo + (t >> 4);
  const bool col_active = j0 < a.W;

  // the request's scene (the same in every lane)
  const int si = a.scene_index ? a.scene_index[b] : 0;
  bool bad = si < 0 || si >= a.n_scenes;
  int beg = 0, nb = 0;
  if (!bad) {
    beg = a.box_begin[si];
    nb = a.box_begin[si + 1] - beg;
    bad = beg < 0 || nb < 0 || nb > NEO_DEPTH_MAX_BOXES;
  }
  if (bad) {
    const float qnan = __uint_as_float(kDepthNaNBits);
    for (int i = i0; i <= ihi; i += kDepthStripH)
      for (int p = 0; p < 4; ++p)
        if (j0 + p < a.W) a.depth_m[((size_t)b * a.H + i) * a.W + j0 + p] = qnan;
    if (t == 0) atomicMax(a.max_bits + b, kDepthNaNBits);
    return;
  }
  if (t == 0) {
    s_n = 0;
    s_max = 0u;
  }
  __syncthreads();

  const double *ps = a.pose + (size_t)b * 5;
  const double ex = ps[0], ey = ps[1], ez = ps[2];
  const float c = (float)ps[3], s = (float)ps[4];

  // ---- cull: the tile's direction ranges, then one box per lane
  {
    const float ua = a.u[jlo], ub = a.u[jhi];
    const float usa = depth_mul(ua, s), usb = depth_mul(ub, s);
    const float dxa = c + usa, dxb = c + usb;
    const float uca = depth_mul(ua, c), ucb = depth_mul(ub, c);
    const float dya = s - uca, dyb = s - ucb;
    const DepthInvRange rx = depth_inv_range(dxa, dxb), ry = depth_inv_range(dya, dyb);
    const DepthInvRange rz = depth_inv_range(-a.v[ilo], -a.v[ihi]);
    for (int k = t; k < nb; k += kDepthThreads) {
      const double *bx = a.boxes + (size_t)(beg + k) * 6;
      const float lx = (float)(bx[0] - ex), ly = (float)(bx[1] - ey), lz = (float)(bx[2] - ez);
      const float hx = (float)(bx[3] - ex), hy = (float)(bx[4] - ey), hz = (float)(bx[5] - ez);
      // a NaN bound makes every ray's tn and tf NaN: a miss everywhere
      if (!(lx == lx && ly == ly && lz == lz && hx == hx && hy == hy && hz == hz)) continue;
      float tn_lo = -INFINITY, tf_hi = INFINITY, nl, fh;
      if (depth_axis_bounds(lx, hx, rx, nl, fh)) tn_lo = fmaxf(tn_lo, nl), tf_hi = fminf(tf_hi, fh);
      if (depth_axis_bounds(ly, hy, ry, nl, fh)) tn_lo = fmaxf(tn_lo, nl), tf_hi = fminf(tf_hi, fh);
      if (depth_axis_bounds(lz, hz, rz, nl, fh)) tn_lo = fmaxf(tn_lo, nl), tf_hi = fminf(tf_hi, fh);
      const float enter = tn_lo > 0.0f ? tn_lo : 0.0f;
      // every ray of the tile misses it (tf <= tf_hi < enter <= max(tn, 0)), or it cannot lower a depth (depth <=
      // max_range <= enter <= max(tn, 0))
      if (tf_hi < enter || enter >= a.max_range) continue;
      const int mask = 8 | ((lx == 0.0f || hx == 0.0f) ? 1 : 0) | ((ly == 0.0f || hy == 0.0f) ? 2 : 0) |
                       ((lz == 0.0f || hz == 0.0f) ? 4 : 0);
      const int at = atomicAdd(&s_n, 1);  // (the order of the list does not matter: min is exact)
      sbox[2 * at] = make_float4(lx, ly, lz, __int_as_float(mask));
      sbox[2 * at + 1] = make_float4(hx, hy, hz, 0.0f);
    }
  }
  __syncthreads();
  const int n = s_n;
  if (a.box_tests && t == 0)
    atomicAdd(a.box_tests, (unsigned long long)n * (unsigned long long)((jhi - jlo + 1) * (ihi - ilo + 1)));

  unsigned mbits = 0u;
  if (col_active) {
    // ---- this lane's four columns: the x and y components of its rays, the same in every strip
    float ix[4], iy[4];
    int xymask[4];
    const float4 u4 = *reinterpret_cast<const float4 *>(a.u + j0);  // (the table is padded to a multiple of 4)
    const float uu[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float us = depth_mul(uu[p], s);
      const float dx = c + us;
      const float uc = depth_mul(uu[p], c);
      const float dy = s - uc;
      ix[p] = 1.0f / dx;
      iy[p] = 1.0f / dy;
      xymask[p] = (depth_not_finite(ix[p]) ? 1 : 0) | (depth_not_finite(iy[p]) ? 2 : 0) |
                  ((ix[p] != ix[p] || iy[p] != iy[p]) ? 8 : 0);
    }
    const float ezn = (float)(-ez);
    for (int i = i0; i <= ihi; i += kDepthStripH) {
      // ---- the row's z component, the ground, the start depth
      const float dz = -a.v[i];
      const float iz = 1.0f / dz;
      const int zmask = (depth_not_finite(iz) ? 4 : 0) | (iz != iz ? 8 : 0);
      float tg = INFINITY;
      if (dz < 0.0f) tg = ezn / dz;
      const float d0 = tg < a.max_range ? tg : a.max_range;  // min(max_range, tg)
      float depth[4] = {d0, d0, d0, d0};
      // ---- the kept boxes: wave-uniform loop, broadcast LDS reads
      for (int k = 0; k < n; ++k) {
        const float4 lo = sbox[2 * k], hi = sbox[2 * k + 1];
        const int mask = __float_as_int(lo.w);
        const float t0z = depth_mul(lo.z, iz), t1z = depth_mul(hi.z, iz);
        const float nz = fminf(t0z, t1z), fz = fmaxf(t0z, t1z);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float t0x = depth_mul(lo.x, ix[p]), t1x = depth_mul(hi.x, ix[p]);
          const float t0y = depth_mul(lo.y, iy[p]), t1y = depth_mul(hi.y, iy[p]);
          const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), nz);
          const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fz);
          const float enter = tn > 0.0f ? tn : 0.0f;  // max(tn, 0), never -0
          const bool hit = tf >= enter && !(mask & (xymask[p] | zmask));
          depth[p] = (hit && enter < depth[p]) ? enter : depth[p];
        }
      }
      // ---- clip(depth, 0, max_range), store, the lane's maximum
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float d = depth[p] > 0.0f ? depth[p] : 0.0f;
        d = d < a.max_range ? d : a.max_range;
        depth[p] = d;
        if (j0 + p < a.W) mbits = max(mbits, __float_as_uint(d));
      }
      float *out = a.depth_m + ((size_t)b * a.H + i) * a.W + j0;
      if (a.vec_m && j0 + 3 < a.W) {
        *reinterpret_cast<float4 *>(out) = make_float4(depth[0], depth[1], depth[2], depth[3]);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (j0 + p < a.W) out[p] = depth[p];
      }
    }
  }
  // ---- the tile's maximum: wavefront, workgroup, then one integer atomic for the image
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mbits = max(mbits, (unsigned)__shfl_xor((int)mbits, off));
  if ((t & 63) == 0) atomicMax(&s_max, mbits);
  __syncthreads();
  if (t == 0) atomicMax(a.max_bits + b, s_max);
}

// depth_u8 = (uint8)(depth / max(depth_max, 1e-9f) * 255.0f): four consecutive pixels of an image per lane
__global__ __launch_bounds__(kDepthThreads) void depth_norm_kernel(DepthArgs a, int img0) {
  const int b = img0 + (int)blockIdx.y;
  const size_t hw = (size_t)a.H * a.W;
  const size_t q = ((size_t)blockIdx.x * kDepthThreads + threadIdx.x) * 4;
  if (q >= hw) return;
  const float dm = __uint_as_float(a.max_bits[b]);
  const bool bad = !(dm == dm);
  const float mx = dm > 1e-9f ? dm : 1e-9f;
  const float *src = a.depth_m + (size_t)b * hw + q;
  unsigned char *dst = a.depth_u8 + (size_t)b * hw + q;
  const int cnt = (int)min((size_t)4, hw - q);
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (a.vec_u8 && cnt == 4) {
    const float4 d4 = *reinterpret_cast<const float4 *>(src);
    d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
  } else {
    for (int p = 0; p < cnt; ++p) d[p] = src[p];
  }
  unsigned o[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float r = d[p] / mx;
    const float r255 = depth_mul(r, 255.0f);
    o[p] = bad ? 0u : (unsigned)(int)r255;
  }
  if (a.vec_u8 && cnt == 4) {
    *reinterpret_cast<unsigned *>(dst) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
  } else {
    for (int p = 0; p < cnt; ++p) dst[p] = (unsigned char)o[p];
  }
}

}  // namespace neo
