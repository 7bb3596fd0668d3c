// neo_map.hpp -- the vocabulary every unit shares: the FLAT slot count, the planner parameters as the kernels see them
// (DevParams and its par_* accessors), the map records (Map2D, Map3D) and the map lookups (Lookup2D, Lookup3D).  No MINCO
// arithmetic: that is neo_device.hpp, which includes this header.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "../../include/neo_planner.h"
#include "neo_wave.hpp"

namespace neo {

constexpr int kSlots = 4;  // FLAT layout: n <= 256
// limits on FLAT slots the host's dispatch and the kernels agree on
#ifndef NEO_SM_MAX_SLOTS
#define NEO_SM_MAX_SLOTS 2  // FLAT slots up to which the optimiser runs as the resumable state machine (neo_lbfgs_sm.hpp)
#endif
#ifndef NEO_W2_MAX_SLOTS
#define NEO_W2_MAX_SLOTS 4  // two waves per SIMD for every n <= 256 (four FLAT slots: with fp32 pairs, pairs_in_f32)
#endif

struct DevParams {
  double v_max, T_min, T_max, safe_dis, delta_t;
  double w[4];
  double coll_tol;
  double ftol, gtol;
  int maxls, maxiter, maxfun, stale_T;
  int dbg;  // timing experiments only (neo_params.flags): 1 skip sample loop, 2 skip joint sweeps, 4 no history -- read by
            // the kernels of -DNEO_EXPERIMENTS builds alone (NEO_DBG, neo_device.hpp); the product's kernels have no such paths
  // fp32 forms of what the fp32 arithmetic uses, derived on the host (derive()): kernel arguments arrive in scalar
  // registers, whereas a (float)prm.x inside a kernel is a vector conversion whose (wave-uniform) result the compiler
  // hoists and then keeps in a vector register across the whole optimiser loop -- nine of them, spilled to scratch in the
  // three-waves-per-SIMD kernels
  struct F32 {
    float T_min, T_span;  // (float)T_max - (float)T_min, rounded as the device expression was
    float dt, inv_dt;     // (float)delta_t, (float)(1 / delta_t)
    float vmax2, safe;
    float w[4];
  } f;
  __host__ __device__ void derive() {
    f.T_min = (float)T_min;
    f.T_span = (float)T_max - (float)T_min;
    f.dt = (float)delta_t;
    f.inv_dt = (float)(1.0 / delta_t);
    f.vmax2 = (float)(v_max * v_max);
    f.safe = (float)safe_dis;
    for (int k = 0; k < 4; ++k) f.w[k] = (float)w[k];
  }
};
// a parameter in the arithmetic N: the double itself, or its fp32 form from DevParams::f
#define NEO_PARAM(name, dexpr, fexpr)                                                  \
  template <typename N>                                                                \
  __device__ __forceinline__ N name(const DevParams &p) {                              \
    if constexpr (sizeof(N) == 4) return (fexpr); else return (N)(dexpr);              \
  }
NEO_PARAM(par_T_min, p.T_min, p.f.T_min)
NEO_PARAM(par_T_span, N(p.T_max) - N(p.T_min), p.f.T_span)
NEO_PARAM(par_dt, p.delta_t, p.f.dt)
NEO_PARAM(par_inv_dt, 1.0 / p.delta_t, p.f.inv_dt)
NEO_PARAM(par_vmax2, p.v_max * p.v_max, p.f.vmax2)
NEO_PARAM(par_safe, p.safe_dis, p.f.safe)
NEO_PARAM(par_w0, p.w[0], p.f.w[0])
NEO_PARAM(par_w1, p.w[1], p.f.w[1])
NEO_PARAM(par_w2, p.w[2], p.f.w[2])
NEO_PARAM(par_w3, p.w[3], p.f.w[3])
#undef NEO_PARAM

// 2-D reference map: one 32-byte record per cell {dist, grad_x, grad_y, 0}
struct Map2D {
  const double4 *rec;
  int W, H;
  double res, ox, oy;
};
// 3-D distance field, element type E
struct Map3D {
  const void *data;
  int nx, ny, nz;
  int layout;  // 0 linear [z][y][x], 1 = yz-quads (the 2x2 (y,z) neighbourhood of every voxel contiguous, x-major),
               // 2 = cell-packed (8 corners of every cell contiguous), 3 = corner bricks (one 128-byte line per block of
               // 2 x 2 x 2 cells (fp32: its 27 corners) or 4 x 2 x 2 cells (fp16: its 45 corners))
  double res, ox, oy, oz;
  unsigned int bytes;  // size of the stored field (buffer-descriptor range)
  // fp32 constants of the lookup (Lookup3D), derived on the host: cell coordinate minus one half = pos * f_inv + f_off,
  // inside <=> -0.5 <= that < f_hi.  Computed in the kernel they are fp64 divisions whose results the compiler hoists
  // out of the optimiser loop and keeps in vector registers (spilled at three wavefronts per SIMD); as part of the
  // map record they arrive in scalar registers.
  float f_inv, f_off[3], f_hi[3];
  int nbx, nby;  // corner-brick layout: blocks along x and y (set by the upload for layout 3)
  double d_inv;  // 1 / res for the fp64 lookups (round 5: three fp64 divisions a sample -- ~10 instructions each with
                 // v_rcp_f64 and its refinement -- became multiplications; the trilinear mode is defined by the oracle,
                 // which divides: cell coordinates differ by an ulp at most, distances by ~1e-13 relative)
  __host__ __device__ void derive() {
    d_inv = 1.0 / res;
    f_inv = (float)(1.0 / res);
    f_off[0] = (float)(-ox / res - 0.5);
    f_off[1] = (float)(-oy / res - 0.5);
    f_off[2] = (float)(-oz / res - 0.5);
    f_hi[0] = (float)nx - 0.5f;
    f_hi[1] = (float)ny - 0.5f;
    f_hi[2] = (float)nz - 0.5f;
  }
};

// ------------------------------------------------------------------ map lookups
// esdf.py:53-82: nearest cell with int() truncation; out of range -> 10000 / zero gradient.
// Returns the distance; the gradient (metres per cell, as np.gradient leaves it) is only
// fetched when the caller needs it -- it lives in the same 32-byte record.
// Lookups are split into prepare (index arithmetic) / load (the gathers) / finish (interpolation) so
// that the sample loop can put the loads of several samples in flight before it consumes any.
template <typename Real>
struct Lookup2D {
  const Map2D &m;
  __device__ __forceinline__ explicit Lookup2D(const Map2D &m_) : m(m_) {}
  struct Addr {
    int idx;
    bool inside;
  };
  struct Raw {
    double4 r;
  };
  static constexpr bool gather_ahead = false;  // (one record a sample: the sample loop stays as it is, minco_sample)
  // `on` = false (an idle sample slot): treated like a point outside the map, so that all idle lanes of a
  // wavefront read one and the same record instead of 64 scattered ones
  template <int D>
  __device__ __forceinline__ Addr prepare(const Real (&pos)[D], bool on = true) const {
    // index arithmetic in fp64 with a true division, exactly like int((y - origin.y) / res)
    const double fy = ((double)pos[1] - m.oy) / m.res;
    const double fx = ((double)pos[0] - m.ox) / m.res;
    Addr a;
    a.idx = 0;
    a.inside = false;
    if (!on || !(fabs(fy) < 1.0e9) || !(fabs(fx) < 1.0e9)) return a;
    const int row = (int)fy, col = (int)fx;  // C casts truncate toward zero, like int()
    if (row < 0 || row >= m.H || col < 0 || col >= m.W) return a;
    a.inside = true;
    a.idx = row * m.W + col;
    return a;
  }
  __device__ __forceinline__ Raw load(const Addr &a) const {
    Raw q;
    q.r = m.rec[a.idx];  // idx = 0 when outside: a valid, ignored record
    return q;
  }
  template <int D>
  __device__ __forceinline__ Real finish(const Addr &a, const Raw &q, Real (&g)[D]) const {
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] = Real(0);
    if (!a.inside) return Real(10000);
    g[0] = (Real)q.r.y;
    g[1] = (Real)q.r.z;
    return (Real)q.r.x;
  }
  template <int D>
  __device__ __forceinline__ Real fetch(const Real (&pos)[D], Real (&g)[D], bool &inside) const {
    const Addr a = prepare<D>(pos);
    inside = a.inside;
    return finish<D>(a, load(a), g);
  }
};

template <typename E>
__device__ __forceinline__ float elem_to_float(E v);
template <>
__device__ __forceinline__ float elem_to_float<float>(float v) { return v; }
template <>
__device__ __forceinline__ float elem_to_float<__half>(__half v) { return __half2float(v); }

// two x-adjacent voxels in ONE load that is only element-aligned: an integer of twice the element
// size with reduced alignment (gfx950 global loads accept dword-aligned dwordx2), split afterwards.
// (Loading a two-member struct instead gets scalarised into two loads before the backend sees it.)
typedef unsigned long long u64_align4 __attribute__((aligned(4)));
typedef unsigned int u32_align2 __attribute__((aligned(2)));
template <typename E>
__device__ __forceinline__ void load_pair(const E *p, float &a, float &b);
template <>
__device__ __forceinline__ void load_pair<float>(const float *p, float &a, float &b) {
  const unsigned long long u = *reinterpret_cast<const u64_align4 *>(p);
  a = __uint_as_float((unsigned int)(u & 0xffffffffull));
  b = __uint_as_float((unsigned int)(u >> 32));
}
// The compiler splits a dword-aligned 8-byte *global* load into two dword loads; a raw buffer load
// of 8 bytes at a dword-aligned offset is one instruction and returns the right data on gfx950
// (tools/probe/unaligned_pair.hip).  `off` = byte offset into the field.
// `soff` is a wave-uniform byte offset (an SGPR operand of the instruction: the four x-pairs of a lookup share
// one address register).
__device__ __forceinline__ void buffer_load_pair_f32(__amdgpu_buffer_rsrc_t rsrc, unsigned int off, unsigned int soff,
                                                     float &a, float &b) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)off, (int)soff, 0);
  a = __uint_as_float(v[0]);
  b = __uint_as_float(v[1]);
}
template <>
__device__ __forceinline__ void load_pair<__half>(const __half *p, float &a, float &b) {
  const unsigned int u = *reinterpret_cast<const u32_align2 *>(p);
  a = __half2float(__ushort_as_half((unsigned short)(u & 0xffffu)));
  b = __half2float(__ushort_as_half((unsigned short)(u >> 16)));
}

// trilinear distance + analytic gradient (oracle/minco_np.py:Grid3DESDF defines the semantics)
// LAYOUT is a template parameter (0 linear, 1 yz-quads, 2 cell-packed, 9 = read Map3D::layout at run time,
// for the point-query kernel only): a run-time branch on the layout inside the sample
// loop makes the compiler join the two load paths and wait for each sample's loads right there,
// which defeats keeping several samples' gathers in flight.
template <typename Real, typename E, int LAYOUT>
struct Lookup3D {
  const Map3D &m;
  __amdgpu_buffer_rsrc_t rsrc;
  // fp32 arithmetic: cell coordinate minus one half in ONE fma, um = pos * inv + off (all wave-uniform operands)
  float inv, off[3], hi[3];
  __device__ __forceinline__ explicit Lookup3D(const Map3D &m_)
      : m(m_), rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(m_.data), 0, (int)m_.bytes, 0x00020000)) {
    inv = m_.f_inv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      off[k] = m_.f_off[k];
      hi[k] = m_.f_hi[k];
    }
  }
  struct Addr {
    int i0[3];
    Real fr[3];
    bool inside;
  };
  struct Raw {
    float c[2][2][2];
  };
  // the gather-ahead form of the sample loop (minco_sample) exists for this lookup on fp32 fields (fp16 fields: the brick
  // members spill 5 - 10 vector registers in that form and keep the blocked loop); pin(): the loaded corners as opaque
  // copies, made where the call stands
  static constexpr bool gather_ahead = sizeof(E) == 4;
  static __device__ __forceinline__ void pin(Raw &q) {
#pragma unroll
    for (int k = 0; k < 8; ++k) q.c[k >> 2][(k >> 1) & 1][k & 1] = opaque(q.c[k >> 2][(k >> 1) & 1][k & 1]);
  }

  // `on` = false (an idle sample slot): treated like a point outside the field -- corner (0,0,0) for every
  // idle lane, i.e. one cache line per wavefront instead of 64 scattered gathers
  template <int D>
  __device__ __forceinline__ Addr prepare(const Real (&pos)[D], bool on = true) const {
#pragma clang fp contract(on)  // fuse a*b+c only as written: the same arithmetic whatever the unrolling around it
    static_assert(D == 3, "the 3-D map needs D = 3");
    const int n[3] = {m.nx, m.ny, m.nz};
    const double org[3] = {m.ox, m.oy, m.oz};
    Addr a;
    a.inside = on;
    if constexpr (sizeof(Real) == 4) {
      // (measured and rejected: clamping the cell coordinate with v_med3_f32 before truncating -- 7 instructions an axis
      // instead of 10, but nine more wave-uniform float constants, of which an instruction can name only one as a
      // scalar operand; the integer clamps below take theirs from scalar registers: 1.22 M against 1.25 M traj/s at cfg2)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float um = fmaf(pos[k], inv, off[k]);
        if (!(um >= -0.5f && um < hi[k])) a.inside = false;
        const int i = min(max((int)floorf(um), 0), n[k] - 2);
        a.i0[k] = i;
        a.fr[k] = __builtin_amdgcn_fmed3f(um - (float)i, 0.0f, 1.0f);
      }
      if (!a.inside) a.i0[0] = a.i0[1] = a.i0[2] = 0;
      return a;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Real u = (Real)(((double)pos[k] - org[k]) * m.d_inv);  // oracle Grid3DESDF._cell divides by res: an ulp apart at most
      if (!(u >= Real(0) && u < (Real)n[k])) a.inside = false;
      u -= Real(0.5);
      const int i = min(max((int)floor(u), 0), n[k] - 2);
      a.i0[k] = i;
      a.fr[k] = fmin(fmax(u - (Real)i, Real(0)), Real(1));
    }
    if (!a.inside) a.i0[0] = a.i0[1] = a.i0[2] = 0;
    return a;
  }
  __device__ __forceinline__ Raw load(const Addr &a) const {
    const E *vox = static_cast<const E *>(m.data);
    Raw q;
    if (LAYOUT == 2 || (LAYOUT == 9 && m.layout == NEO_LAYOUT_CELL8)) {
      // cell-packed: the 8 corners [dz][dy][dx] of cell (ix, iy, iz) are contiguous and 16-byte aligned:
      // one lookup = one 32-byte (fp32) or 16-byte (fp16) read instead of four gathers
      const unsigned int cell = __umul24(__umul24((unsigned)a.i0[2], (unsigned)m.ny) + (unsigned)a.i0[1], (unsigned)m.nx) +
                                (unsigned)a.i0[0];
      if constexpr (sizeof(E) == 4) {
        const auto lo = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(cell * 32u), 0, 0);
        const auto hi = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(cell * 32u + 16u), 0, 0);
        q.c[0][0][0] = __uint_as_float(lo[0]); q.c[0][0][1] = __uint_as_float(lo[1]);
        q.c[0][1][0] = __uint_as_float(lo[2]); q.c[0][1][1] = __uint_as_float(lo[3]);
        q.c[1][0][0] = __uint_as_float(hi[0]); q.c[1][0][1] = __uint_as_float(hi[1]);
        q.c[1][1][0] = __uint_as_float(hi[2]); q.c[1][1][1] = __uint_as_float(hi[3]);
      } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(cell * 16u), 0, 0);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          q.c[w >> 1][w & 1][0] = __half2float(__ushort_as_half((unsigned short)(v[w] & 0xffffu)));
          q.c[w >> 1][w & 1][1] = __half2float(__ushort_as_half((unsigned short)(v[w] >> 16)));
        }
      }
    } else if (LAYOUT == 3 || (LAYOUT == 9 && m.layout == NEO_LAYOUT_BRICK)) {
      // corner bricks: the cells are grouped in blocks of 2 x 2 x 2 (fp32) or 4 x 2 x 2 (fp16: x is the direction most
      // requests fly in), and all (2+1)^3 = 27 (or 5 x 3 x 3 = 45) corners of a block sit in ONE 128-byte line, [z][y][x]
      // inside the line.  A lookup is four x-pairs of that line -- one address register, four immediate offsets -- and
      // a path stays on the line for two cells in EVERY direction, where the yz-quad line is eight cells along x and one
      // along y and z: fewer lines per path (tools/sim_esdf_locality.py: -27 % lines fetched at cfg2), the same memory
      // (16 bytes a cell in fp32).
      constexpr int SHX = sizeof(E) == 4 ? 1 : 2, CX = (1 << SHX) + 1;  // cells (log2) and corners of a block along x
      const unsigned int bx = (unsigned)a.i0[0] >> SHX, by = (unsigned)a.i0[1] >> 1, bz = (unsigned)a.i0[2] >> 1;
      const unsigned int lx = (unsigned)a.i0[0] & ((1u << SHX) - 1u), ly = (unsigned)a.i0[1] & 1u, lz = (unsigned)a.i0[2] & 1u;
      const unsigned int blk = __umul24(__umul24(bz, (unsigned)m.nby) + by, (unsigned)m.nbx) + bx;
      const unsigned int in_line = (lz * 3u + ly) * (unsigned)CX + lx;  // element of corner (0,0,0) inside the line
#pragma unroll
      for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          const unsigned int so = (unsigned)((dz * 3 + dy) * CX);  // compile-time: the instruction's immediate offset
          if constexpr (sizeof(E) == 4) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(blk * 128u + in_line * 4u + so * 4u), 0, 0);
            q.c[dz][dy][0] = __uint_as_float(v[0]);
            q.c[dz][dy][1] = __uint_as_float(v[1]);
          } else {
            load_pair<E>(vox + blk * 64u + in_line + so, q.c[dz][dy][0], q.c[dz][dy][1]);
          }
        }
    } else if (LAYOUT == 0 || (LAYOUT == 9 && m.layout == NEO_LAYOUT_LINEAR)) {
      // 32-bit element index of corner (0,0,0); the other three x-pairs sit at +nx, +nx*ny, +nx*ny+nx
      const unsigned int base = __umul24(__umul24((unsigned)a.i0[2], (unsigned)m.ny) + (unsigned)a.i0[1], (unsigned)m.nx) +
                                (unsigned)a.i0[0];
      const unsigned int sy = (unsigned)m.nx, sz = (unsigned)m.nx * (unsigned)m.ny;
#pragma unroll
      for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          const unsigned int so = (dy ? sy : 0u) + (dz ? sz : 0u);
          if constexpr (sizeof(E) == 4)
            buffer_load_pair_f32(rsrc, base * 4u, so * 4u, q.c[dz][dy][0], q.c[dz][dy][1]);
          else  // (a 4-byte buffer load at a 2-byte-aligned offset works too, tools/probe/unaligned_half_pair.hip,
                //  but measured 2 % slower at cfg5 than the global load)
            load_pair<E>(vox + base + so, q.c[dz][dy][0], q.c[dz][dy][1]);
        }
    } else {
      // yz-quads: voxel (ix, iy, iz) stores {d(iy,iz), d(iy+1,iz), d(iy,iz+1), d(iy+1,iz+1)} at x = ix, records in
      // [z][y][x] order: the 8 corners of a cell are the records ix and ix + 1 = 32 contiguous bytes (fp32; 16 for fp16),
      // and x-adjacent cells share half of them -- 4x the memory of the linear layout instead of 8x, one line per
      // lookup instead of four, and a sample triple walking along x stays on its 128-byte line for 8 cells
      const unsigned int cell = __umul24(__umul24((unsigned)a.i0[2], (unsigned)m.ny) + (unsigned)a.i0[1], (unsigned)m.nx) +
                                (unsigned)a.i0[0];
      if constexpr (sizeof(E) == 4) {
        const auto lo = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(cell * 16u), 0, 0);
        const auto hi = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(cell * 16u + 16u), 0, 0);
        q.c[0][0][0] = __uint_as_float(lo[0]); q.c[0][1][0] = __uint_as_float(lo[1]);
        q.c[1][0][0] = __uint_as_float(lo[2]); q.c[1][1][0] = __uint_as_float(lo[3]);
        q.c[0][0][1] = __uint_as_float(hi[0]); q.c[0][1][1] = __uint_as_float(hi[1]);
        q.c[1][0][1] = __uint_as_float(hi[2]); q.c[1][1][1] = __uint_as_float(hi[3]);
      } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(cell * 8u), 0, 0);
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
#pragma unroll
          for (int dz = 0; dz < 2; ++dz) {
            const unsigned int u = v[2 * dx + dz];
            q.c[dz][0][dx] = __half2float(__ushort_as_half((unsigned short)(u & 0xffffu)));
            q.c[dz][1][dx] = __half2float(__ushort_as_half((unsigned short)(u >> 16)));
          }
      }
    }
    return q;
  }
  template <int D>
  __device__ __forceinline__ Real finish(const Addr &a, const Raw &q, Real (&g)[D]) const {
#pragma clang fp contract(on)  // fuse a*b+c only as written: the same arithmetic whatever the unrolling around it
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] = Real(0);
    if (!a.inside) return Real(10000);
    const Real fx = a.fr[0], fy = a.fr[1], fz = a.fr[2];
    const Real inv_res = sizeof(Real) == 4 ? (Real)m.f_inv : (Real)m.d_inv;
    const Real c000 = (Real)q.c[0][0][0], c100 = (Real)q.c[0][0][1], c010 = (Real)q.c[0][1][0], c110 = (Real)q.c[0][1][1];
    const Real c001 = (Real)q.c[1][0][0], c101 = (Real)q.c[1][0][1], c011 = (Real)q.c[1][1][0], c111 = (Real)q.c[1][1][1];
    const Real dx00 = c100 - c000, dx10 = c110 - c010, dx01 = c101 - c001, dx11 = c111 - c011;
    const Real c00 = c000 + fx * dx00, c10 = c010 + fx * dx10;
    const Real c01 = c001 + fx * dx01, c11 = c011 + fx * dx11;
    const Real c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    const Real dx0 = dx00 + fy * (dx10 - dx00), dx1 = dx01 + fy * (dx11 - dx01);
    const Real dy0 = c10 - c00, dy1 = c11 - c01;
    g[0] = (dx0 + fz * (dx1 - dx0)) * inv_res;
    g[1] = (dy0 + fz * (dy1 - dy0)) * inv_res;
    g[2] = (c1 - c0) * inv_res;
    return c0 + fz * (c1 - c0);
  }
  template <int D>
  __device__ __forceinline__ Real fetch(const Real (&pos)[D], Real (&g)[D], bool &inside) const {
    const Addr a = prepare<D>(pos);
    inside = a.inside;
    return finish<D>(a, load(a), g);
  }
};

}  // namespace neo
