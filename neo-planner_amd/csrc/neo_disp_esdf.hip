// neo_disp_esdf.hip -- the map kernels' launches (neo_esdf.hpp): 2-D build and pack, 3-D EDT and pack, point query.
// Every entry point launches on the context's stream, on device arrays the caller (neo_abi.hip) carved, and allocates
// nothing; arguments were checked there.
#include "neo_host.hpp"
#include "neo_esdf.hpp"

namespace neo {

void esdf_build_2d(neo_ctx *c, const Edt2DWork &w, int W, int H, double res, double4 *rec) {
  const size_t ncell = (size_t)W * H;
  if (W <= 512 && H <= 512) {
    const dim3 grid((W + 63) / 64, H);
    hipLaunchKernelGGL(edt2_columns_bf_kernel, grid, dim3(64), 0, c->stream, w.occ, W, H, w.g);
    hipLaunchKernelGGL(edt2_rows_bf_kernel, grid, dim3(64), 0, c->stream, w.g, W, H, res, w.dist);
  } else {
    hipLaunchKernelGGL(edt_columns_kernel, dim3((W + 63) / 64), dim3(64), 0, c->stream, w.occ, W, H, w.g);
    hipLaunchKernelGGL(edt_rows_kernel, dim3((H + 63) / 64), dim3(64), 0, c->stream, w.g, W, H, res, w.v, w.z, w.dist);
  }
  hipLaunchKernelGGL(gradient_pack_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream, w.dist, W, H,
                     rec, nullptr, w.gx, w.gy);
}

// the same launches with the maps of a batch in the grid (at most 65535 a call: grid.y / grid.z)
void esdf_build_2d_batch(neo_ctx *c, const Edt2DWork &w, int nmap, int W, int H, double res, double4 *const *recs) {
  const size_t ncell = (size_t)W * H;
  const unsigned nm = (unsigned)nmap;
  // The column pass is always the sweep, one lane per column: a batch has the columns of all its maps to fill the machine
  // with, and the exhaustive column kernel was two thirds of a batch's time (4096 maps of 300 x 300: 88.4 ms with it,
  // 27.5 ms with the sweep; the row sweep as well: 32.3 ms -- `tools/gpu_onboard_time.py rebuild`).  Both give the same integers.  Rows: exhaustive up to
  // 512 x 512, the sweep beyond, as for one map.
  hipLaunchKernelGGL(edt_columns_kernel, dim3((W + 63) / 64, nm), dim3(64), 0, c->stream, w.occ, W, H, w.g);
  if (W <= 512 && H <= 512) {
    hipLaunchKernelGGL(edt2_rows_bf_kernel, dim3((W + 63) / 64, H, nm), dim3(64), 0, c->stream, w.g, W, H, res, w.dist);
  } else {
    hipLaunchKernelGGL(edt_rows_kernel, dim3((H + 63) / 64, nm), dim3(64), 0, c->stream, w.g, W, H, res, w.v, w.z, w.dist);
  }
  hipLaunchKernelGGL(gradient_pack_kernel, dim3((unsigned)((ncell + 255) / 256), nm), dim3(256), 0, c->stream, w.dist, W, H,
                     nullptr, recs, nullptr, nullptr);
}

void esdf_pack_2d(neo_ctx *c, const double *dist, const double *gx, const double *gy, size_t ncell, double4 *rec) {
  hipLaunchKernelGGL(pack2d_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream, dist, gx, gy,
                     (int)ncell, rec);
}

// f(Type<SrcT>, Type<DstT>) for the source and stored element types of a 3-D field: double | float into float | __half
// (neo_esdf_upload_3d admits nothing else)
template <class F>
static void visit_pack_types(int src_dtype, int store_dtype, F f) {
  if (src_dtype == NEO_F64 && store_dtype == NEO_F32) f(Type<double>{}, Type<float>{});
  else if (src_dtype == NEO_F64) f(Type<double>{}, Type<__half>{});
  else if (store_dtype == NEO_F32) f(Type<float>{}, Type<float>{});
  else f(Type<float>{}, Type<__half>{});
}

void esdf_pack_3d(neo_ctx *c, const void *src, int src_dtype, int nx, int ny, int nz, int store_dtype, int layout, int nbx,
                  int nby, int nbz, void *dst) {
  const size_t nvox = (size_t)nx * ny * nz;
  const dim3 grid((unsigned)((nvox + 255) / 256)), blk(256);
  visit_pack_types(src_dtype, store_dtype, [&](auto s, auto d) {
    using SrcT = type_of<decltype(s)>;
    using DstT = type_of<decltype(d)>;
    const SrcT *in = static_cast<const SrcT *>(src);
    DstT *out = static_cast<DstT *>(dst);
    if (layout == NEO_LAYOUT_BRICK) {
      const dim3 gb((unsigned)((nbx + kBrickXB - 1) / kBrickXB), (unsigned)nby, (unsigned)nbz);
      hipLaunchKernelGGL((pack3d_brick_kernel<SrcT, DstT>), gb, blk, 0, c->stream, in, nx, ny, nz, nbx, nby, out);
    } else if (layout == NEO_LAYOUT_CELL8) {
      hipLaunchKernelGGL((pack3d_cell8_kernel<SrcT, DstT>), grid, blk, 0, c->stream, in, nx, ny, nz, out);
    } else if (layout == NEO_LAYOUT_YZ4) {
      hipLaunchKernelGGL((pack3d_yz4_kernel<SrcT, DstT>), grid, blk, 0, c->stream, in, nx, ny, nz, out);
    } else {
      hipLaunchKernelGGL((pack3d_kernel<SrcT, DstT>), grid, blk, 0, c->stream, in, nx, ny, nz, out);
    }
  });
}

// ---- the y / z passes of the 3-D EDT: TX x-columns by the whole line in LDS
// tiles of at most 64 KB of LDS INCLUDING the general kernel's 2 KB of static part_best / part_arg
constexpr size_t kEdtTile = 65536 - 2 * kEdtThreads * sizeof(int);
constexpr int kEdtMaxLine = 4096;  // neo_esdf_build_3d admits no longer axis

// Columns of a general-form tile for lines of `nline` voxels: 16 (measured at 300^3: y pass 248 -> 204 us, z pass 384 ->
// 252 us against 32 columns; 8 columns in the z pass: 278) while they fit at the z pass' 6 bytes a voxel, else the widest
// narrower tile that does.  The y pass stores 4 bytes a voxel and takes the same widths.
constexpr int edt_tile_columns(int nline) {
  return (size_t)nline * 16 * 6 <= kEdtTile ? 16 : ((size_t)nline * 8 * 6 <= kEdtTile ? 8 : 2);
}
static_assert(edt_tile_columns(661) == 16 && edt_tile_columns(662) == 8, "last 16-column line: 661 * 96 = 63456 bytes");
static_assert(edt_tile_columns(1322) == 8 && edt_tile_columns(1323) == 2, "last 8-column line");
static_assert(edt_tile_columns(kEdtMaxLine) == 2 && (size_t)kEdtMaxLine * 2 * 6 <= kEdtTile, "the longest line fits a 2-column tile");

// Bits of the minimiser field of the packed keys for lines of `nline` voxels in a volume of squared diagonal (+ 1)
// `diag2`, or 0 when the keys do not fit: (squared diagonal + 2 nline^2) << bits(nline) must stay below 2^31
constexpr int key_bits(long long diag2, int nline) {
  int qb = 1;
  while ((1 << qb) < nline) ++qb;
  const long long span = (diag2 + 2LL * nline * nline) << qb;
  return (span < (1LL << 31) && ((long long)nline << (qb + 1)) < (1LL << 23)) ? qb : 0;
}
// The packed-key tile is always 16 columns of 4 bytes a voxel.  The other two axes hold 2 voxels or more, so diag2 >=
// nline^2 + 9, and the longest line the keys admit is 836 voxels: it fits.
constexpr int kKeyTX = 16, kKeyMaxLine = 836;
static_assert(key_bits((long long)kKeyMaxLine * kKeyMaxLine + 9, kKeyMaxLine) == 10 &&
              key_bits((long long)(kKeyMaxLine + 1) * (kKeyMaxLine + 1) + 9, kKeyMaxLine + 1) == 0, "836 is the longest key line");
static_assert((size_t)kKeyMaxLine * kKeyTX * sizeof(int) <= kEdtTile, "and its 16-column tile fits");

// one line pass: lines of `nline` voxels `sline` elements apart, `nslab` slabs `sslab` elements apart
template <typename SrcT>
struct LinePass {
  const SrcT *src;
  int nx, nline;
  size_t sline, sslab;
  int nslab;
  double res;
  uint32_t *out_sq;  // the y pass' plane distances (squared), or
  float *out_dist;   // the z pass' distances (FINAL)
};

template <typename SrcT, int TX, bool FINAL>
static void launch_line(neo_ctx *c, const LinePass<SrcT> &p) {
  hipLaunchKernelGGL((edt3_line_kernel<SrcT, TX, FINAL>), dim3((unsigned)((p.nx + TX - 1) / TX), (unsigned)p.nslab),
                     dim3(kEdtThreads), (size_t)p.nline * TX * (sizeof(SrcT) == 2 ? 4 : 6), c->stream, p.src, p.nx, p.nline,
                     p.sline, p.sslab, p.res, p.out_sq, p.out_dist);
}

template <typename SrcT, int TX, bool FINAL>
static void launch_line_keys(neo_ctx *c, const LinePass<SrcT> &p, int big, int qb) {
  hipLaunchKernelGGL((edt3_line_keys_kernel<SrcT, TX, FINAL>), dim3((unsigned)(((p.nx + TX - 1) / TX) * ((p.nslab + 7) / 8) * 8)),
                     dim3(kEdtThreads), (size_t)p.nline * TX * sizeof(int), c->stream, p.src, p.nx, p.nline, p.sline, p.sslab,
                     p.nslab, p.res, big, qb, p.out_sq, p.out_dist);
}

// packed keys where they fit (qb != 0), else the general form at the widest tile the line allows
template <typename SrcT, bool FINAL>
static void line_pass(neo_ctx *c, const LinePass<SrcT> &p, int big, int qb) {
  if (qb) return launch_line_keys<SrcT, kKeyTX, FINAL>(c, p, big, qb);
  switch (edt_tile_columns(p.nline)) {
    case 16: return launch_line<SrcT, 16, FINAL>(c, p);
    case 8: return launch_line<SrcT, 8, FINAL>(c, p);
    default: return launch_line<SrcT, 2, FINAL>(c, p);
  }
}

void esdf_edt_3d(neo_ctx *c, const uint8_t *occ, int nx, int ny, int nz, double res, uint16_t *gx, uint32_t *sq, float *dist) {
  const size_t rows = (size_t)ny * nz;
  const dim3 xgrid((unsigned)((rows + 3) / 4));
  // (the occupancy's rows must be 4-byte aligned for the wide form: nx a multiple of four and an aligned base)
  const bool wide = nx % 4 == 0 && (reinterpret_cast<uintptr_t>(occ) & 3) == 0;
  if (wide && nx <= 8 * kWave)
    hipLaunchKernelGGL(edt3_xv_kernel<8>, xgrid, dim3(256), 0, c->stream, occ, nx, rows, gx);
  else if (wide && nx <= 16 * kWave)
    hipLaunchKernelGGL(edt3_xv_kernel<16>, xgrid, dim3(256), 0, c->stream, occ, nx, rows, gx);
  else
    hipLaunchKernelGGL(edt3_x_kernel, xgrid, dim3(256), 4 * (size_t)nx * sizeof(uint16_t), c->stream, occ, nx, rows, gx);
  const size_t plane = (size_t)nx * ny;
  const long long diag2 = (long long)nx * nx + (long long)ny * ny + (long long)nz * nz + 1;
  const int big = (int)std::min<long long>(diag2, 1 << 30);
  // (neo_esdf_build_config(ctx, NEO_EDT_GENERIC_LINES): the general form for every volume -- the tests run both)
  const bool generic = (c->edt_flags & NEO_EDT_GENERIC_LINES) != 0;
  // pass Y: lines along y (stride nx) in every z slab; pass Z: lines along z (stride nx * ny) for every y row
  line_pass<uint16_t, false>(c, {gx, nx, ny, (size_t)nx, plane, nz, res, sq, nullptr}, big, generic ? 0 : key_bits(diag2, ny));
  line_pass<uint32_t, true>(c, {sq, nx, nz, plane, (size_t)nx, ny, res, nullptr, dist}, big, generic ? 0 : key_bits(diag2, nz));
}

void esdf_query(neo_ctx *c, const MapEntry &e, int n, const double *pts, double *dist, double *grad) {
  const dim3 grid((n + 127) / 128), blk(128);
  if (e.kind == 0)
    hipLaunchKernelGGL((query_kernel<double, Map2D, Lookup2D<double>, 2>), grid, blk, 0, c->stream, n, e.m2, pts, dist, grad);
  else if (e.elem == NEO_F32)
    hipLaunchKernelGGL((query_kernel<double, Map3D, Lookup3D<double, float, 9>, 3>), grid, blk, 0, c->stream, n, e.m3, pts, dist, grad);
  else
    hipLaunchKernelGGL((query_kernel<double, Map3D, Lookup3D<double, __half, 9>, 3>), grid, blk, 0, c->stream, n, e.m3, pts, dist, grad);
}

}  // namespace neo
