// neo_disp_depth.hip -- the batched depth camera (neo_depth.hpp): the pixel tables, the render pass (depth_m and the
// images' maxima) and the normalise pass (depth_u8) of one neo_depth_render_batch_dev call
#include "neo_host.hpp"
#include "neo_depth.hpp"

namespace neo {

int depth_render(neo_ctx *c, const DepthCall &k) {
  DepthState &st = c->depth;
  const int Wp = (k.W + 3) & ~3;
  if (!st.uv) HIPCHK(c, hipMalloc(&st.uv, sizeof(float) * 2 * kDepthMaxSide));
  unsigned *max_bits = reinterpret_cast<unsigned *>(k.depth_max);
  if (!max_bits) {  // the normalise pass needs the maxima even when the caller does not
    if ((size_t)k.B > st.max_cap) {
      if (st.max_bits) hipFree(st.max_bits);
      st.max_bits = nullptr;
      st.max_cap = 0;
      HIPCHK(c, hipMalloc(&st.max_bits, sizeof(unsigned) * (size_t)k.B));
      st.max_cap = (size_t)k.B;
    }
    max_bits = st.max_bits;
  }
  DepthArgs a{};
  a.W = k.W, a.H = k.H, a.n_scenes = k.n_scenes, a.B = k.B;
  a.max_range = (float)k.max_range;
  a.boxes = k.boxes, a.box_begin = k.box_begin, a.scene_index = k.scene_index, a.pose = k.pose;
  a.u = st.uv, a.v = st.uv + Wp;
  a.depth_m = k.depth_m, a.depth_u8 = k.depth_u8, a.max_bits = max_bits;
  a.box_tests = st.box_tests;
  const size_t hw = (size_t)k.W * k.H;
  const bool m16 = reinterpret_cast<uintptr_t>(k.depth_m) % 16 == 0;
  a.vec_m = m16 && k.W % 4 == 0;
  a.vec_u8 = m16 && hw % 4 == 0 && reinterpret_cast<uintptr_t>(k.depth_u8) % 4 == 0;

  hipLaunchKernelGGL(depth_uv_kernel, dim3((Wp + k.H + kDepthThreads - 1) / kDepthThreads), dim3(kDepthThreads), 0,
                     c->stream, k.W, k.H, k.focal, st.uv, st.uv + Wp);
  HIPCHK(c, hipMemsetAsync(max_bits, 0, sizeof(unsigned) * (size_t)k.B, c->stream));
  const int tiles_x = (k.W + kDepthTileW - 1) / kDepthTileW, tiles_y = (k.H + kDepthTileH - 1) / kDepthTileH;
  const int quads = (int)((hw + 4 * (size_t)kDepthThreads - 1) / (4 * (size_t)kDepthThreads));
  constexpr int kImagesPerLaunch = 32768;  // grid.y
  for (int b0 = 0; b0 < k.B; b0 += kImagesPerLaunch) {
    const int nimg = std::min(kImagesPerLaunch, k.B - b0);
    hipLaunchKernelGGL(depth_render_kernel, dim3(tiles_x * tiles_y, nimg), dim3(kDepthThreads), 0, c->stream, a, b0, tiles_x);
    if (k.depth_u8)
      hipLaunchKernelGGL(depth_norm_kernel, dim3(quads, nimg), dim3(kDepthThreads), 0, c->stream, a, b0);
  }
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

void depth_release(neo_ctx *c) {
  if (c->depth.uv) hipFree(c->depth.uv);
  if (c->depth.max_bits) hipFree(c->depth.max_bits);
  c->depth = DepthState{};
}

}  // namespace neo
