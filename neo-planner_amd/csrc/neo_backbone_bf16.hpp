// neo_backbone_bf16.hpp -- the image backbone of the learned warm start with bf16 storage and the bf16 matrix cores
// (include/neo_planner.h, neo_backbone_*bf16*): the same ResNet18OneChannel, the same 21 launches and the same forward
// order as neo_backbone.hpp, from n uint8 depth images to n x 24 fp32 features.  A second, opt-in route: this header
// shares no text with the fp32 one, whose kernels and bits stay as they are.
//
// PACKED BLOB (NEO_BACKBONE_BF16_BYTES = 22 396 000 bytes; bb_pack_bf16_kernel makes it from the fp32 blob, and
// initializer.pack_backbone_weights_bf16 is its NumPy twin, written from this text).  The parts follow each other in the
// fp32 blob's order -- the stem, the eight blocks (conv1, conv2, then the downsample branch where there is one), the fc --
// without padding; every part starts 16-byte aligned because every part's size is a multiple of 16 bytes:
//   the stem           W [49][64] fp32, b [64] fp32, copied verbatim
//   a convolution      W as bf16 in the layout [ky][kx][cin / 8][cout][8]: the value at [ky][kx][g][co][j] is the fp32
//                      blob's W[ky][kx][ci = 8 g + j][co], rounded to nearest even; then b [cout] fp32, verbatim
//   the fc             W [24][512] fp32, b [24] fp32, verbatim
// 11 157 504 bf16 values and 20 248 floats.  The 8 consecutive input channels of one output channel are one 16-byte
// run: an A fragment of v_mfma_f32_32x32x16_bf16 (row = output channel, 8 consecutive k) is one 16-byte load.
//
// ACTIVATIONS are channels-last bf16, [image][y][x][c]; a lane's B fragment (its column's 8 consecutive channels) is
// one 16-byte load.  The workspace is three such buffers (neo_backbone_bf16_workspace_bytes).
//
//   bb_pack_bf16_kernel   one convolution's W, fp32 [ky][kx][ci][co] -> bf16 [ky][kx][ci / 8][co][8]
//   bb_stem_bf16_kernel   the fp32 stem's arithmetic (uint8 -> float, 7 x 7 stride 2 as one fp32 fmaf chain from the bias
//                         over the 49 taps row-major, ReLU, 3 x 3 stride-2 max pool); the pooled value is rounded ONCE, at
//                         the store
//   bb_conv_bf16_kernel   3 x 3 (stride 1 or 2, padding 1) or 1 x 1 (stride 2) convolution as an implicit GEMM on
//                         v_mfma_f32_32x32x16_bf16: rows = output channels, columns = the flattened (image, y, x) of the
//                         output, across images.  A block of four waves owns kBhTileCo = 64 channels x kBhTileCols = 128
//                         columns; a wave 64 channels x 32 columns, two accumulator tiles that share the activation
//                         fragment.  K advances in steps of kBhStepK = 64 (a tap's 64 input channels: four MFMA pairs).
//                         The block's weight tile of a step (8 channel groups x 64 channels x 16 bytes = 8 KB) is staged
//                         in LDS, double buffered, one barrier a step, and every wave reads its A fragments from there as
//                         lane-contiguous 16-byte reads; a lane reads its column's activations from global memory, 16
//                         bytes a k-step, one step ahead.  Epilogue in fp32: + residual (bf16, widened), ReLU, round to
//                         bf16, 16-byte stores.
//   bb_pool_fc_bf16_kernel  global average pool and the fc: reads bf16, computes in fp32 exactly as the fp32 kernel,
//                         writes fp32 features
//
// ROWS OF A TILE.  The C/D layout gives lane (r = lane & 31, h = lane >> 5) the rows (reg & 3) + 8 (reg >> 2) + 4 h of
// column r.  Which output channel a row holds is free, so row m of accumulator tile t holds channel
//   co0 + 16 (m >> 3) + 8 ((m >> 2) & 1) + 4 t + (m & 3):
// registers 4 g .. 4 g + 3 of the two tiles are then the 8 consecutive channels co0 + 16 g + 8 h .. + 7 of the lane's
// column, one 16-byte store (and one 16-byte residual load).  The permutation is applied where the weight tile is
// written to LDS.
//
// WHAT IS PROMISED ABOUT THE SUM.  An output element's accumulator is fp32 and starts from the fp32 bias.  K runs over
// the taps (ky, kx) row-major and, inside a tap, over the input channels ascending, 16 an instruction; K is never split
// across waves or blocks; a padding tap contributes zeros; no value depends on which other columns share a tile, so an
// image's features depend on neither the batch nor the image's position in it.  A product of two bf16 values is exact
// in fp32, so a launch's fp32 value differs from the exact sum of its products only by the accumulation's rounding.
// What is NOT promised: how the instruction sums its 16 products and adds them to the accumulator -- unlike the f32
// instruction of the fp32 route it is not asserted to be a k-ordered fmaf chain.  The test holds every launch to the
// bound of ANY fp32 accumulation of K + 2 terms instead (tests/test_gpu_backbone_bf16.py), and the stored bf16 bits to
// round-to-nearest-even of the fp32 value (the debug epilogue below hands that value out).  No global atomics, no scratch.
//
// DEBUG EPILOGUE.  The stem and the convolution take `dbg`: NULL, or an fp32 array of the output's shape, into which
// the same launch also writes the value it is about to round, on the same path up to the store
// (neo_backbone_bf16_activation_dev only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace neo {

constexpr int kBhThreads = 256;
constexpr int kBhStemC = 64;                                      // channels of the stem
constexpr int kBhPoolW = 8, kBhPoolH = 4;                         // pooled pixels a stem block
constexpr int kBhConvW = 2 * kBhPoolW + 1, kBhConvH = 2 * kBhPoolH + 1;   // convolution outputs under them: 17 x 9
constexpr int kBhInW = 2 * (kBhConvW - 1) + 7, kBhInH = 2 * (kBhConvH - 1) + 7;   // input pixels under those: 39 x 23
constexpr int kBhInPitch = kBhInW + 1;
constexpr int kBhTileCo = 64;                                     // a conv block: 64 output channels ...
constexpr int kBhTileCols = 128;                                  // ... x 128 columns (the tests read this line)
constexpr int kBhStepK = 64;                                      // input channels of one tap a step of the K loop
constexpr int kBhStepBytes = (kBhStepK / 8) * kBhTileCo * 16;     // the weight tile of a step in LDS: 8 KB
constexpr int kBhFcIn = 512, kBhFcOut = 24;

typedef float bh_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bh_bf16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ inline int bh_out_size(int size, int stride) { return (size - 1) / stride + 1; }

__device__ inline float bh_widen(__bf16 v) { return (float)v; }

// one convolution's weights: w32 [taps][cin][cout] fp32 -> w16 [taps][cin / 8][cout][8] bf16, a thread a 16-byte run
__global__ __launch_bounds__(kBhThreads) void bb_pack_bf16_kernel(const float *__restrict__ w32, __bf16 *__restrict__ w16,
                                                                  int taps, int cin, int cout) {
  const size_t runs = (size_t)taps * (cin >> 3) * cout;
  const size_t e = (size_t)blockIdx.x * kBhThreads + threadIdx.x;
  if (e >= runs) return;
  const int co = (int)(e % cout);
  const size_t tg = e / cout;                      // tap * (cin / 8) + g: 8 tg is the row tap * cin + 8 g of w32
  bh_bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (__bf16)w32[(tg * 8 + j) * cout + co];
  *reinterpret_cast<bh_bf16x8 *>(w16 + e * 8) = v;
}

// images [n][H][W] uint8 -> out [n][Hp][Wp][64] bf16; w [49][64], bias [64] fp32; grid: n * tiles_x * tiles_y blocks
__global__ __launch_bounds__(kBhThreads) void bb_stem_bf16_kernel(const uint8_t *__restrict__ images,
                                                                  const float *__restrict__ w, const float *__restrict__ bias,
                                                                  __bf16 *__restrict__ out, float *__restrict__ dbg, int H,
                                                                  int W, int Hc, int Wc, int Hp, int Wp, int tiles_x,
                                                                  int tiles_y) {
  __shared__ float in_s[kBhInH * kBhInPitch];
  __shared__ float conv_s[kBhConvH * kBhConvW * kBhStemC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const int py0 = (tile / tiles_x) * kBhPoolH, px0 = (tile % tiles_x) * kBhPoolW;
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;        // first convolution output under the tile (may be -1: padding)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;        // first input pixel under that
  const uint8_t *im = images + (size_t)img * H * W;
  for (int i = tid; i < kBhInH * kBhInW; i += kBhThreads) {
    const int r = i / kBhInW, q = i - r * kBhInW;
    const int iy = iy0 + r, ix = ix0 + q;
    float v = 0.0f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = (float)im[(size_t)iy * W + ix];
    in_s[r * kBhInPitch + q] = v;
  }
  float wr[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) wr[t] = w[t * kBhStemC + lane];
  const float b = bias[lane];
  __syncthreads();
  // a lane per channel, a wave per convolution output: positions outside the convolution's output are the pool's padding
  // and hold 0, which after the ReLU never wins a window that has a real value (every window has its centre)
  for (int pos = wave; pos < kBhConvH * kBhConvW; pos += kBhThreads / 64) {
    const int r = pos / kBhConvW, q = pos - r * kBhConvW;
    const int cy = cy0 + r, cx = cx0 + q;
    float v = 0.0f;
    if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {
      float acc = b;
      const float *ip = in_s + (2 * r) * kBhInPitch + 2 * q;
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) acc = __builtin_fmaf(wr[ky * 7 + kx], ip[ky * kBhInPitch + kx], acc);
      v = fmaxf(acc, 0.0f);
    }
    conv_s[pos * kBhStemC + lane] = v;
  }
  __syncthreads();
  for (int o = tid; o < kBhPoolH * kBhPoolW * kBhStemC; o += kBhThreads) {
    const int c = o & (kBhStemC - 1), pp = o / kBhStemC;
    const int py = pp / kBhPoolW, px = pp - py * kBhPoolW;
    if (py0 + py >= Hp || px0 + px >= Wp) continue;
    float m = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, conv_s[((2 * py + dy) * kBhConvW + 2 * px + dx) * kBhStemC + c]);
    const size_t at = (((size_t)img * Hp + py0 + py) * Wp + px0 + px) * kBhStemC + c;
    if (dbg) dbg[at] = m;
    out[at] = (__bf16)m;
  }
}

// in [n][Hi][Wi][Cin] bf16 -> out [n][Ho][Wo][Cout] bf16; w [KS][KS][Cin / 8][Cout][8] bf16, bias [Cout] fp32; resid NULL
// or [n][Ho][Wo][Cout] bf16 (it may be `out`: the lane that writes an element is the one that read its residual, and it
// reads first); dbg NULL or [n][Ho][Wo][Cout] fp32.  Cin a power of two >= 64 (cs_shift = log2(Cin / 64)), Cout a
// multiple of 64.  grid: (ceil(n Ho Wo / 128), Cout / 64)
template <int KS>
__global__ __launch_bounds__(kBhThreads) void bb_conv_bf16_kernel(const __bf16 *__restrict__ in, const __bf16 *__restrict__ w,
                                                                  const float *__restrict__ bias, const __bf16 *resid,
                                                                  __bf16 *out, float *__restrict__ dbg, int ncols, int Hi,
                                                                  int Wi, int Cin, int cs_shift, int Ho, int Wo, int Cout,
                                                                  int stride, int relu) {
  constexpr int kPad = KS / 2;
  __shared__ __attribute__((aligned(16))) unsigned char w_s[2][kBhStepBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int col = blockIdx.x * kBhTileCols + wave * 32 + r;
  const int co0 = blockIdx.y * kBhTileCo;
  const bool live = col < ncols;
  int img = 0, oy = 0, ox = 0;
  if (live) {
    img = col / (Ho * Wo);
    const int rem = col - img * (Ho * Wo);
    oy = rem / Wo;
    ox = rem - oy * Wo;
  }
  bh_f32x16 acc0, acc1;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int ch = 16 * (g >> 2) + 8 * h + (g & 3);
    acc0[g] = bias[co0 + ch];
    acc1[g] = bias[co0 + ch + 4];
  }
  const int chunks = Cin >> 6, steps = KS * KS * chunks;      // a step: 64 channels of one tap, four MFMA pairs

  // the weight tile of step s: groups 8 (s's chunk) .. + 7 of its tap, channels co0 .. co0 + 63, 512 runs of 16 bytes, two
  // a thread; run (gl, c) goes to slot gl * 64 + t * 32 + m of the LDS image (ROWS OF A TILE: c = 16 (m >> 3) + 8 ((m >> 2)
  // & 1) + 4 t + (m & 3))
  const int gl0 = tid >> 6, c = tid & 63;
  const int slot = ((c >> 2) & 1) * 32 + 8 * (c >> 4) + 4 * ((c >> 3) & 1) + (c & 3);
  const uint4 *wg = reinterpret_cast<const uint4 *>(w) + co0 + c;
  auto load_weights = [&](int s, uint4 &a, uint4 &b) {
    const size_t g = (size_t)s * 8 + gl0;        // tap * (Cin / 8) + the group: the steps of a tap follow each other
    a = wg[g * Cout];
    b = wg[(g + 4) * Cout];
  };
  auto store_weights = [&](int buf, const uint4 &a, const uint4 &b) {
    uint4 *ws = reinterpret_cast<uint4 *>(w_s[buf]);
    ws[gl0 * 64 + slot] = a;
    ws[(gl0 + 4) * 64 + slot] = b;
  };
  struct Cols {
    bh_bf16x8 v[4];
  };
  auto load_cols = [&](int s) {
    Cols f;
    const int tap = s >> cs_shift, j = (s & (chunks - 1)) << 6;
    const int ky = tap / KS, kx = tap - ky * KS;
    const int iy = oy * stride + ky - kPad, ix = ox * stride + kx - kPad;
    const bool ok = live && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
    const bh_bf16x8 *ip = reinterpret_cast<const bh_bf16x8 *>(in + (((size_t)img * Hi + iy) * Wi + ix) * Cin + j + 8 * h);
    const bh_bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) f.v[q] = ok ? ip[2 * q] : zero;
    return f;
  };

  uint4 wa, wb;
  load_weights(0, wa, wb);
  Cols cols = load_cols(0);
  store_weights(0, wa, wb);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    Cols cols_next = cols;
    if (s + 1 < steps) {
      load_weights(s + 1, wa, wb);
      cols_next = load_cols(s + 1);
    }
    const bh_bf16x8 *ws = reinterpret_cast<const bh_bf16x8 *>(w_s[s & 1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bh_bf16x8 a0 = ws[(2 * q + h) * 64 + r], a1 = ws[(2 * q + h) * 64 + 32 + r];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, cols.v[q], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, cols.v[q], acc1, 0, 0, 0);
    }
    // (the other buffer was last read in step s - 1, which every wave left through the barrier below)
    if (s + 1 < steps) store_weights((s + 1) & 1, wa, wb);
    __syncthreads();
    cols = cols_next;
  }

  if (!live) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = acc0[4 * g + i], v[4 + i] = acc1[4 * g + i];
    const size_t o = (size_t)col * Cout + co0 + 16 * g + 8 * h;
    if (resid) {
      const bh_bf16x8 q = *reinterpret_cast<const bh_bf16x8 *>(resid + o);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += bh_widen(q[i]);
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.0f);
    }
    if (dbg) {
      *reinterpret_cast<float4 *>(dbg + o) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4 *>(dbg + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    bh_bf16x8 p;
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (__bf16)v[i];
    *reinterpret_cast<bh_bf16x8 *>(out + o) = p;
  }
}

// in [n][P][512] bf16 -> feature [n][24] fp32: a lane sums its channel over the P pixels in ascending order (fp32) and
// divides by P, then lane j < 24 runs fc row j as one fmaf chain from its bias over the 512 means in ascending order.
__global__ __launch_bounds__(kBhThreads) void bb_pool_fc_bf16_kernel(const __bf16 *__restrict__ in, const float *__restrict__ w,
                                                                     const float *__restrict__ bias,
                                                                     float *__restrict__ feature, int P) {
  __shared__ float mean_s[kBhFcIn];
  const int tid = threadIdx.x;
  const __bf16 *x = in + (size_t)blockIdx.x * P * kBhFcIn;
  for (int c = tid; c < kBhFcIn; c += kBhThreads) {
    float s = 0.0f;
    for (int p = 0; p < P; ++p) s += bh_widen(x[(size_t)p * kBhFcIn + c]);
    mean_s[c] = s / (float)P;
  }
  __syncthreads();
  if (tid < kBhFcOut) {
    float acc = bias[tid];
    const float *wr = w + tid * kBhFcIn;
    for (int k = 0; k < kBhFcIn; ++k) acc = __builtin_fmaf(wr[k], mean_s[k], acc);
    feature[(size_t)blockIdx.x * kBhFcOut + tid] = acc;
  }
}

}  // namespace neo
