// neo_backbone.hpp -- the image backbone of the learned warm start, inference only (include/neo_planner.h,
// neo_backbone_*): ResNet18OneChannel (initializer.py; nn_trainer/nn_trainer.py:119-122) from n uint8 depth images to n x 24
// fp32 features.  Every BatchNorm is folded into its convolution when the blob is packed: the device sees convolutions
// with a bias.  Activations are channels-last fp32, [image][y][x][c].
//
//   bb_stem_kernel   uint8 -> float, 7 x 7 stride-2 convolution (1 -> 64), ReLU, 3 x 3 stride-2 max pool, fused: a block
//                    computes the 17 x 9 convolution outputs under 8 x 4 pooled pixels into LDS (a lane per channel,
//                    its 49 weights in registers), then pools them
//   bb_conv_kernel   3 x 3 (stride 1 or 2, padding 1) or 1 x 1 (stride 2) convolution as an implicit GEMM on
//                    v_mfma_f32_32x32x2_f32: rows = output channels, columns = the flattened (image, y, x) of the output
//                    -- across images, so layer 4's few pixels an image still fill 32-wide tiles.  A wave owns 64
//                    channels x 32 columns (two accumulator tiles that share the activation operand), a block of four
//                    waves 64 x 128.  No LDS: a lane reads 16 consecutive input channels of its column as four 16-byte
//                    loads, a tap's group of 32 channels ahead of the MFMAs that use them, and the weights as coalesced
//                    dwords, four MFMA pairs ahead.  Epilogue: + residual, ReLU, 16-byte stores.
//   bb_pool_fc_kernel  global average pool and the 512 -> 24 fc, a block an image
//
// SUMMATION RULE.  An MFMA accumulator is bit for bit a k-ordered fmaf chain, so an output element of a convolution is ONE
// chain that starts from the folded bias and runs over the taps (ky, kx) in row-major order and, inside a tap, over the
// input channels in groups of 32, a group in the order 0, 16, 1, 17, ..., 15, 31 (the two k of an MFMA step are the lane
// halves, each holding 16 consecutive channels).  K is never split across waves or blocks, padding taps contribute
// +0 * w products, and no value depends on which other columns share a tile: an image's features depend on neither the
// batch nor the image's position in it.  No global atomics, no scratch.  The stem is one fmaf chain from its bias over
// its 49 taps row-major; the pool + fc adds a channel's pixels in ascending order, divides once, and runs an fc row as
// one chain from its bias over k ascending.
// The rule is ASSERTED, launch by launch: tests/host_harness/backbone_host.cpp restates it as plain host loops of
// std::fmaf (from this text, not from the kernels), and tests/test_gpu_backbone_launches.py requires every launch's output
// on the MI355X to equal that program's values from the same inputs (neo_backbone_activation_dev) -- which the f32 MFMA of
// gfx950 does, to the last bit, in all 171 convolution launches tested.  A change that keeps "the same bits" keeps that test.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace neo {

constexpr int kBbThreads = 256;
constexpr int kBbStemC = 64;                                      // channels of the stem
constexpr int kBbPoolW = 8, kBbPoolH = 4;                         // pooled pixels a stem block
constexpr int kBbConvW = 2 * kBbPoolW + 1, kBbConvH = 2 * kBbPoolH + 1;   // convolution outputs under them: 17 x 9
constexpr int kBbInW = 2 * (kBbConvW - 1) + 7, kBbInH = 2 * (kBbConvH - 1) + 7;   // input pixels under those: 39 x 23
constexpr int kBbInPitch = kBbInW + 1;
constexpr int kBbTileCo = 64, kBbTileCols = 128;                  // a conv block: 64 output channels x 128 columns
constexpr int kBbFcIn = 512, kBbFcOut = 24;

typedef float bb_f32x16 __attribute__((ext_vector_type(16)));

// output size of every stride-s layer of the network (7 x 7 pad 3, 3 x 3 pad 1, 1 x 1 pad 0: all (size - 1) / s + 1)
__host__ __device__ inline int bb_out_size(int size, int stride) { return (size - 1) / stride + 1; }

// images [n][H][W] uint8 -> out [n][Hp][Wp][64]; w [49][64], bias [64]; grid: n * tiles_x * tiles_y blocks
__global__ __launch_bounds__(kBbThreads) void bb_stem_kernel(const uint8_t *__restrict__ images, const float *__restrict__ w,
                                                             const float *__restrict__ bias, float *__restrict__ out, int H,
                                                             int W, int Hc, int Wc, int Hp, int Wp, int tiles_x, int tiles_y) {
  __shared__ float in_s[kBbInH * kBbInPitch];
  __shared__ float conv_s[kBbConvH * kBbConvW * kBbStemC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const int py0 = (tile / tiles_x) * kBbPoolH, px0 = (tile % tiles_x) * kBbPoolW;
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;        // first convolution output under the tile (may be -1: padding)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;        // first input pixel under that
  const uint8_t *im = images + (size_t)img * H * W;
  for (int i = tid; i < kBbInH * kBbInW; i += kBbThreads) {
    const int r = i / kBbInW, q = i - r * kBbInW;
    const int iy = iy0 + r, ix = ix0 + q;
    float v = 0.0f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = (float)im[(size_t)iy * W + ix];
    in_s[r * kBbInPitch + q] = v;
  }
  float wr[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) wr[t] = w[t * kBbStemC + lane];
  const float b = bias[lane];
  __syncthreads();
  // a lane per channel, a wave per convolution output: positions outside the convolution's output are the pool's padding
  // and hold 0, which after the ReLU never wins a window that has a real value (every window has its centre)
  for (int pos = wave; pos < kBbConvH * kBbConvW; pos += kBbThreads / 64) {
    const int r = pos / kBbConvW, q = pos - r * kBbConvW;
    const int cy = cy0 + r, cx = cx0 + q;
    float v = 0.0f;
    if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {
      float acc = b;
      const float *ip = in_s + (2 * r) * kBbInPitch + 2 * q;
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) acc = __builtin_fmaf(wr[ky * 7 + kx], ip[ky * kBbInPitch + kx], acc);
      v = fmaxf(acc, 0.0f);
    }
    conv_s[pos * kBbStemC + lane] = v;
  }
  __syncthreads();
  for (int o = tid; o < kBbPoolH * kBbPoolW * kBbStemC; o += kBbThreads) {
    const int c = o & (kBbStemC - 1), pp = o / kBbStemC;
    const int py = pp / kBbPoolW, px = pp - py * kBbPoolW;
    if (py0 + py >= Hp || px0 + px >= Wp) continue;
    float m = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, conv_s[((2 * py + dy) * kBbConvW + 2 * px + dx) * kBbStemC + c]);
    out[(((size_t)img * Hp + py0 + py) * Wp + px0 + px) * kBbStemC + c] = m;
  }
}

// what a lane holds of one tap's group of 32 input channels: its column's 16 channels (16 h .. 16 h + 15, one 64-byte
// run: the four loads of a group share their cache lines), and of a quarter of them the 2 x 4 weights
struct BbCols {
  float4 v[4];
};
struct BbWeights {
  float a0[4], a1[4];
};

// in [n][Hi][Wi][Cin] -> out [n][Ho][Wo][Cout]; w [KS][KS][Cin][Cout], bias [Cout]; resid NULL or [n][Ho][Wo][Cout]
// (it may be `out`: a lane reads the elements it writes).  Cin a power of two >= 32 (cg_shift = log2(Cin / 32)), Cout a
// multiple of 64.  grid: (ceil(n Ho Wo / 128), Cout / 64)
template <int KS>
__global__ __launch_bounds__(kBbThreads) void bb_conv_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                             const float *__restrict__ bias, const float *resid, float *out,
                                                             int ncols, int Hi, int Wi, int Cin, int cg_shift, int Ho, int Wo,
                                                             int Cout, int stride, int relu) {
  constexpr int kPad = KS / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int col = blockIdx.x * kBbTileCols + wave * 32 + r;
  const int co0 = blockIdx.y * kBbTileCo;
  const bool live = col < ncols;
  int img = 0, oy = 0, ox = 0;
  if (live) {
    img = col / (Ho * Wo);
    const int rem = col - img * (Ho * Wo);
    oy = rem / Wo;
    ox = rem - oy * Wo;
  }
  bb_f32x16 acc0, acc1;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
    acc0[g] = bias[co0 + row];
    acc1[g] = bias[co0 + 32 + row];
  }
  const float *wl = w + co0 + r;
  const int groups = Cin >> 5, steps = KS * KS * groups;      // a step: one tap's group of 32 channels, 16 MFMA pairs

  auto load_cols = [&](int s) {
    BbCols f;
    const int tap = s >> cg_shift, j = (s & (groups - 1)) << 5;
    const int ky = tap / KS, kx = tap - ky * KS;
    const int iy = oy * stride + ky - kPad, ix = ox * stride + kx - kPad;
    const bool ok = live && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
    const float4 *ip = reinterpret_cast<const float4 *>(in + (((size_t)img * Hi + iy) * Wi + ix) * Cin + j + 16 * h);
#pragma unroll
    for (int q = 0; q < 4; ++q) f.v[q] = ok ? ip[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return f;
  };
  // quarter q4 = 4 s + q of the flattened (tap, group, quarter): channels j + 16 h + 4 q .. + 3 of the tap's rows of W
  auto load_weights = [&](int q4) {
    BbWeights f;
    const int s = q4 >> 2, q = q4 & 3;
    const int tap = s >> cg_shift, j = (s & (groups - 1)) << 5;
    const float *wt = wl + ((size_t)tap * Cin + j + 16 * h + 4 * q) * Cout;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f.a0[t] = wt[(size_t)t * Cout];
      f.a1[t] = wt[(size_t)t * Cout + 32];
    }
    return f;
  };

  BbCols cols = load_cols(0);
  BbWeights wts = load_weights(0);
  for (int s = 0; s < steps; ++s) {
    BbCols cols_next = cols;
    if (s + 1 < steps) cols_next = load_cols(s + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      BbWeights wts_next = wts;
      if (4 * s + q + 1 < 4 * steps) wts_next = load_weights(4 * s + q + 1);
      const float bv[4] = {cols.v[q].x, cols.v[q].y, cols.v[q].z, cols.v[q].w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wts.a0[t], bv[t], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wts.a1[t], bv[t], acc1, 0, 0, 0);
      }
      wts = wts_next;
    }
    cols = cols_next;
  }

  if (!live) return;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const bb_f32x16 &a = half ? acc1 : acc0;
      float4 v = make_float4(a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]);
      const size_t o = (size_t)col * Cout + co0 + 32 * half + 8 * g + 4 * h;
      if (resid) {
        const float4 q = *reinterpret_cast<const float4 *>(resid + o);
        v.x += q.x;
        v.y += q.y;
        v.z += q.z;
        v.w += q.w;
      }
      if (relu) {
        v.x = fmaxf(v.x, 0.0f);
        v.y = fmaxf(v.y, 0.0f);
        v.z = fmaxf(v.z, 0.0f);
        v.w = fmaxf(v.w, 0.0f);
      }
      *reinterpret_cast<float4 *>(out + o) = v;
    }
  }
}

// in [n][P][512] -> feature [n][24]: a lane sums its channel over the P pixels in ascending order and divides by P, then
// lane j < 24 runs fc row j as one fmaf chain from its bias over the 512 means in ascending order.  A block an image.
__global__ __launch_bounds__(kBbThreads) void bb_pool_fc_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                                const float *__restrict__ bias, float *__restrict__ feature,
                                                                int P) {
  __shared__ float mean_s[kBbFcIn];
  const int tid = threadIdx.x;
  const float *x = in + (size_t)blockIdx.x * P * kBbFcIn;
  for (int c = tid; c < kBbFcIn; c += kBbThreads) {
    float s = 0.0f;
    for (int p = 0; p < P; ++p) s += x[(size_t)p * kBbFcIn + c];
    mean_s[c] = s / (float)P;
  }
  __syncthreads();
  if (tid < kBbFcOut) {
    float acc = bias[tid];
    const float *wr = w + tid * kBbFcIn;
    for (int k = 0; k < kBbFcIn; ++k) acc = __builtin_fmaf(wr[k], mean_s[k], acc);
    feature[(size_t)blockIdx.x * kBbFcOut + tid] = acc;
  }
}

}  // namespace neo
