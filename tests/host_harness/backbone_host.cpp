// TEST HARNESS ONLY (built by tests/test_backbone_chain.py with g++, never part of the product library): the SUMMATION
// RULE of the image backbone (the header comment of csrc/neo_backbone.hpp, include/neo_planner.h) restated as plain
// nested loops on the host.  It includes nothing of csrc/: it is written from the rule's text, not from the kernels, so
// that the tests can hold the kernels to the rule.  Every accumulation is one std::fmaf in fp32 in the stated order;
// built with -ffp-contract=off, so nothing else is fused.  Arrays are the device's: activations channels-last
// [image][y][x][c], a convolution's W [ky][kx][ci][co], the fc's W [24][512].
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

inline int out_size(int size, int stride) { return (size - 1) / stride + 1; }
inline float relu(float v) { return v > 0.0f ? v : 0.0f; }

}  // namespace

extern "C" {

// images [n][H][W] uint8 -> out [n][Hp][Wp][64]: the 7 x 7 stride-2 padding-3 convolution as one chain from the bias over
// (ky, kx) row-major on the pixel values as floats (padding pixels are 0), ReLU, then the 3 x 3 stride-2 padding-1 max
// over the convolution outputs that exist and 0
void bb_host_stem(const uint8_t *images, const float *w, const float *bias, float *out, int n, int H, int W) {
  const int C = 64, Hc = out_size(H, 2), Wc = out_size(W, 2), Hp = out_size(Hc, 2), Wp = out_size(Wc, 2);
  std::vector<float> conv((size_t)Hc * Wc * C);
  for (int img = 0; img < n; ++img) {
    const uint8_t *im = images + (size_t)img * H * W;
    for (int cy = 0; cy < Hc; ++cy)
      for (int cx = 0; cx < Wc; ++cx)
        for (int c = 0; c < C; ++c) {
          float acc = bias[c];
          for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx) {
              const int iy = 2 * cy + ky - 3, ix = 2 * cx + kx - 3;
              const float v = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? (float)im[(size_t)iy * W + ix] : 0.0f;
              acc = std::fmaf(w[(ky * 7 + kx) * C + c], v, acc);
            }
          conv[((size_t)cy * Wc + cx) * C + c] = relu(acc);
        }
    for (int py = 0; py < Hp; ++py)
      for (int px = 0; px < Wp; ++px)
        for (int c = 0; c < C; ++c) {
          float m = 0.0f;
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int cy = 2 * py + dy, cx = 2 * px + dx;
              if (cy < 0 || cy >= Hc || cx < 0 || cx >= Wc) continue;
              const float v = conv[((size_t)cy * Wc + cx) * C + c];
              if (v > m) m = v;
            }
          out[(((size_t)img * Hp + py) * Wp + px) * C + c] = m;
        }
  }
}

// in [n][Hi][Wi][Cin] -> out [n][Ho][Wo][Cout], ks x ks, padding ks / 2: an output element is one chain from its bias over
// the taps row-major and, inside a tap, over the groups of 32 input channels, a group in the order 0, 16, 1, 17, ..., 15,
// 31; a padding tap contributes fmaf(w, +0, acc).  Then one fp32 add of the residual (NULL: none), then the ReLU.
// The chains of a pixel's Cout channels run side by side (co innermost): each is still its own sequence.
void bb_host_conv(const float *in, const float *w, const float *bias, const float *resid, float *out, int n, int Hi, int Wi,
                  int Cin, int Ho, int Wo, int Cout, int ks, int stride, int relu_on) {
  const int pad = ks / 2;
  std::vector<float> acc(Cout);
  for (int img = 0; img < n; ++img)
    for (int oy = 0; oy < Ho; ++oy)
      for (int ox = 0; ox < Wo; ++ox) {
        for (int co = 0; co < Cout; ++co) acc[co] = bias[co];
        for (int ky = 0; ky < ks; ++ky)
          for (int kx = 0; kx < ks; ++kx) {
            const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
            const bool inside = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
            const float *xp = inside ? in + (((size_t)img * Hi + iy) * Wi + ix) * Cin : nullptr;
            const float *wt = w + (size_t)(ky * ks + kx) * Cin * Cout;
            for (int g = 0; g < Cin; g += 32)
              for (int i = 0; i < 16; ++i)
                for (int half = 0; half < 2; ++half) {
                  const int ci = g + i + 16 * half;
                  const float x = inside ? xp[ci] : 0.0f;
                  const float *wr = wt + (size_t)ci * Cout;
                  for (int co = 0; co < Cout; ++co) acc[co] = std::fmaf(wr[co], x, acc[co]);
                }
          }
        const size_t o = (((size_t)img * Ho + oy) * Wo + ox) * Cout;
        for (int co = 0; co < Cout; ++co) {
          float v = acc[co];
          if (resid) v = v + resid[o + co];
          out[o + co] = relu_on ? relu(v) : v;
        }
      }
}

// in [n][P][cin] -> out [n][cout]: a channel's sum over the pixels in ascending order with plain adds from 0, one
// division by P, then fc row j as one chain from its bias over k ascending (w [cout][cin])
void bb_host_pool_fc(const float *in, const float *w, const float *bias, float *out, int n, int P, int cin, int cout) {
  std::vector<float> mean(cin);
  for (int img = 0; img < n; ++img) {
    const float *x = in + (size_t)img * P * cin;
    for (int c = 0; c < cin; ++c) {
      float s = 0.0f;
      for (int p = 0; p < P; ++p) s = s + x[(size_t)p * cin + c];
      mean[c] = s / (float)P;
    }
    for (int j = 0; j < cout; ++j) {
      float acc = bias[j];
      for (int k = 0; k < cin; ++k) acc = std::fmaf(w[(size_t)j * cin + k], mean[k], acc);
      out[(size_t)img * cout + j] = acc;
    }
  }
}

}  // extern "C"
