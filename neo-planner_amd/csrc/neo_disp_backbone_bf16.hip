// neo_disp_backbone_bf16.hip -- the image backbone on bf16 storage and the bf16 matrix cores (neo_backbone_bf16.hpp): the
// packed blob from the fp32 one, and ResNet18OneChannel in eval mode from n uint8 depth images to n x 24 fp32 features, 21
// launches on the context's stream.  Every pointer is a device array; the arguments were checked by the C ABI.
#include "neo_host.hpp"
#include "neo_backbone_bf16.hpp"

namespace neo {

namespace {

constexpr int kBhChannels[4] = {64, 128, 256, 512};

// bf16 values of one activation buffer: the largest layer output of n images of H x W, rounded up to 256 bytes
size_t bh_buffer_elems(int n, int H, int W) {
  int h = bh_out_size(bh_out_size(H, 2), 2), w = bh_out_size(bh_out_size(W, 2), 2);   // after the stem and the pool
  size_t most = 0;
  for (int l = 0; l < 4; ++l) {
    if (l) h = bh_out_size(h, 2), w = bh_out_size(w, 2);
    most = std::max(most, (size_t)n * h * w * kBhChannels[l]);
  }
  return (most + 127) & ~size_t(127);
}

struct BhConv {
  const __bf16 *w;
  const float *b;
};

// the next convolution of the packed blob: W [ks][ks][cin / 8][cout][8] bf16, then b [cout] fp32
BhConv bh_take(const unsigned char *&p, int ks, int cin, int cout) {
  BhConv c{reinterpret_cast<const __bf16 *>(p), reinterpret_cast<const float *>(p + (size_t)ks * ks * cin * cout * 2)};
  p = reinterpret_cast<const unsigned char *>(c.b + cout);
  return c;
}

void bh_conv(neo_ctx *c, const BhConv &cv, int ks, const __bf16 *in, const __bf16 *resid, __bf16 *out, float *dbg, int n,
             int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int stride, int relu) {
  const int ncols = n * Ho * Wo;
  int cs_shift = 0;
  while ((kBhStepK << cs_shift) < Cin) ++cs_shift;
  const dim3 grid((ncols + kBhTileCols - 1) / kBhTileCols, Cout / kBhTileCo);
  if (ks == 3)
    hipLaunchKernelGGL(bb_conv_bf16_kernel<3>, grid, dim3(kBhThreads), 0, c->stream, in, cv.w, cv.b, resid, out, dbg, ncols, Hi,
                       Wi, Cin, cs_shift, Ho, Wo, Cout, stride, relu);
  else
    hipLaunchKernelGGL(bb_conv_bf16_kernel<1>, grid, dim3(kBhThreads), 0, c->stream, in, cv.w, cv.b, resid, out, dbg, ncols, Hi,
                       Wi, Cin, cs_shift, Ho, Wo, Cout, stride, relu);
}

}  // namespace

size_t backbone_bf16_workspace_bytes(int n, int H, int W) { return 3 * bh_buffer_elems(n, H, W) * 2; }

int backbone_bf16_pack(neo_ctx *c, const float *weights, void *packed) {
  const float *src = weights;
  unsigned char *dst = static_cast<unsigned char *>(packed);
  auto copy = [&](size_t floats) {
    const hipError_t e = hipMemcpyAsync(dst, src, floats * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    src += floats, dst += floats * sizeof(float);
    return e;
  };
  auto conv = [&](int ks, int cin, int cout) {
    const size_t runs = (size_t)ks * ks * (cin / 8) * cout;
    hipLaunchKernelGGL(bb_pack_bf16_kernel, dim3((unsigned)((runs + kBhThreads - 1) / kBhThreads)), dim3(kBhThreads), 0,
                       c->stream, src, reinterpret_cast<__bf16 *>(dst), ks * ks, cin, cout);
    src += runs * 8, dst += runs * 16;
    return copy(cout);
  };
  HIPCHK(c, copy(49 * kBhStemC + kBhStemC));
  int cin = kBhStemC;
  for (int l = 0; l < 4; ++l) {
    const int cout = kBhChannels[l];
    for (int blk = 0; blk < 2; ++blk) {
      HIPCHK(c, conv(3, cin, cout));
      HIPCHK(c, conv(3, cout, cout));
      if (cin != cout) HIPCHK(c, conv(1, cin, cout));
      cin = cout;
    }
  }
  HIPCHK(c, copy((size_t)kBhFcIn * kBhFcOut + kBhFcOut));
  return NEO_OK;
}

int backbone_bf16_features(neo_ctx *c, const void *packed, const unsigned char *images, int n, int H, int W, void *workspace,
                           float *feature_out, hipEvent_t *events, int last, const void **written, float *dbg_last) {
  int launches = 0;
  // (neo_backbone_bf16_launch_times: an event in front of the chain and one behind every launch)
  hipError_t mark_err = hipSuccess;
  auto mark = [&]() {
    if (!events) return;
    const hipError_t e = hipEventRecord(events[launches++], c->stream);
    if (mark_err == hipSuccess) mark_err = e;
  };
  // behind every launch: its event; true when the chain ends here (`out`: the buffer the launch wrote)
  int ran = 0;
  auto ends = [&](const void *out) {
    mark();
    if (written) *written = out;
    return ran++ == last;
  };
  // the debug array of the launch about to run: the chain's last launch alone writes it
  auto dbg = [&]() { return ran == last ? dbg_last : nullptr; };
  auto result = [&]() {
    if (mark_err != hipSuccess)
      return fail(c, NEO_ERR_HIP, std::string("backbone bf16: hipEventRecord: ") + hipGetErrorString(mark_err));
    return (int)NEO_OK;
  };
  mark();
  const size_t buf = bh_buffer_elems(n, H, W);
  __bf16 *x = static_cast<__bf16 *>(workspace), *t = x + buf, *y = t + buf;   // block input, conv1's output, the spare
  const unsigned char *p = static_cast<const unsigned char *>(packed);
  const int Hc = bh_out_size(H, 2), Wc = bh_out_size(W, 2);
  int h = bh_out_size(Hc, 2), w = bh_out_size(Wc, 2);
  {
    const float *sw = reinterpret_cast<const float *>(p), *sb = sw + 49 * kBhStemC;
    p = reinterpret_cast<const unsigned char *>(sb + kBhStemC);
    const int tx = (w + kBhPoolW - 1) / kBhPoolW, ty = (h + kBhPoolH - 1) / kBhPoolH;
    hipLaunchKernelGGL(bb_stem_bf16_kernel, dim3((unsigned)((size_t)n * tx * ty)), dim3(kBhThreads), 0, c->stream, images, sw, sb,
                       x, dbg(), H, W, Hc, Wc, h, w, tx, ty);
    if (ends(x)) return result();
  }
  int cin = kBhStemC;
  for (int l = 0; l < 4; ++l) {
    const int cout = kBhChannels[l];
    for (int blk = 0; blk < 2; ++blk) {
      const int stride = (l > 0 && blk == 0) ? 2 : 1;
      const int ho = bh_out_size(h, stride), wo = bh_out_size(w, stride);
      const BhConv c1 = bh_take(p, 3, cin, cout), c2 = bh_take(p, 3, cout, cout);
      bh_conv(c, c1, 3, x, nullptr, t, dbg(), n, h, w, cin, ho, wo, cout, stride, 1);
      if (ends(t)) return result();
      if (stride != 1 || cin != cout) {
        // the identity goes through the 1 x 1 stride-2 branch into the spare buffer, which conv2 then finishes in place
        const BhConv ds = bh_take(p, 1, cin, cout);
        bh_conv(c, ds, 1, x, nullptr, y, dbg(), n, h, w, cin, ho, wo, cout, stride, 0);
        std::swap(x, y);
        if (ends(x)) return result();
      }
      bh_conv(c, c2, 3, t, x, x, dbg(), n, ho, wo, cout, ho, wo, cout, 1, 1);
      if (ends(x)) return result();
      h = ho, w = wo, cin = cout;
    }
  }
  const float *fw = reinterpret_cast<const float *>(p);
  hipLaunchKernelGGL(bb_pool_fc_bf16_kernel, dim3(n), dim3(kBhThreads), 0, c->stream, x, fw, fw + (size_t)kBhFcIn * kBhFcOut,
                     feature_out, h * w);
  ends(feature_out);
  return result();
}

}  // namespace neo
