// neo_disp_backbone.hip -- the image backbone of the learned warm start (neo_backbone.hpp): ResNet18OneChannel in eval mode
// from n uint8 depth images to n x 24 features, 21 launches on the context's stream.  Every pointer is a device array; the
// arguments were checked by the C ABI.
#include "neo_host.hpp"
#include "neo_backbone.hpp"

namespace neo {

namespace {

constexpr int kBbChannels[4] = {64, 128, 256, 512};

// floats of one activation buffer: the largest layer output of n images of H x W, rounded up to 256 bytes
size_t bb_buffer_floats(int n, int H, int W) {
  int h = bb_out_size(bb_out_size(H, 2), 2), w = bb_out_size(bb_out_size(W, 2), 2);   // after the stem and the pool
  size_t most = 0;
  for (int l = 0; l < 4; ++l) {
    if (l) h = bb_out_size(h, 2), w = bb_out_size(w, 2);
    most = std::max(most, (size_t)n * h * w * kBbChannels[l]);
  }
  return (most + 63) & ~size_t(63);
}

struct BbConv {
  const float *w, *b;
};

// the next convolution of the blob: W [ks][ks][cin][cout], then b [cout]
BbConv bb_take(const float *&p, int ks, int cin, int cout) {
  BbConv c{p, p + (size_t)ks * ks * cin * cout};
  p = c.b + cout;
  return c;
}

void bb_conv(neo_ctx *c, const BbConv &cv, int ks, const float *in, const float *resid, float *out, int n, int Hi, int Wi,
             int Cin, int Ho, int Wo, int Cout, int stride, int relu) {
  const int ncols = n * Ho * Wo;
  int cg_shift = 0;
  while ((32 << cg_shift) < Cin) ++cg_shift;
  const dim3 grid((ncols + kBbTileCols - 1) / kBbTileCols, Cout / kBbTileCo);
  if (ks == 3)
    hipLaunchKernelGGL(bb_conv_kernel<3>, grid, dim3(kBbThreads), 0, c->stream, in, cv.w, cv.b, resid, out, ncols, Hi, Wi, Cin,
                       cg_shift, Ho, Wo, Cout, stride, relu);
  else
    hipLaunchKernelGGL(bb_conv_kernel<1>, grid, dim3(kBbThreads), 0, c->stream, in, cv.w, cv.b, resid, out, ncols, Hi, Wi, Cin,
                       cg_shift, Ho, Wo, Cout, stride, relu);
}

}  // namespace

size_t backbone_workspace_bytes(int n, int H, int W) { return 3 * bb_buffer_floats(n, H, W) * sizeof(float); }

void backbone_activation_shape(int launch, int H, int W, int *h, int *w, int *c) {
  // launches: the stem; layer 1 (conv1, conv2 twice): 1 .. 4; layers 2 .. 4 (conv1, downsample, conv2, conv1, conv2): five each
  // from 5; the pool + fc
  if (launch == NEO_BACKBONE_LAUNCHES - 1) {
    *h = *w = 1, *c = kBbFcOut;
    return;
  }
  const int layer = launch < 5 ? 0 : (launch - 5) / 5 + 1;
  *h = bb_out_size(bb_out_size(H, 2), 2), *w = bb_out_size(bb_out_size(W, 2), 2);
  for (int l = 0; l < layer; ++l) *h = bb_out_size(*h, 2), *w = bb_out_size(*w, 2);
  *c = kBbChannels[layer];
}

int backbone_features(neo_ctx *c, const float *weights, const unsigned char *images, int n, int H, int W, void *workspace,
                      float *feature_out, hipEvent_t *events, int last, const float **written) {
  int launches = 0;
  // (neo_backbone_launch_times: an event in front of the chain and one behind every launch)
  hipError_t mark_err = hipSuccess;
  auto mark = [&]() {
    if (!events) return;
    const hipError_t e = hipEventRecord(events[launches++], c->stream);
    if (mark_err == hipSuccess) mark_err = e;
  };
  // behind every launch: its event; true when the chain ends here (`out`: the buffer the launch wrote)
  int ran = 0;
  auto ends = [&](const float *out) {
    mark();
    if (written) *written = out;
    return ran++ == last;
  };
  auto result = [&]() {
    if (mark_err != hipSuccess) return fail(c, NEO_ERR_HIP, std::string("backbone: hipEventRecord: ") + hipGetErrorString(mark_err));
    return (int)NEO_OK;
  };
  mark();
  const size_t buf = bb_buffer_floats(n, H, W);
  float *x = static_cast<float *>(workspace), *t = x + buf, *y = t + buf;   // block input, conv1's output, the spare
  const float *p = weights;
  const int Hc = bb_out_size(H, 2), Wc = bb_out_size(W, 2);
  int h = bb_out_size(Hc, 2), w = bb_out_size(Wc, 2);
  {
    const BbConv stem = bb_take(p, 7, 1, kBbStemC);
    const int tx = (w + kBbPoolW - 1) / kBbPoolW, ty = (h + kBbPoolH - 1) / kBbPoolH;
    hipLaunchKernelGGL(bb_stem_kernel, dim3((unsigned)((size_t)n * tx * ty)), dim3(kBbThreads), 0, c->stream, images, stem.w,
                       stem.b, x, H, W, Hc, Wc, h, w, tx, ty);
    if (ends(x)) return result();
  }
  int cin = kBbStemC;
  for (int l = 0; l < 4; ++l) {
    const int cout = kBbChannels[l];
    for (int blk = 0; blk < 2; ++blk) {
      const int stride = (l > 0 && blk == 0) ? 2 : 1;
      const int ho = bb_out_size(h, stride), wo = bb_out_size(w, stride);
      const BbConv c1 = bb_take(p, 3, cin, cout), c2 = bb_take(p, 3, cout, cout);
      bb_conv(c, c1, 3, x, nullptr, t, n, h, w, cin, ho, wo, cout, stride, 1);
      if (ends(t)) return result();
      if (stride != 1 || cin != cout) {
        // the identity goes through the 1 x 1 stride-2 branch into the spare buffer, which conv2 then finishes in place
        const BbConv ds = bb_take(p, 1, cin, cout);
        bb_conv(c, ds, 1, x, nullptr, y, n, h, w, cin, ho, wo, cout, stride, 0);
        std::swap(x, y);
        if (ends(x)) return result();
      }
      bb_conv(c, c2, 3, t, x, x, n, ho, wo, cout, ho, wo, cout, 1, 1);
      if (ends(x)) return result();
      h = ho, w = wo, cin = cout;
    }
  }
  hipLaunchKernelGGL(bb_pool_fc_kernel, dim3(n), dim3(kBbThreads), 0, c->stream, x, p, p + (size_t)kBbFcIn * kBbFcOut,
                     feature_out, h * w);
  ends(feature_out);
  return result();
}

}  // namespace neo
