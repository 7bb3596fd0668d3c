// neo_init.hpp -- the learned warm start on RESIDENT arrays (include/neo_planner.h, neo_init_*): what
// traj_planner/neo_planner.py does between the depth image's features and the optimiser -- form_nn_input's motion
// vector (record_planner.py:13-58), PlannerNet's dense layers (nn_trainer.py:123-155) and the network's output as the
// optimiser's first guess (nn_planner.py:104-134, map_T2tau) -- for the requests of a launch list.
//
//   init_motion_kernel   the 24 values record_commit_kernel writes into a row's motion, as fp32    one lane per request
//   init_head_kernel     PlannerNet.head: motion branch, concatenation, fusion MLP, all fp32        256 lanes per 32 requests
//   init_guess_kernel    the 9 outputs to x0 = [x_0, x_1, y_0, y_1, tau_0, tau_1, tau_2]             one lane per request
//
// Included by neo_disp_init.hip only.  Every product, sum and difference is rounded on its own (contraction off), in the
// order written here: NumPy gives the same bits (tests/init_oracle_np.py), the device's fp64 log apart.  Request-indexed
// arrays throughout; lane / workgroup position p works on request list.request(p) (neo_launch_list.hpp).
#pragma once
#include "neo_launch_list.hpp"
#define NEO_RECORD_HELPERS_ONLY  // record_to_body and the kRecord* sizes, not the recorder's kernels
#include "neo_record.hpp"

namespace neo {

constexpr int kInitThreads = 256;  // motion, guess: requests per workgroup; head: lanes of a tile's workgroup
constexpr int kInitTile = 32;      // head: requests per workgroup
constexpr int kInitRows = kInitThreads / kInitTile;  // head: output neurons computed at a time
constexpr int kInitMaxWidth = 96;  // widest layer
constexpr int kInitOut = NEO_INIT_OUTPUT;
// the largest layer's W and b, and two activation buffers [neuron][request] of a tile
constexpr int kInitWeightLds = kInitMaxWidth * kInitMaxWidth + kInitMaxWidth;
constexpr int kInitActLds = kInitMaxWidth * kInitTile;
static_assert((kInitWeightLds + 2 * kInitActLds) * sizeof(float) <= 64 * 1024, "the head kernel's static LDS");
static_assert(kRecordMotion == NEO_INIT_MOTION, "the motion vector is the recorder's");

__global__ __launch_bounds__(kInitThreads) void init_motion_kernel(
    LaunchList list, const double *__restrict__ pose, const double *__restrict__ cur_vel, const double *__restrict__ head,
    const double *__restrict__ tail, float *__restrict__ motion) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x * kInitThreads + threadIdx.x);
  if (b < 0) return;
  const double *ps = pose + (size_t)b * 5;
  const double px = ps[0], py = ps[1], pz = ps[2], c = ps[3], s = ps[4];
  const double vx = cur_vel[(size_t)b * 2], vy = cur_vel[(size_t)b * 2 + 1];
  const double *hd = head + (size_t)b * kRecordRow, *tl = tail + (size_t)b * kRecordRow;
  const double dz = pz - pz;  // as record_commit_kernel: NaN for a non-finite eye height
  double m[kRecordMotion];
  record_to_body(c, s, vx, vy, 0.0, m);
  m[3] = c, m[4] = -s, m[5] = 0.0;
  m[6] = s, m[7] = c, m[8] = 0.0;
  m[9] = 0.0, m[10] = 0.0, m[11] = 1.0;
  record_to_body(c, s, hd[0] - px, hd[1] - py, dz, m + 12);
  record_to_body(c, s, hd[2] - vx, hd[3] - vy, 0.0, m + 15);
  record_to_body(c, s, tl[0] - px, tl[1] - py, dz, m + 18);
  record_to_body(c, s, tl[2] - vx, tl[3] - vy, 0.0, m + 21);
  float *o = motion + (size_t)b * kRecordMotion;
#pragma unroll
  for (int i = 0; i < kRecordMotion; ++i) o[i] = (float)m[i];
}

__device__ __forceinline__ float init_leaky(float v) {
#pragma clang fp contract(off)
  return v > 0.0f ? v : 0.01f * v;
}

// One Linear layer of a tile: W [OUT][IN] then b [OUT] from `w` (global) through `wl` (LDS); the tile's activations
// in[k][r] -> out[j][r] (LDS, [neuron][request]).  Lane = (output neuron tid / 32 + 8 m, request tid % 32): the 32 lanes
// of a neuron read one weight (a broadcast) and 32 consecutive activations.  acc = b[j]; k ascending: p = W[j][k] a[k];
// acc = acc + p.  Ends with a barrier: `out` is complete and `wl` free.  Every lane of the workgroup calls it.
template <int IN, int OUT, bool LEAKY>
__device__ __forceinline__ void init_layer(const float *__restrict__ w, float *__restrict__ wl, const float *__restrict__ in,
                                           float *__restrict__ out, int tid) {
#pragma clang fp contract(off)
  static_assert(IN <= kInitMaxWidth && OUT <= kInitMaxWidth, "layer wider than the LDS buffers");
  constexpr int kFloats = OUT * IN + OUT;
  for (int i = tid; i < kFloats; i += kInitThreads) wl[i] = w[i];
  __syncthreads();  // the weights are staged, and `in` (the layer before, or the inputs) is complete
  const int r = tid % kInitTile;
  for (int j = tid / kInitTile; j < OUT; j += kInitRows) {
    const float *wj = wl + j * IN;
    float acc = wl[OUT * IN + j];
#pragma unroll 8
    for (int k = 0; k < IN; ++k) {
      const float p = wj[k] * in[k * kInitTile + r];
      acc = acc + p;
    }
    out[j * kInitTile + r] = LEAKY ? init_leaky(acc) : acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kInitThreads) void init_head_kernel(
    LaunchList list, const float *__restrict__ weights, const float *__restrict__ feature, int feature_rows,
    const float *__restrict__ motion, float *__restrict__ out) {
  __shared__ float wl[kInitWeightLds];
  __shared__ float act[2][kInitActLds];
  const int tid = threadIdx.x;
  float *A = act[0], *B = act[1];
  // the tile's inputs: motion into A rows 0 .. 23; the image features wait in B rows 48 .. 71, which no layer of the
  // motion branch touches (its widest output is 48 rows)
  constexpr int kFeatureAt = 48;
  for (int i = tid; i < kInitTile * NEO_INIT_MOTION; i += kInitThreads) {
    const int r = i / NEO_INIT_MOTION, k = i % NEO_INIT_MOTION;
    const int b = list.request(blockIdx.x * kInitTile + r);
    A[k * kInitTile + r] = b >= 0 ? motion[(size_t)b * NEO_INIT_MOTION + k] : 0.0f;
    B[(kFeatureAt + k) * kInitTile + r] = b >= 0 ? feature[(feature_rows == 1 ? (size_t)0 : (size_t)b) * NEO_INIT_FEATURE + k] : 0.0f;
  }
  const float *w = weights;
  init_layer<24, 48, true>(w, wl, A, B, tid);
  w += 24 * 48 + 48;
  init_layer<48, 24, true>(w, wl, B, A, tid);
  w += 48 * 24 + 24;
  init_layer<24, 24, true>(w, wl, A, B, tid);
  w += 24 * 24 + 24;
  init_layer<24, 24, false>(w, wl, B, A + NEO_INIT_FEATURE * kInitTile, tid);  // [feature, motion_feature]: rows 24 .. 47
  w += 24 * 24 + 24;
  for (int i = tid; i < kInitTile * NEO_INIT_FEATURE; i += kInitThreads) A[i] = B[kFeatureAt * kInitTile + i];
  // (the next layer's first barrier comes before its first read of A)
  init_layer<48, 48, true>(w, wl, A, B, tid);
  w += 48 * 48 + 48;
  init_layer<48, 96, true>(w, wl, B, A, tid);
  w += 48 * 96 + 96;
  init_layer<96, 96, true>(w, wl, A, B, tid);
  w += 96 * 96 + 96;
  init_layer<96, kInitOut, false>(w, wl, B, A, tid);
  for (int i = tid; i < kInitTile * kInitOut; i += kInitThreads) {
    const int r = i / kInitOut, j = i % kInitOut;
    const int b = list.request(blockIdx.x * kInitTile + r);
    if (b >= 0) out[(size_t)b * kInitOut + j] = A[j * kInitTile + r];
  }
}

__global__ __launch_bounds__(kInitThreads) void init_guess_kernel(
    LaunchList list, const float *__restrict__ out, const double *__restrict__ pose, double T_min, double T_max,
    double *__restrict__ x0) {
#pragma clang fp contract(off)
  const int b = list.request(blockIdx.x * kInitThreads + threadIdx.x);
  if (b < 0) return;
  const double *ps = pose + (size_t)b * 5;
  const double px = ps[0], py = ps[1], c = ps[3], s = ps[4];
  const float *o = out + (size_t)b * kInitOut;
  double *x = x0 + (size_t)b * NEO_INIT_X;
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // the body-frame z is dropped (nn_planner.py:104-134)
    const double lx = (double)o[3 * i], ly = (double)o[3 * i + 1];
    const double a = c * lx, e = s * ly;
    const double f = s * lx, g = c * ly;
    x[i] = (a - e) + px;
    x[2 + i] = (f + g) + py;
  }
  const double span = T_max - T_min;
  const double eps = 1e-3 * span;
  const double lo = T_min + eps, hi = T_max - eps;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double t = (double)o[6 + j];
    t = t < lo ? lo : (t > hi ? hi : t);  // a NaN passes, as in np.clip
    const double q = span / (t - T_min);
    x[4 + j] = -log(q - 1.0);  // map_T2tau
  }
}

}  // namespace neo
