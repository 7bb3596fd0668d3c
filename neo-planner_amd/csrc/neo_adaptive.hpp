// neo_adaptive.hpp -- adaptive waypoint counts (generate_init_variables with init_wpts_mode 'adaptive',
// traj_planner/expert_planner.py:86-88) for a batch on RESIDENT arrays (include/neo_planner.h, neo_adaptive_*): every
// request its own count, the launch list grouped by count, and what BatchPlanner.plan's retry chain needs to run over
// the groups without a host wait per group.
//
//   adaptive_count_kernel     max(ceil(L / init_seg_len - 1), 1), clamped                one lane per request
//   adaptive_bucket_kernel    the launch list as a stable counting sort by count         ONE workgroup
//   adaptive_compact_kernel   batch_compact_kernel (neo_batch.hpp) per group's segment    one workgroup per group
// A group's merge is the plan unit's plan_merge_kernel, with the row length of the longest group for x.
//
// Included by neo_disp_adaptive.hip only.  fp64, D = 2 or 3.  Request-indexed arrays are indexed by request b; packed
// arrays by the request's position p in the launch list (neo_launch_list.hpp).  No atomics, no scratch.
#pragma once
#include "neo_wave.hpp"
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kAdaptiveThreads = 256;   // count: requests per workgroup; compact: lanes of a group's workgroup
constexpr int kBucketThreads = 1024;    // bucket: the one workgroup
constexpr int kBucketWaves = kBucketThreads / kWave;
constexpr int kBuckets = NEO_MAX_PIECES;  // counts 0 .. 63 (a count is at least 1: group 0 stays empty)

// The count is BatchPlanner.adaptive_counts', operation by operation (every one rounded on its own, nothing fused):
//   d_k = target_k - start_k;  s = d_0 * d_0 + d_1 * d_1 (+ d_2 * d_2) from left to right;  L = sqrt(s)
//   c = ceil(L / seg_len - 1.0);  count = max(c, 1) -- 1 when L is not finite (the optimiser reports such a request)
//   count > max_w: count = max_w, clamped = 1
// compared as doubles: L / seg_len may be anything up to +inf.
template <int D>
__global__ __launch_bounds__(kAdaptiveThreads) void adaptive_count_kernel(LaunchList list, const double *__restrict__ head,
                                                                          const double *__restrict__ tail, double seg_len,
                                                                          int max_w, int *__restrict__ counts,
                                                                          int *__restrict__ clamped) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * kAdaptiveThreads + threadIdx.x;
  const int b = list.request(p);
  if (b < 0) return;
  const double *hd = head + (size_t)b * 3 * D, *tl = tail + (size_t)b * 3 * D;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double d = tl[k] - hd[k];
    const double sq = d * d;
    s = k == 0 ? sq : s + sq;
  }
  const double L = sqrt(s);
  int count = 1, cl = 0;
  if (L - L == 0.0) {  // finite
    const double ratio = L / seg_len;
    const double c = ceil(ratio - 1.0);
    if (c > (double)max_w) {
      count = max_w;
      cl = 1;
    } else if (c > 1.0) {
      count = (int)c;
    }
  }
  counts[b] = count;
  clamped[b] = cl;
}

// The lanes of the wavefront that hold the same key as this one (keys 0 .. 63; a lane with key < 0 gets 0): six
// ballots, one per bit of the key, and one for the valid lanes.
__device__ __forceinline__ unsigned long long same_key_lanes(int key) {
  unsigned long long m = __ballot(key >= 0);
#pragma unroll
  for (int bit = 0; bit < 6; ++bit) {
    const bool set = (key >> bit) & 1;
    const unsigned long long bal = __ballot(set);
    m &= set ? bal : ~bal;
  }
  return key >= 0 ? m : 0ull;
}

// order = the launch list's valid requests by ascending counts[b], in list order within a count; bucket_begin[c] the
// first place of count c, bucket_begin[kBuckets] = *total the requests kept.  A stable counting sort by ONE workgroup:
// wavefront w owns the contiguous positions [w * span, (w + 1) * span) and row w of the LDS table.
//   1. histogram: per chunk of 64 positions the lowest lane of every key adds the key's lanes to table[w][key] -- one
//      wavefront a row, one lane a cell: no atomics;
//   2. the first wavefront (lane = key) scans the 64 column totals and turns every cell into the place of the row's
//      first request of that key: bucket_begin[key] + the cells of the rows above;
//   3. placement: the same walk; a lane's place is table[w][key] + the lanes below it with its key, then the key's
//      lowest lane moves the cell on.  A wavefront's LDS operations execute in issue order (lds_wave_sync keeps the
//      compiler to it), so the walk needs no barrier; the kernel has three.
// Places follow from the positions alone, whatever the scheduling.  A request whose count is outside 0 .. kBuckets - 1
// is dropped like a skipped index.
__global__ __launch_bounds__(kBucketThreads) void adaptive_bucket_kernel(LaunchList list, const int *__restrict__ counts,
                                                                         int *__restrict__ order,
                                                                         int *__restrict__ bucket_begin,
                                                                         int *__restrict__ total) {
  __shared__ int table[kBucketWaves][kBuckets];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int P = list.size();
  const int chunks = (P + kWave - 1) / kWave;                         // of 64 positions
  const int span = (chunks + kBucketWaves - 1) / kBucketWaves * kWave;  // positions a wavefront owns
  const int first = wv * span;
  const int last = min(first + span, P);                              // (first >= P: the wavefront owns nothing)
  const unsigned long long below = (1ull << lane) - 1ull;
  table[wv][lane] = 0;
  __syncthreads();
  for (int at = first; at < last; at += kWave) {  // wave-uniform bounds
    const int b = list.request(at + lane);
    int key = b >= 0 ? counts[b] : -1;
    if (key >= kBuckets) key = -1;
    const unsigned long long same = same_key_lanes(key);
    if (key >= 0 && (same & below) == 0) table[wv][key] += __popcll(same);
    lds_wave_sync();  // (the next chunk's lowest lane of a key may be another one)
  }
  __syncthreads();
  if (wv == 0) {
    int sum = 0;
    for (int q = 0; q < kBucketWaves; ++q) sum += table[q][lane];
    const int incl = wave_scan_add(sum);
    int place = incl - sum;
    bucket_begin[lane] = place;
    if (lane == kWave - 1) {
      bucket_begin[kBuckets] = incl;
      *total = incl;
    }
    for (int q = 0; q < kBucketWaves; ++q) {
      const int cell = table[q][lane];
      table[q][lane] = place;
      place += cell;
    }
  }
  __syncthreads();
  for (int at = first; at < last; at += kWave) {
    const int b = list.request(at + lane);
    int key = b >= 0 ? counts[b] : -1;
    if (key >= kBuckets) key = -1;
    const unsigned long long same = same_key_lanes(key);
    int place = 0;
    if (key >= 0) place = table[wv][key] + __popcll(same & below);
    lds_wave_sync();  // every lane has read its cell ...
    if (key >= 0) {
      order[place] = b;
      if ((same & below) == 0) table[wv][key] += __popcll(same);  // ... before the key's lowest lane moves it on
    }
    lds_wave_sync();
  }
}

// the groups' segments of `pending`, by value: group c owns pending[begin[c] .. begin[c] + len[c] - 1]
struct AdaptiveSegs {
  int begin[kBuckets];
  int len[kBuckets];
};

// batch_compact_kernel (neo_batch.hpp) per segment: workgroup c packs the entries >= 0 of its group's segment to the
// segment's front in the order of their positions (compact_in_place, neo_launch_list.hpp) and writes their number to
// n_failed[c] (0 for an empty segment).
__global__ __launch_bounds__(kAdaptiveThreads) void adaptive_compact_kernel(AdaptiveSegs segs, int *__restrict__ pending,
                                                                            int *__restrict__ n_failed) {
  const int c = blockIdx.x;
  const int kept = compact_in_place<kAdaptiveThreads>(pending + segs.begin[c], segs.len[c]);  // workgroup-uniform
  if (threadIdx.x == 0) n_failed[c] = kept;
}

}  // namespace neo
