// neo_launch_list.hpp -- what the kernels that run on RESIDENT arrays share (fleet, record, onboard, batch, plan,
// init and adaptive units): the list of a launch, the map table of a call, the six result arrays of an optimiser launch,
// and the one-workgroup ordered rank with the in-place compaction built on it.  Included by neo_host.hpp and by the seven kernel headers; it needs nothing but HIP and the cross-lane layer (neo_wave.hpp).
//
// A launch covers n positions.  Position p works on request (mission) subset[p], or on p when there is no subset.  An
// index outside 0 .. B - 1 is skipped: request() answers -1, the kernel returns, and every row of that index -- the
// request-indexed ones it has none of, the packed ones of position p -- stays as it is.  Request-indexed arrays have B
// rows; packed arrays are indexed by position.
#pragma once
#include <hip/hip_runtime.h>

#include "neo_wave.hpp"

namespace neo {

constexpr int kListWave = 64;  // lanes of a wavefront (gfx950)

struct LaunchList {
  const int *subset;  // device array of n request indices, or NULL: position p is request p
  int B;              // rows of the request-indexed arrays
  int n;              // positions launched
  __host__ __device__ int size() const { return n; }
  __device__ __forceinline__ int request(int p) const {  // -1: p >= n, or an index outside 0 .. B - 1
    if (p >= n) return -1;
    const int b = subset ? subset[p] : p;
    return (b >= 0 && b < B) ? b : -1;
  }
};
// the C ABI's (B, subset, n_subset): n_subset counts only with a subset
inline LaunchList launch_list(int B, const int *subset, int n_subset) { return {subset, B, subset ? n_subset : B}; }

// the map table (or the one map) of a call's kind
struct MapRef {
  const void *table;
  const int *slots;  // device array [B] of map-table slots, or NULL (every request uses table[0])
  int nmaps;         // entries of `table` (slots are checked against it on the device)
};

// the six result arrays of an optimiser launch: x [rows][n], costs4 and costs4_last [rows][4], the integers [rows]
struct RunRowsIn {
  const double *x, *costs4, *costs4_last;
  const int *nit, *nfev, *status;
};
struct RunRows {
  double *x, *costs4, *costs4_last;
  int *nit, *nfev, *status;  // nit, nfev: or NULL (not kept)
};

// row `row` of the packed results to row b of the request-indexed ones, by one wavefront: x strided over the lanes,
// the two cost rows by lanes 0 - 3, the integers by lane 0.  The request-indexed x has rows of `ldx` >= n doubles (the
// packed one rows of n); what lies behind the n values of a row is the caller's.
__device__ __forceinline__ void scatter_run_row(int lane, int n, int ldx, const RunRowsIn &packed, size_t row,
                                                const RunRows &out, int b) {
  for (int i = lane; i < n; i += kListWave) out.x[(size_t)b * ldx + i] = packed.x[row * n + i];
  if (lane < 4) {
    out.costs4[(size_t)b * 4 + lane] = packed.costs4[row * 4 + lane];
    out.costs4_last[(size_t)b * 4 + lane] = packed.costs4_last[row * 4 + lane];
  }
  if (lane == 0) {
    out.status[b] = packed.status[row];
    if (out.nit) out.nit[b] = packed.nit[row];
    if (out.nfev) out.nfev[b] = packed.nfev[row];
  }
}

// the boundary of packed row `row` from request b's: head, tail (3 x D doubles each) and, when kept, the map slot
template <int D>
__device__ __forceinline__ void pack_boundary(const double *__restrict__ head, const double *__restrict__ tail,
                                              const int *__restrict__ slots, int b, double *__restrict__ head_k,
                                              double *__restrict__ tail_k, int *__restrict__ slots_k, size_t row) {
  const double *hd = head + (size_t)b * 3 * D, *tl = tail + (size_t)b * 3 * D;
  double *hk = head_k + row * 3 * D, *tk = tail_k + row * 3 * D;
#pragma unroll
  for (int q = 0; q < 3 * D; ++q) {
    hk[q] = hd[q];
    tk[q] = tl[q];
  }
  if (slots_k) slots_k[row] = slots ? slots[b] : 0;
}

// The ordered rank of ONE workgroup of THREADS lanes that walks an array in chunks of THREADS positions: ordered_rank
// answers how many lanes before this one, in this chunk and in every chunk before it, came with `take` set, and
// advances the base by the chunk's takers.  A ballot, per-wavefront counts in LDS, a running base, three barriers a
// call: ranks follow the positions whatever the scheduling.  The workgroup zeroes `base` (and meets a barrier) before
// its first call, every lane makes every call, and `base` is the number of takers after the last.  Whatever a lane
// read of its chunk before the call has been read by every lane when the call returns: a chunk can be written in place.
template <int THREADS>
struct RankLds {
  int wave_cnt[THREADS / kListWave];
  int base;
};
template <int THREADS>
__device__ __forceinline__ int ordered_rank(bool take, RankLds<THREADS> &s) {
  constexpr int kWaves = THREADS / kListWave;
  const int tid = threadIdx.x, lane = tid & (kListWave - 1), wv = tid / kListWave;
  const unsigned long long m = __ballot(take);
  if (lane == 0) s.wave_cnt[wv] = __popcll(m);
  __syncthreads();  // every read of this chunk is done, the counts are visible
  int rank = s.base;
  for (int q = 0; q < wv; ++q) rank += s.wave_cnt[q];
  rank += __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int q = 0; q < kWaves; ++q) total += s.wave_cnt[q];
    s.base += total;
  }
  __syncthreads();
  return rank;
}

// seg[len] (a request index, or -1) -> its entries >= 0 packed to the front in the order of their positions, by ONE
// workgroup of THREADS lanes; returns their number (to every lane).  A chunk is read whole, then written at or before
// the places it was read from, so the packing is done in place and no position depends on scheduling.  `len` is
// workgroup-uniform; every lane of the workgroup makes the call.
template <int THREADS>
__device__ __forceinline__ int compact_in_place(int *__restrict__ seg, int len) {
  __shared__ RankLds<THREADS> ranks;
  const int tid = threadIdx.x;
  if (tid == 0) ranks.base = 0;
  __syncthreads();
  for (int at = 0; at < len; at += THREADS) {
    const int i = at + tid;
    const int v = i < len ? seg[i] : -1;        // the chunk is read whole ...
    const int rank = ordered_rank(v >= 0, ranks);
    if (v >= 0) seg[rank] = v;                  // ... before any of it is written: rank <= i
  }
  return ranks.base;
}

}  // namespace neo
