// neo_record.hpp -- the fleet's `record` mode (include/neo_planner.h, neo_record_*): what traj_planner/record_planner.py
// saves of every successful plan -- the depth image, form_nn_input's 24-d motion vector (:13-58), form_nn_output's
// body-frame waypoints (:61-72) and the durations -- as one row of a RESIDENT dataset.
//
//   record_state_kernel    the vehicle's velocity now (drone_state.global_vel)         one lane per mission
//   record_rank_kernel     the dataset rows of the launched missions that solved        one workgroup
//   record_commit_kernel   one dataset row: motion, waypoints, tau, pose, meta, image   one workgroup per mission
//
// Included by neo_disp_record.hip and, for record_to_body and the sizes of a row, by neo_init.hpp, which defines
// NEO_RECORD_HELPERS_ONLY first: its unit then gets no copy of the kernels.  D = 2, fp64, every operation rounded on its
// own (contraction off): NumPy gives the same bits (tests/record_oracle_np.py).  No atomics: the row of a mission
// follows from its position in the launch and the counters alone.  Mission-indexed arrays are indexed by mission b; workgroup / lane k works on the mission at
// position k of the launch list (neo_launch_list.hpp).
#pragma once
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kRecordThreads = 256;     // state: missions per workgroup; commit: lanes of a mission's workgroup
constexpr int kRecordRankThreads = 1024;
constexpr int kRecordD = 2;
constexpr int kRecordRow = 3 * kRecordD;  // doubles of a command row / a head or tail state
constexpr int kRecordMotion = 24;         // form_nn_input's vector
constexpr int kRecordUnroll = 4;          // 16-byte pieces a lane has in flight in the image copy (written out below)

#ifndef NEO_RECORD_HELPERS_ONLY
// drone_state.global_vel at the time of the plan: the velocity of the command row being flown, or, before the first
// plan, of the plan's initial state (traj_planner_node.py first_plan: drone_state is plan_init_state).
__global__ __launch_bounds__(kRecordThreads) void record_state_kernel(
    LaunchList list, const double *__restrict__ cmd, int cap, const int *__restrict__ cmd_len,
    const int *__restrict__ cmd_index, const double *__restrict__ head, double *__restrict__ cur_vel) {
  const int b = list.request(blockIdx.x * kRecordThreads + threadIdx.x);
  if (b < 0) return;
  int len = cmd_len[b];
  len = len > cap ? cap : len;
  const double *v;
  if (len >= 1) {
    int k = cmd_index[b];
    k = k < 0 ? 0 : (k > len - 1 ? len - 1 : k);  // (the loop keeps 0 <= cmd_index < cmd_len: no row outside the array)
    v = cmd + ((size_t)b * cap + k) * kRecordRow + kRecordD;
  } else {
    v = head + (size_t)b * kRecordRow + kRecordD;
  }
  cur_vel[(size_t)b * 2] = v[0];
  cur_vel[(size_t)b * 2 + 1] = v[1];
}

// row_of[k], k < n: the dataset row of the mission at position k -- *n_rows + its rank among the launched missions
// with solved != 0 -- or -1: not solved, not a mission, or the row would lie at or beyond `capacity` (counted in
// *dropped).  ONE workgroup walks the positions in chunks of kRecordRankThreads with ordered_rank
// (neo_launch_list.hpp): rows follow the positions whatever the scheduling.  *n_rows advances by the rows given.
__global__ __launch_bounds__(kRecordRankThreads) void record_rank_kernel(
    LaunchList list, const int *__restrict__ solved, int capacity, int *__restrict__ row_of, int *__restrict__ n_rows,
    int *__restrict__ dropped) {
  __shared__ RankLds<kRecordRankThreads> ranks;
  __shared__ int first_s;
  const int tid = threadIdx.x, n = list.size();
  if (tid == 0) {
    const int at = *n_rows;
    first_s = at < 0 ? 0 : (at > capacity ? capacity : at);
    ranks.base = 0;
  }
  __syncthreads();
  const int first = first_s;
  const int room = capacity - first;  // >= 0
  for (int at = 0; at < n; at += kRecordRankThreads) {
    const int k = at + tid;
    const int b = list.request(k);
    const bool take = b >= 0 && (!solved || solved[b] != 0);
    const int rank = ordered_rank(take, ranks);
    if (k < n) row_of[k] = (take && rank < room) ? first + rank : -1;
  }
  if (tid == 0) {
    const int total = ranks.base, given = total < room ? total : room;
    *n_rows = first + given;
    *dropped += total - given;
  }
}

#endif  // NEO_RECORD_HELPERS_ONLY

// R^T v for R = [[c, -s, 0], [s, c, 0], [0, 0, 1]]: (c vx + s vy, -s vx + c vy, vz), every product rounded on its own
__device__ __forceinline__ void record_to_body(double c, double s, double vx, double vy, double vz, double *o) {
#pragma clang fp contract(off)
  const double a = c * vx, b = s * vy;
  const double e = (-s) * vx, f = c * vy;
  o[0] = a + b;
  o[1] = e + f;
  o[2] = vz;
}

struct RecordBytes16 {
  unsigned int w[4];
};

// nvec 16-byte pieces from src to the 16-byte aligned dst: whole rounds of kRecordUnroll pieces a lane, all their loads
// issued before the first store, then the rest one piece at a time
template <bool kAlignedSrc>
__device__ __forceinline__ RecordBytes16 record_load16(const unsigned char *__restrict__ src) {
  RecordBytes16 r;
  if (kAlignedSrc)
    r = *reinterpret_cast<const RecordBytes16 *>(__builtin_assume_aligned(src, 16));
  else
    __builtin_memcpy(&r, src, 16);
  return r;
}
__device__ __forceinline__ void record_store16(unsigned char *__restrict__ dst, const RecordBytes16 &r) {
  *reinterpret_cast<RecordBytes16 *>(__builtin_assume_aligned(dst, 16)) = r;
}

template <bool kAlignedSrc>
__device__ __forceinline__ void record_copy_middle(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst,
                                                   size_t nvec, int tid) {
  constexpr size_t kRound = (size_t)kRecordThreads * kRecordUnroll;
  const size_t whole = nvec - nvec % kRound;
  for (size_t v0 = 0; v0 < whole; v0 += kRound) {
    const size_t at = (v0 + tid) * 16;
    const RecordBytes16 r0 = record_load16<kAlignedSrc>(src + at);
    const RecordBytes16 r1 = record_load16<kAlignedSrc>(src + at + (size_t)kRecordThreads * 16);
    const RecordBytes16 r2 = record_load16<kAlignedSrc>(src + at + (size_t)kRecordThreads * 32);
    const RecordBytes16 r3 = record_load16<kAlignedSrc>(src + at + (size_t)kRecordThreads * 48);
    record_store16(dst + at, r0);
    record_store16(dst + at + (size_t)kRecordThreads * 16, r1);
    record_store16(dst + at + (size_t)kRecordThreads * 32, r2);
    record_store16(dst + at + (size_t)kRecordThreads * 48, r3);
  }
  for (size_t v = whole + tid; v < nvec; v += kRecordThreads) record_store16(dst + v * 16, record_load16<kAlignedSrc>(src + v * 16));
}

// n bytes from src to dst, any alignment of either: bytes up to dst's first 16-byte boundary, 16-byte stores over the
// aligned middle -- 16-byte loads too; where src sits differently inside its 16 bytes than dst they are unaligned loads,
// which global memory takes -- and bytes after it.  Every lane of the workgroup calls it with the same arguments.
__device__ __forceinline__ void record_copy_bytes(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst,
                                                  size_t n, int tid) {
  const size_t to_boundary = (size_t)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u);
  const size_t lead = to_boundary < n ? to_boundary : n;
  const size_t nvec = (n - lead) / 16;
  const size_t tail0 = lead + nvec * 16;
  if ((size_t)tid < lead) dst[tid] = src[tid];
  if ((((uintptr_t)(src + lead)) & 15u) == 0)
    record_copy_middle<true>(src + lead, dst + lead, nvec, tid);
  else
    record_copy_middle<false>(src + lead, dst + lead, nvec, tid);
  if (tail0 + (size_t)tid < n) dst[tail0 + tid] = src[tail0 + tid];  // fewer than 16 bytes
}

#ifndef NEO_RECORD_HELPERS_ONLY
struct RecordData {  // the dataset: `capacity` rows each
  double *motion;         // [capacity][24]
  double *wpts_local;     // [capacity][3 (M - 1)]
  double *tau;            // [capacity][M]
  double *pose;           // [capacity][5]
  int *meta;              // [capacity][3]: mission id, tick, target round
  unsigned char *images;  // [capacity][H][W]
};

__global__ __launch_bounds__(kRecordThreads) void record_commit_kernel(
    LaunchList list, const int *__restrict__ row_of, int capacity, int M, const double *__restrict__ x,
    const double *__restrict__ head, const double *__restrict__ tail, const double *__restrict__ pose,
    const double *__restrict__ cur_vel, const unsigned char *__restrict__ staging, size_t hw,
    const int *__restrict__ mission_ids, int tick, int round, RecordData d) {
#pragma clang fp contract(off)
  const int k = blockIdx.x;
  const int b = list.request(k);  // workgroup-uniform
  if (b < 0) return;
  const int row = row_of[k];
  if (row < 0 || row >= capacity) return;
  const int tid = threadIdx.x;
  const int nw = M - 1, nx = kRecordD * nw + M;
  const double *ps = pose + (size_t)b * 5;
  const double px = ps[0], py = ps[1], pz = ps[2], c = ps[3], s = ps[4];
  const double *xb = x + (size_t)b * nx;
  const double dz = pz - pz;  // (q, des_pos_z) - global_pos: the eye flies at des_pos_z
  for (int i = tid; i < nw; i += kRecordThreads)
    record_to_body(c, s, xb[i] - px, xb[nw + i] - py, dz, d.wpts_local + ((size_t)row * nw + i) * 3);
  for (int i = tid; i < M; i += kRecordThreads) d.tau[(size_t)row * M + i] = xb[kRecordD * nw + i];
  if (tid == kRecordThreads - 1) {
    const double vx = cur_vel[(size_t)b * 2], vy = cur_vel[(size_t)b * 2 + 1];
    const double *hd = head + (size_t)b * kRecordRow, *tl = tail + (size_t)b * kRecordRow;
    double *m = d.motion + (size_t)row * kRecordMotion;
    record_to_body(c, s, vx, vy, 0.0, m);  // drone_state.local_vel
    m[3] = c, m[4] = -s, m[5] = 0.0;       // attitude.rotation_matrix, row-major
    m[6] = s, m[7] = c, m[8] = 0.0;
    m[9] = 0.0, m[10] = 0.0, m[11] = 1.0;
    record_to_body(c, s, hd[0] - px, hd[1] - py, dz, m + 12);
    record_to_body(c, s, hd[2] - vx, hd[3] - vy, 0.0, m + 15);
    record_to_body(c, s, tl[0] - px, tl[1] - py, dz, m + 18);
    record_to_body(c, s, tl[2] - vx, tl[3] - vy, 0.0, m + 21);
    double *po = d.pose + (size_t)row * 5;
    po[0] = px, po[1] = py, po[2] = pz, po[3] = c, po[4] = s;
    int *mt = d.meta + (size_t)row * 3;
    mt[0] = mission_ids ? mission_ids[b] : b;
    mt[1] = tick;
    mt[2] = round;
  }
  record_copy_bytes(staging + (size_t)b * hw, d.images + (size_t)row * hw, hw, tid);
}
#endif  // NEO_RECORD_HELPERS_ONLY

}  // namespace neo
