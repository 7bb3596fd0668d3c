// neo_abi.hip -- C ABI of libneo_planner_hip.so (include/neo_planner.h): argument checks, locking, scratch layout
// (Carver, HostStage) and host copies, the map bookkeeping, and one call into the kernel family's unit (neo_disp_*.hip)
// per entry point.  The kernels it still holds are the small ones around the optimiser's results:
//
//   traj_state_kernel   get_full_state_cmd                      (traj_utils.py:85-195)
//   pack_results_kernel, effort_keys_kernel and the rocPRIM sort of the dispatch order
//
// The map kernels are in neo_esdf.hpp (launched from neo_disp_esdf.hip); the fused kernels (eval / optimize / sample)
// are templates in neo_kernels.hpp, instantiated per family in the neo_disp_*.hip translation units.
#include <cstring>
#include "neo_host.hpp"
#include <rocprim/device/device_radix_sort.hpp>
#include "neo_kernels.hpp"

namespace neo {

// get_full_state_cmd (traj_utils.py:85-195): one wavefront per trajectory solves the
// coefficients, then its lanes walk the sample times.
template <int D>
__global__ __launch_bounds__(kWave) void traj_state_kernel(int B, int M, DevParams prm,
                                                            const double *__restrict__ x,
                                                            const double *__restrict__ head,
                                                            const double *__restrict__ tail, double hz, int K,
                                                            double *__restrict__ state, int *__restrict__ count) {
  __shared__ double xs[kSlots * kWave];
  __shared__ double cs[kWave * 6 * D];
  __shared__ double tcum[kWave + 1];
  const int b = blockIdx.x;
  if (b >= B) return;
  struct NoMap {};
  struct NoLookup {
    __device__ explicit NoLookup(const NoMap &) {}
  };
  DevParams p = prm;
  NoMap nm;
  DevBackend<D, kSlots, double, NoMap, NoLookup> be(p, nm);
  be.xs = xs;
  be.hist = nullptr;
  be.m = NEO_LBFGS_M;
  be.coeff_out = nullptr;
  load_boundary(be.t, head + (size_t)b * 3 * D, tail + (size_t)b * 3 * D, M);
  const int n = be.t.n;
  const int lane = lane_id();
  typename DevBackend<D, kSlots, double, NoMap, NoLookup>::Vec xv;
#pragma unroll
  for (int k = 0; k < kSlots; ++k) xv.v[k] = (k * kWave + lane < n) ? x[(size_t)b * n + k * kWave + lane] : 0.0;
  be.scatter_x(xv);
  double e, ts;
  const int st = minco_forward<D>(be.t, p, e, ts);
  if (st != 0) {
    if (lane == 0) count[b] = -1;
    return;
  }
  if (lane < M) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int d = 0; d < D; ++d) cs[(lane * 6 + k) * D + d] = be.t.c[k][d];
  }
  // sequential prefix sums like Python's sum(ts[:k]) (traj_utils.py:98-101)
  if (lane == 0) tcum[0] = 0.0;
  for (int pce = 0; pce < M; ++pce) {
    const double Tp = rdlane(be.t.T, pce);
    if (lane == 0) tcum[pce + 1] = tcum[pce] + Tp;
  }
  __syncthreads();
  const double total = tcum[M];
  const double step = 1.0 / hz;
  const int cnt = (int)ceil(total / step);  // len(np.arange(0, total, 1/hz))
  if (lane == 0) count[b] = cnt;
  for (int k = lane; k < K; k += kWave) {
    double *out = state + ((size_t)b * K + k) * 3 * D;
    if (k >= cnt) {
#pragma unroll
      for (int q = 0; q < 3 * D; ++q) out[q] = 0.0;
      continue;
    }
    double tt = (double)k * step;
    if (tt > total) tt = total;
    int pc = 0;
    while (pc < M - 1 && tcum[pc + 1] < tt) ++pc;
    const double T = tt - tcum[pc];
    const double T2 = T * T, T3 = T2 * T, T4 = T2 * T2, T5 = T4 * T;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double c0 = cs[(pc * 6 + 0) * D + d], c1 = cs[(pc * 6 + 1) * D + d], c2 = cs[(pc * 6 + 2) * D + d];
      const double c3 = cs[(pc * 6 + 3) * D + d], c4 = cs[(pc * 6 + 4) * D + d], c5 = cs[(pc * 6 + 5) * D + d];
      out[0 * D + d] = c0 + c1 * T + c2 * T2 + c3 * T3 + c4 * T4 + c5 * T5;
      out[1 * D + d] = c1 + 2.0 * c2 * T + 3.0 * c3 * T2 + 4.0 * c4 * T3 + 5.0 * c5 * T4;
      out[2 * D + d] = 2.0 * c2 + 6.0 * c3 * T + 12.0 * c4 * T2 + 20.0 * c5 * T3;
    }
  }
}

}  // namespace neo

// =================================================================== host side
using namespace neo;

namespace {

void fill_dev_params(neo_ctx *c) {
  const neo_params &p = c->params;
  DevParams &d = c->dev;
  d.v_max = p.v_max;
  d.T_min = p.T_min;
  d.T_max = p.T_max;
  d.safe_dis = p.safe_dis;
  d.delta_t = p.delta_t;
  for (int k = 0; k < 4; ++k) d.w[k] = p.weights[k];
  d.coll_tol = p.collision_cost_tol;
  d.ftol = p.ftol;
  d.gtol = p.gtol;
  d.maxls = p.maxls;
  d.maxiter = p.maxiter;
  d.maxfun = p.maxfun;
  d.stale_T = p.bugcompat_stale_T;
  d.dbg = p.flags;
  d.derive();
}

int ensure_scratch(neo_ctx *c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return NEO_OK;
  if (c->scratch) hipFree(c->scratch);
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  HIPCHK(c, hipMalloc(&c->scratch, bytes));
  c->scratch_bytes = bytes;
  return NEO_OK;
}

int ensure_pinned(neo_ctx *c, size_t bytes) {
  if (bytes <= c->pinned_bytes) return NEO_OK;
  if (c->pinned) hipHostFree(c->pinned);
  c->pinned = nullptr;
  c->pinned_bytes = 0;
  HIPCHK(c, hipHostMalloc(&c->pinned, bytes, hipHostMallocDefault));
  c->pinned_bytes = bytes;
  return NEO_OK;
}

// bump allocator over the scratch buffer (device-only work buffers of the ESDF upload / build paths)
struct Carver {
  char *base;
  size_t off = 0;
  explicit Carver(void *b) : base(static_cast<char *>(b)) {}
  template <typename T>
  T *take(size_t count) {
    off = (off + 255) & ~size_t(255);
    T *p = reinterpret_cast<T *>(base + off);
    off += count * sizeof(T);
    return p;
  }
};

// Calls whose whole scratch layout is at most this many bytes go through the pinned mirror: ONE copy in and ONE copy out
// instead of one per array from pageable memory (a single plan() of the reference's shape: 0.36 -> 0.27 ms; ten such
// copies cost almost as much as the kernel).  Small calls only: from a megabyte on, the extra pass over the data costs
// more than the copies' latencies -- 8192 replans of the reference's shape per call: 1.46 M/s direct, 1.28 M/s staged.
// (neo_optimize_batch, neo_cost_grad_batch, neo_eval_traj_batch; the other host forms pass 0 = never: the mirror has
// not been measured there.)
constexpr size_t kStagedUpTo = (size_t)256 * 1024;

// The arrays of one host-pointer call, staged through c->scratch.  Declare the fields in layout order -- in(), then
// inout(), then out(), each 256-byte aligned -- then upload(), run the `_dev` form on dev() pointers, then download().
// A null host pointer reserves the field and copies nothing for it (device-only, or the caller did not ask).  The
// scratch is sized from the declarations.  Calls up to `staged_up_to` bytes move the contiguous input range and the
// contiguous output range through the pinned mirror of the same layout, whole, null fields included; larger ones copy
// field by field.  A stage that goes out of scope between upload() and a completed download() (an error return) waits
// for the stream first: copies in flight read the caller's arrays and the wrapper's locals.
// The context stays locked for the stage's lifetime (c->scratch and c->pinned are the context's only ones).
class HostStage {
 public:
  template <typename T>
  struct Ref { int i; };

  HostStage(neo_ctx *c, size_t staged_up_to) : c_(c), staged_up_to_(staged_up_to) { f_.reserve(12); }
  HostStage(const HostStage &) = delete;
  HostStage &operator=(const HostStage &) = delete;
  ~HostStage() {
    if (in_flight_) hipStreamSynchronize(c_->stream);
  }

  // `count` elements are copied; `reserve` (>= count) sizes the field when the device side wants more room
  template <typename T>
  Ref<T> in(const T *host, size_t count, size_t reserve = 0) { return {add(0, host, nullptr, count * sizeof(T), reserve * sizeof(T))}; }
  template <typename T>
  Ref<T> inout(T *host, size_t count) { return {add(1, host, host, count * sizeof(T), 0)}; }
  template <typename T>
  Ref<T> out(T *host, size_t count, size_t reserve = 0) { return {add(2, nullptr, host, count * sizeof(T), reserve * sizeof(T))}; }

  // an array the caller may leave out (a subset, slots, ...): staged like in() / inout() when it is given; dev() of
  // the field is NULL when it is not, which is what the `_dev` form takes for "none"
  template <typename T>
  Ref<T> in_optional(const T *host, size_t count) { return {add(0, host, nullptr, host ? count * sizeof(T) : 0, sizeof(T), !host)}; }
  template <typename T>
  Ref<T> inout_optional(T *host, size_t count) { return {add(1, host, host, host ? count * sizeof(T) : 0, 0, !host)}; }

  // the field's device array: valid from upload() on (growing the scratch moves it), NULL before
  template <typename T>
  T *dev(Ref<T> r) const { return dbase_ && !f_[r.i].absent ? reinterpret_cast<T *>(dbase_ + f_[r.i].off) : nullptr; }

  int upload() {
    if (!ordered_) return fail(c_, NEO_ERR_INVALID, "internal: staged fields declared out of order");
    staged_ = staged_up_to_ && end_ <= staged_up_to_;
    int rc = ensure_scratch(c_, end_ + 256);
    if (!rc && staged_) rc = ensure_pinned(c_, end_ + 256);
    if (rc) return rc;
    dbase_ = static_cast<char *>(c_->scratch);
    hbase_ = static_cast<char *>(c_->pinned);
    in_flight_ = true;
    if (staged_) {
      for (const Field &f : f_)
        if (f.src) std::memcpy(hbase_ + f.off, f.src, f.bytes);
      HIPCHK(c_, hipMemcpyAsync(dbase_, hbase_, std::min(in_end_, end_), hipMemcpyHostToDevice, c_->stream));
      return NEO_OK;
    }
    for (const Field &f : f_)
      if (f.src) HIPCHK(c_, hipMemcpyAsync(dbase_ + f.off, f.src, f.bytes, hipMemcpyHostToDevice, c_->stream));
    return NEO_OK;
  }

  int download() {
    if (staged_) {
      const size_t o = std::min(out_begin_, end_);
      HIPCHK(c_, hipMemcpyAsync(hbase_ + o, dbase_ + o, end_ - o, hipMemcpyDeviceToHost, c_->stream));
    } else {
      for (const Field &f : f_)
        if (f.dst) HIPCHK(c_, hipMemcpyAsync(f.dst, dbase_ + f.off, f.bytes, hipMemcpyDeviceToHost, c_->stream));
    }
    HIPCHK(c_, hipStreamSynchronize(c_->stream));
    in_flight_ = false;
    if (staged_)
      for (const Field &f : f_)
        if (f.dst) std::memcpy(f.dst, hbase_ + f.off, f.bytes);
    return NEO_OK;
  }

 private:
  struct Field {
    size_t off, bytes;
    const void *src;  // host array copied up, or NULL
    void *dst;        // host array copied back, or NULL
    bool absent;      // an optional field the caller left out
  };
  int add(int role, const void *src, void *dst, size_t bytes, size_t reserve, bool absent = false) {
    ordered_ = ordered_ && role >= role_;
    role_ = role;
    const size_t off = (end_ + 255) & ~size_t(255);
    if (role >= 1) out_begin_ = std::min(out_begin_, off);
    if (role == 2) in_end_ = std::min(in_end_, off);
    end_ = off + std::max(bytes, reserve);
    f_.push_back({off, bytes, src, dst, absent});
    return (int)f_.size() - 1;
  }
  neo_ctx *c_;
  size_t staged_up_to_;
  std::vector<Field> f_;
  size_t end_ = 0;                  // bytes of the layout (the last field's end)
  size_t in_end_ = ~size_t(0);      // the input range is [0, first out() field)
  size_t out_begin_ = ~size_t(0);   // the output range is [first inout() / out() field, end)
  int role_ = 0;
  bool ordered_ = true, staged_ = false, in_flight_ = false;
  char *dbase_ = nullptr, *hbase_ = nullptr;
};

int rebuild_tables(neo_ctx *c) {
  if (!c->table_dirty) return NEO_OK;
  std::vector<Map2D> t2;
  std::vector<Map3D> t3;
  for (auto &kv : c->maps) {
    MapEntry &e = kv.second;
    if (e.kind == 0) {
      e.slot = (int)t2.size();
      t2.push_back(e.m2);
    } else if (e.kind == 1) {
      e.slot = (int)t3.size();
      t3.push_back(e.m3);
    }
  }
  if (c->table2d) hipFree(c->table2d);
  if (c->table3d) hipFree(c->table3d);
  c->table2d = c->table3d = nullptr;
  if (!t2.empty()) {
    HIPCHK(c, hipMalloc(&c->table2d, t2.size() * sizeof(Map2D)));
    HIPCHK(c, hipMemcpyAsync(c->table2d, t2.data(), t2.size() * sizeof(Map2D), hipMemcpyHostToDevice, c->stream));
  }
  if (!t3.empty()) {
    HIPCHK(c, hipMalloc(&c->table3d, t3.size() * sizeof(Map3D)));
    HIPCHK(c, hipMemcpyAsync(c->table3d, t3.data(), t3.size() * sizeof(Map3D), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->n2d = (int)t2.size();
  c->n3d = (int)t3.size();
  c->table_dirty = false;
  return NEO_OK;
}

// (callers do not hold the context lock yet: take it for the error string)
int check_shape(neo_ctx *c, int B, int M, int D) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (B < 0 || M < 1 || M > NEO_MAX_PIECES || D < 2 || D > NEO_MAX_DIM)
    return fail(c, NEO_ERR_INVALID, "shape out of range (1 <= M <= 64, D in {2,3})");
  if (D * (M - 1) + M > kSlots * kWave) return fail(c, NEO_ERR_INVALID, "n = D(M-1)+M exceeds 256");
  return NEO_OK;
}

// host scene ids of a multi-scene call -> map-table slots (context locked).  The maps must all be of one kind, or, for
// the geo warm start (`geo`: the reference's A* is 2-D only), all 2-D.
int scene_slots(neo_ctx *c, const int32_t *scene_ids, size_t B, bool geo, std::vector<int> &slots) {
  int rc = rebuild_tables(c);
  if (rc) return rc;
  slots.resize(B);
  int kind0 = geo ? 0 : -1;
  for (size_t i = 0; i < B; ++i) {
    auto it = c->maps.find(scene_ids[i]);
    if (it == c->maps.end())
      return fail(c, NEO_ERR_NO_MAP, geo ? "geo: no ESDF for one of scene_ids" : "no ESDF for one of scene_ids");
    if (kind0 < 0) kind0 = it->second.kind;
    if (it->second.kind != kind0)
      return geo ? fail(c, NEO_ERR_UNSUPPORTED, "geo: one of scene_ids is a 3-D map")
                 : fail(c, NEO_ERR_INVALID, "scene_ids mix 2-D and 3-D maps");
    slots[i] = it->second.slot;
  }
  return NEO_OK;
}

// From this batch size on the kernels take the two-wavefronts-per-SIMD register allocation (three in the all-fp32
// mode, always).  Measured in round 3, one launch at a time, two waves against one: fp64 mode +4 % at 1024, +9 % at 2048,
// +23 % at 3072 trajectories; mixed mode +2 %, +5 %, +23 % (round 2 had found one wave faster up to 2048: 9.1 against
// 10.1 ms -- before the per-evaluation loads and the spills of the two-waves kernels were gone).
constexpr int kTwoWavesFromBatch = 1024;
bool two_waves_wanted(const neo_ctx *c, int B) {
  const int fl = c->params.flags;
  return (B >= kTwoWavesFromBatch && !(fl & NEO_FLAG_ONE_WAVE_PER_SIMD)) || (fl & NEO_FLAG_TWO_WAVES_PER_SIMD);
}

int fail_locked(neo_ctx *c, int code, const char *msg) {
  std::lock_guard<std::recursive_mutex> g(c->mu);
  return fail(c, code, msg);
}

// the end of a `_dev` entry point: the launcher's return code, then the launch's own error
int launched(neo_ctx *c, int rc) {
  if (rc) return rc;
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

// the (B, subset, n_subset) of the entry points that take a launch list (context unlocked): B_min <= B, B <= B_max
// where there is a bound (a power of two), at most B entries
int list_check(neo_ctx *c, const char *who, int B, int B_min, int B_max, const int32_t *subset, int n_subset) {
  if (!c) return NEO_ERR_INVALID;
  if (B < B_min || B > B_max) {
    std::string msg = std::string(who) + ": B must be ";
    if (B_max == INT32_MAX) {
      msg += ">= " + std::to_string(B_min);
    } else {
      int k = 0;
      while ((1 << k) < B_max) ++k;
      msg += "in " + std::to_string(B_min) + " .. 2^" + std::to_string(k);
    }
    return fail_locked(c, NEO_ERR_INVALID, msg.c_str());
  }
  if (subset && (n_subset < 0 || n_subset > B))
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": bad subset size").c_str());
  return NEO_OK;
}

// the six result arrays of an optimiser launch through a stage: the packed rows go up, the request-indexed ones go up
// and come back (rows outside the launch stay); an array the caller left out stays out
struct RowRefs {
  HostStage::Ref<double> x, costs4, costs4_last;
  HostStage::Ref<int32_t> nit, nfev, status;
};
RowRefs stage_rows_in(HostStage &st, const RunRowsIn &r, size_t rows, size_t n) {
  return {st.in(r.x, rows * n), st.in(r.costs4, rows * 4), st.in(r.costs4_last, rows * 4), st.in(r.nit, rows),
          st.in_optional(r.nfev, rows), st.in(r.status, rows)};
}
RowRefs stage_rows_inout(HostStage &st, const RunRows &r, size_t rows, size_t n) {
  return {st.inout(r.x, rows * n), st.inout(r.costs4, rows * 4), st.inout(r.costs4_last, rows * 4),
          st.inout_optional(r.nit, rows), st.inout_optional(r.nfev, rows), st.inout(r.status, rows)};
}
RunRows staged_rows(const HostStage &st, const RowRefs &f) {
  return {st.dev(f.x), st.dev(f.costs4), st.dev(f.costs4_last), st.dev(f.nit), st.dev(f.nfev), st.dev(f.status)};
}
RunRowsIn as_const(const RunRows &r) { return {r.x, r.costs4, r.costs4_last, r.nit, r.nfev, r.status}; }

// dispatch_opt sends this launch to the lane-group kernel (several small trajectories per wavefront, opt-in):
// on the reference's own map small planar problems (M = 3 -> n = 7), on 3-D fields small problems in fp32 sampling
bool lane_group_launch(const neo_ctx *c, int kind, int layout, int D, const OptArgs &a) {
  if (!(c->params.flags & NEO_FLAG_LANE_GROUPS) || a.slots || a.M > 16 || D * (a.M - 1) + a.M > 32) return false;
  if (kind == 0) return D == 2;
  return D == 3 && c->params.sample_dtype == NEO_F32 &&
         (layout == NEO_LAYOUT_LINEAR || layout == NEO_LAYOUT_YZ4 || layout == NEO_LAYOUT_BRICK);
}

int dispatch_opt(neo_ctx *c, int kind, int elem, int layout, int D, const OptArgs &a) {
  const bool f32 = c->params.sample_dtype == NEO_F32;
  if (kind == 0) {
    if (lane_group_launch(c, kind, layout, D, a)) return launch_opt_groups_2d(c, f32, a);
    const int fl2 = c->params.flags;
    // all-fp32 mode on the reference's own map: the timed arithmetic, pinned to the reference's fixtures there
    if ((fl2 & NEO_FLAG_F32_SOLVE) && f32) return launch_opt_2d_x(c, D, a);
    if (D == 2 && slots_for(a.M, D) <= 2 && two_waves_wanted(c, a.B)) return launch_opt_2d_w2(c, f32, a);
    return launch_opt_2d(c, D, f32, a);
  }
  if (D != 3) return fail(c, NEO_ERR_INVALID, "a 3-D map needs D = 3");
  const int fl = c->params.flags;
  if (lane_group_launch(c, kind, layout, D, a)) return launch_opt_groups(c, elem, layout, a);
  if ((fl & NEO_FLAG_F32_SOLVE) && f32) return launch_opt_3d_x(c, elem, layout, a);  // all-fp32 mode
  // two trajectories per SIMD for calls that queue for the SIMDs anyway (3-D fields, fp32 sampling; beyond n = 128 with
  // the pairs stored in fp32 so that eight wavefronts still fit a CU's LDS, neo_kernels.hpp pairs_in_f32)
  if (f32 && slots_for(a.M, D) <= NEO_W2_MAX_SLOTS && two_waves_wanted(c, a.B)) return launch_opt_3d_w2(c, elem, layout, a);
  // fp64 sampling (the parity mode): two wavefronts per SIMD for n <= 128 when the batch queues for the SIMDs (the
  // unit is compiled so that these kernels spill 0 - 13 registers, build.py; cfg2 360 k -> 637 k traj/s, M = 25 239 k
  // -> 400 k, M = 32 162 k -> 241 k; four FLAT slots would spill 112)
  if (!f32 && slots_for(a.M, D) <= 2 && two_waves_wanted(c, a.B)) return launch_opt_3d_f64_w2(c, elem, layout, a);
  return f32 ? launch_opt_3d_f32(c, elem, layout, a) : launch_opt_3d_f64(c, elem, layout, a);
}

void drain_profile(neo_ctx *c) {
  for (int k = 0; k < NEO_KERNEL_COUNT; ++k) {
    for (auto &pr : c->prof[k].pending) {
      float ms = 0.f;
      hipEventSynchronize(pr.second);
      hipEventElapsedTime(&ms, pr.first, pr.second);
      c->prof[k].ms += ms;
      c->prof[k].launches += 1;
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
    c->prof[k].pending.clear();
  }
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int neo_abi_version(void) { return NEO_ABI_VERSION; }

int neo_params_default(neo_params *p) {
  if (!p) return NEO_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  // launch/config/planner_config.yaml:2-13
  p->v_max = 1.0;
  p->T_min = 0.5;
  p->T_max = 5.0;
  p->safe_dis = 0.7;
  p->delta_t = 0.1;
  p->weights[0] = 1.0;
  p->weights[1] = 1.0;
  p->weights[2] = 1.0;
  p->weights[3] = 10000.0;
  p->collision_cost_tol = 5.0;
  // expert_planner.py:213-225
  p->ftol = 1e-4;
  p->gtol = 1e-4;
  p->maxls = 20;
  p->maxiter = 15000;
  p->maxfun = 15000;
  p->bugcompat_stale_T = 1;
  p->sample_dtype = NEO_F64;
  return NEO_OK;
}

int neo_ctx_create(int device_id, void *stream, neo_ctx **out) {
  if (!out) return NEO_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NEO_ERR_HIP;
  if (device_id < 0 || device_id >= count) return NEO_ERR_INVALID;
  if (hipSetDevice(device_id) != hipSuccess) return NEO_ERR_HIP;
  neo_ctx *c = new neo_ctx();
  c->device = device_id;
  if (stream) {
    c->stream = static_cast<hipStream_t>(stream);
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return NEO_ERR_HIP;
    }
    c->own_stream = true;
  }
  c->home_stream = c->stream;
  neo_params_default(&c->params);
  fill_dev_params(c);
  *out = c;
  return NEO_OK;
}

int neo_ctx_set_stream(neo_ctx *c, void *stream) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->stream = stream ? static_cast<hipStream_t>(stream) : c->home_stream;
  return NEO_OK;
}

int neo_ctx_destroy(neo_ctx *c) {
  if (!c) return NEO_ERR_INVALID;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  if (c->stream != c->home_stream) hipStreamSynchronize(c->home_stream);
  drain_profile(c);
  geo_release(c);
  depth_release(c);
  for (auto &kv : c->maps)
    if (kv.second.data) hipFree(kv.second.data);
  if (c->order_buf) hipFree(c->order_buf);
  if (c->sample_order) hipFree(c->sample_order);
  if (c->tickets) hipFree(c->tickets);
  if (c->table2d) hipFree(c->table2d);
  if (c->table3d) hipFree(c->table3d);
  if (c->scratch) hipFree(c->scratch);
  if (c->pinned) hipHostFree(c->pinned);
  if (c->own_stream) hipStreamDestroy(c->home_stream);
  delete c;
  return NEO_OK;
}

const char *neo_last_error(neo_ctx *c) { return c ? c->err.c_str() : "null context"; }

int neo_params_set(neo_ctx *c, const neo_params *p) {
  if (!c || !p) return NEO_ERR_INVALID;
  if (!(p->T_max > p->T_min) || !(p->delta_t > 0.0) || p->maxls < 1)
    return fail(c, NEO_ERR_INVALID, "bad parameters");
  if (p->sample_dtype != NEO_F64 && p->sample_dtype != NEO_F32)
    return fail(c, NEO_ERR_INVALID, "sample_dtype must be NEO_F64 or NEO_F32");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->params = *p;
  fill_dev_params(c);
  return NEO_OK;
}

int neo_ctx_synchronize(neo_ctx *c) {
  if (!c) return NEO_ERR_INVALID;
  hipStream_t st;
  {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    st = c->stream;
  }
  const hipError_t e = hipStreamSynchronize(st);  // (not under the lock: other threads may keep launching)
  if (e != hipSuccess) return fail_locked(c, NEO_ERR_HIP, hipGetErrorString(e));
  return NEO_OK;
}

// Map updates wait for ALL device work first (hipDeviceSynchronize), not only for the context's current stream:
// `_dev` launches of neo_ctx_set_stream callers may still be reading the scene's buffer on other streams.
static int drop_locked(neo_ctx *c, int scene_id) {
  auto it = c->maps.find(scene_id);
  if (it != c->maps.end()) {
    hipDeviceSynchronize();
    if (it->second.data) hipFree(it->second.data);
    c->maps.erase(it);
    geo_forget(c, scene_id);
    c->table_dirty = true;
  }
  return NEO_OK;
}

int neo_esdf_drop(neo_ctx *c, int scene_id) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return drop_locked(c, scene_id);
}

// the scene's map is the 2-D one whose records `rec` holds: the entry takes the buffer over
static void adopt_map_2d(neo_ctx *c, int scene_id, DevBuf &rec, int W, int H, double res, double ox, double oy) {
  MapEntry e;
  e.kind = 0;
  e.elem = NEO_F64;
  e.data = rec.release();
  e.m2 = Map2D{static_cast<const double4 *>(e.data), W, H, res, ox, oy};
  e.version = ++c->map_serial;
  c->maps[scene_id] = e;
  c->table_dirty = true;
}

int neo_esdf_upload_2d(neo_ctx *c, int scene_id, const double *dist, const double *gx, const double *gy, int W,
                       int H, double res, double ox, double oy) {
  if (!c || !dist || !gx || !gy || W < 1 || H < 1 || !(res > 0.0)) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  drop_locked(c, scene_id);
  const size_t ncell = (size_t)W * H;
  int rc = ensure_scratch(c, 3 * ncell * sizeof(double) + 1024);
  if (rc) return rc;
  Carver cv(c->scratch);
  double *d0 = cv.take<double>(ncell), *d1 = cv.take<double>(ncell), *d2 = cv.take<double>(ncell);
  DevBuf rec;
  HIPCHK(c, rec.alloc(ncell * sizeof(double4)));
  HIPCHK(c, hipMemcpyAsync(d0, dist, ncell * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d1, gx, ncell * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d2, gy, ncell * sizeof(double), hipMemcpyHostToDevice, c->stream));
  esdf_pack_2d(c, d0, d1, d2, ncell, rec.as<double4>());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  adopt_map_2d(c, scene_id, rec, W, H, res, ox, oy);
  return NEO_OK;
}

// the device work of neo_esdf_build_2d into `rec`; scratch carved by the caller
static int build_2d_into(neo_ctx *c, double4 *rec, const int8_t *occ, int W, int H, double res, double *out_dist,
                         double *out_gx, double *out_gy) {
  const size_t ncell = (size_t)W * H;
  Carver cv(c->scratch);
  int8_t *d_occ = cv.take<int8_t>(ncell);
  int *d_g = cv.take<int>(ncell);
  int *d_v = cv.take<int>(ncell);
  double *d_z = cv.take<double>((size_t)H * (W + 1));
  double *d_dist = cv.take<double>(ncell);
  double *d_gx = cv.take<double>(ncell);
  double *d_gy = cv.take<double>(ncell);
  HIPCHK(c, hipMemcpyAsync(d_occ, occ, ncell, hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, NEO_KERNEL_ESDF_BUILD);
    esdf_build_2d(c, {d_occ, d_g, d_v, d_z, d_dist, d_gx, d_gy}, W, H, res, rec);
  }
  HIPCHK(c, hipGetLastError());
  if (out_dist) HIPCHK(c, hipMemcpyAsync(out_dist, d_dist, ncell * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (out_gx) HIPCHK(c, hipMemcpyAsync(out_gx, d_gx, ncell * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (out_gy) HIPCHK(c, hipMemcpyAsync(out_gy, d_gy, ncell * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NEO_OK;
}

int neo_esdf_build_2d(neo_ctx *c, int scene_id, const int8_t *occ, int W, int H, double res, double ox, double oy,
                      double *out_dist, double *out_gx, double *out_gy) {
  if (!c || !occ || W < 1 || H < 1 || !(res > 0.0)) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t ncell = (size_t)W * H;
  const size_t need = ncell * (sizeof(int8_t) + 2 * sizeof(int) + 3 * sizeof(double)) +
                      (size_t)H * (W + 1) * sizeof(double) + 4096;
  int rc = ensure_scratch(c, need);
  if (rc) return rc;
  // a map update of the same size rewrites the scene's record buffer in place (no hipFree / hipMalloc per
  // update), once nothing on the device can still be reading it
  auto it = c->maps.find(scene_id);
  const bool reuse = it != c->maps.end() && it->second.kind == 0 && it->second.data &&
                     (size_t)it->second.m2.W * it->second.m2.H == ncell;
  if (reuse) {
    HIPCHK(c, hipDeviceSynchronize());
    rc = build_2d_into(c, static_cast<double4 *>(it->second.data), occ, W, H, res, out_dist, out_gx, out_gy);
    if (rc) {
      drop_locked(c, scene_id);  // the buffer may be half rewritten: the scene has no map any more
      return rc;
    }
    const Map2D m{static_cast<const double4 *>(it->second.data), W, H, res, ox, oy};
    if (memcmp(&m, &it->second.m2, sizeof(m)) != 0) c->table_dirty = true;  // same buffer: usually the same descriptor
    it->second.m2 = m;
    it->second.version = ++c->map_serial;  // new contents: the geo mask is stale
    return NEO_OK;
  }
  drop_locked(c, scene_id);
  DevBuf rec;
  HIPCHK(c, rec.alloc(ncell * sizeof(double4)));
  rc = build_2d_into(c, rec.as<double4>(), occ, W, H, res, out_dist, out_gx, out_gy);
  if (rc) return rc;
  adopt_map_2d(c, scene_id, rec, W, H, res, ox, oy);
  return NEO_OK;
}

// Scratch of neo_esdf_build_2d_batch_dev, carved once for a pass of `chunk` maps: per map g (4 bytes a cell) and dist
// (8), beyond 512 x 512 also the sweeps' v (4) and z (8 (W + 1) H); plus the chunk's record pointers.  A pass takes as
// many maps as fit kBatchBuildScratch (and grid.y / grid.z): 12 bytes a cell -- 1.08 MB for 300 x 300, 993 maps a pass.
static const size_t kBatchBuildScratch = (size_t)1 << 30;
static size_t batch_build_bytes_per_map(int W, int H, bool sweeps) {
  const size_t ncell = (size_t)W * H;
  size_t per = ncell * (sizeof(int) + sizeof(double)) + 512;
  if (sweeps) per += ncell * sizeof(int) + (size_t)H * (W + 1) * sizeof(double) + 512;
  return per;
}

int neo_esdf_build_2d_batch_dev(neo_ctx *c, const int32_t *scene_ids, int n, const int8_t *occ, int W, int H, double res,
                                const double *origins) {
  if (!c) return NEO_ERR_INVALID;
  if (n < 0 || W < 1 || H < 1 || !(res > 0.0) || !std::isfinite(res))
    return fail_locked(c, NEO_ERR_INVALID, "batch build: n >= 0, width and height >= 1, resolution finite and > 0");
  if (n == 0) return NEO_OK;
  if (!scene_ids || !occ || !origins) return fail_locked(c, NEO_ERR_INVALID, "batch build: null buffer");
  if ((size_t)W * H > (size_t)1 << 28) return fail_locked(c, NEO_ERR_INVALID, "batch build: more than 2^28 cells a map");
  {
    std::vector<int32_t> ids(scene_ids, scene_ids + n);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end())
      return fail_locked(c, NEO_ERR_INVALID, "batch build: a scene id is listed twice");
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t ncell = (size_t)W * H;
  const bool sweeps = W > 512 || H > 512;
  const size_t per = batch_build_bytes_per_map(W, H, sweeps);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, kBatchBuildScratch / per, (size_t)65535}));
  int rc = ensure_scratch(c, (size_t)chunk * (per + sizeof(void *)) + 4096);
  if (rc) return rc;
  // the record buffer of every scene: its own where it already holds a 2-D map of this size (rewritten in place, the
  // descriptor -- and with it the map table and every slot -- usually unchanged), a new one otherwise
  std::vector<double4 *> recs((size_t)n);
  std::vector<char> fresh((size_t)n, 0);
  bool any_reuse = false;
  for (int k = 0; k < n; ++k) {
    auto it = c->maps.find(scene_ids[k]);
    if (it != c->maps.end() && it->second.kind == 0 && it->second.data && it->second.m2.W == W && it->second.m2.H == H) {
      recs[k] = static_cast<double4 *>(it->second.data);
      any_reuse = true;
    }
  }
  // nothing on the device may still read a buffer that is rewritten: one wait for the whole call
  if (any_reuse) HIPCHK(c, hipDeviceSynchronize());
  bool launched = false;
  auto undo = [&]() {  // a failed call leaves no half-written map behind: the scenes it rewrote have none any more
    hipStreamSynchronize(c->stream);
    for (int k = 0; k < n; ++k) {
      if (fresh[k]) hipFree(recs[k]);
      else if (recs[k] && launched) drop_locked(c, scene_ids[k]);
    }
  };
  for (int k = 0; k < n; ++k) {
    if (recs[k]) continue;
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, ncell * sizeof(double4));
    if (e != hipSuccess) {
      undo();
      return fail(c, NEO_ERR_HIP, std::string("batch build: hipMalloc of a record buffer: ") + hipGetErrorString(e));
    }
    recs[k] = static_cast<double4 *>(p);
    fresh[k] = 1;
  }
  {
    ProfScope ps(c, NEO_KERNEL_ESDF_BUILD);
    for (int k0 = 0; k0 < n; k0 += chunk) {
      const int nm = std::min(chunk, n - k0);
      Carver cv(c->scratch);  // (the passes follow one another on the stream: one carving serves them all)
      double4 **d_recs = cv.take<double4 *>((size_t)chunk);
      Edt2DWork w{};
      w.occ = occ + (size_t)k0 * ncell;
      w.g = cv.take<int>((size_t)chunk * ncell);
      w.dist = cv.take<double>((size_t)chunk * ncell);
      if (sweeps) {
        w.v = cv.take<int>((size_t)chunk * ncell);
        w.z = cv.take<double>((size_t)chunk * H * (W + 1));
      }
      const hipError_t e = hipMemcpyAsync(d_recs, recs.data() + k0, (size_t)nm * sizeof(double4 *), hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) {
        undo();
        return fail(c, NEO_ERR_HIP, std::string("batch build: ") + hipGetErrorString(e));
      }
      launched = true;
      esdf_build_2d_batch(c, w, nm, W, H, res, d_recs);
    }
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (also: `recs` outlives the copies that read it)
  if (e != hipSuccess) {
    undo();
    return fail(c, NEO_ERR_HIP, std::string("batch build: ") + hipGetErrorString(e));
  }
  for (int k = 0; k < n; ++k) {
    const double ox = origins[(size_t)k * 2], oy = origins[(size_t)k * 2 + 1];
    if (fresh[k]) {
      drop_locked(c, scene_ids[k]);  // (a map of another kind or size)
      DevBuf rec;
      rec.p = recs[k];
      adopt_map_2d(c, scene_ids[k], rec, W, H, res, ox, oy);
      continue;
    }
    MapEntry &en = c->maps.find(scene_ids[k])->second;
    const Map2D m{static_cast<const double4 *>(en.data), W, H, res, ox, oy};
    if (memcmp(&m, &en.m2, sizeof(m)) != 0) c->table_dirty = true;
    en.m2 = m;
    en.version = ++c->map_serial;  // new contents: the geo mask is stale
  }
  return NEO_OK;
}

int neo_esdf_upload_3d(neo_ctx *c, int scene_id, const void *dist, int src_dtype, int src_is_device, int nx, int ny,
                       int nz, double res, const double origin[3], int store_dtype, int layout) {
  if (!c || !dist || !origin || nx < 2 || ny < 2 || nz < 2 || !(res > 0.0)) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (src_dtype != NEO_F64 && src_dtype != NEO_F32) return fail(c, NEO_ERR_INVALID, "src_dtype must be f64 or f32");
  if (store_dtype != NEO_F32 && store_dtype != NEO_F16)
    return fail(c, NEO_ERR_INVALID, "store_dtype must be f32 or f16");
  if (layout != NEO_LAYOUT_LINEAR && layout != NEO_LAYOUT_YZ4 && layout != NEO_LAYOUT_CELL8 && layout != NEO_LAYOUT_BRICK)
    return fail(c, NEO_ERR_INVALID, "bad layout");
  // the lookups form voxel indices with 24-bit multiplies: (iz * ny + iy) * nx + ix
  if ((size_t)ny * nz >= ((size_t)1 << 24) || (size_t)nx >= ((size_t)1 << 24))
    return fail(c, NEO_ERR_INVALID, "field too large: ny * nz and nx must be below 2^24");
  hipSetDevice(c->device);
  drop_locked(c, scene_id);
  const size_t nvox = (size_t)nx * ny * nz;
  const size_t ssz = src_dtype == NEO_F64 ? 8 : 4, dsz = store_dtype == NEO_F32 ? 4 : 2;
  // corner bricks: blocks of 2 x 2 x 2 cells (fp32) / 4 x 2 x 2 cells (fp16), one 128-byte line each
  const int bshx = store_dtype == NEO_F32 ? 1 : 2;
  const int nbx = ((nx - 1) + (1 << bshx) - 1) >> bshx, nby = (ny - 1 + 1) / 2, nbz = (nz - 1 + 1) / 2;
  const size_t nstore = layout == NEO_LAYOUT_YZ4 ? nvox * 4 : (layout == NEO_LAYOUT_CELL8 ? nvox * 8 :
                        (layout == NEO_LAYOUT_BRICK ? (size_t)nbx * nby * nbz * (128 / dsz) : nvox));
  if ((nstore + 64) * dsz >= (size_t)4 << 30) return fail(c, NEO_ERR_INVALID, "field too large for 32-bit buffer offsets in this layout");
  if (layout == NEO_LAYOUT_BRICK && (nby > 65535 || nbz > 65535))
    return fail(c, NEO_ERR_INVALID, "field too large for the brick layout: at most 131070 voxels along y and z");
  const void *src = dist;
  DevBuf staged, field;
  if (!src_is_device) {
    HIPCHK(c, staged.alloc(nvox * ssz));
    HIPCHK(c, hipMemcpyAsync(staged.p, dist, nvox * ssz, hipMemcpyHostToDevice, c->stream));
    src = staged.p;
  }
  MapEntry e;
  e.kind = 1;
  e.elem = store_dtype;
  // +64 elements of slack: the x-pair load of the last voxel row touches one element past the end
  HIPCHK(c, field.alloc((nstore + 64) * dsz));
  // (the pack kernels write every stored element; only the 64 elements of padding behind them need zeroing)
  HIPCHK(c, hipMemsetAsync(static_cast<char *>(field.p) + nstore * dsz, 0, 64 * dsz, c->stream));
  esdf_pack_3d(c, src, src_dtype, nx, ny, nz, store_dtype, layout, nbx, nby, nbz, field.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  e.data = field.release();
  e.m3 = Map3D{e.data, nx, ny, nz, layout, res, origin[0], origin[1], origin[2], (unsigned int)((nstore + 64) * dsz)};
  e.m3.derive();
  e.m3.nbx = nbx;
  e.m3.nby = nby;
  c->maps[scene_id] = e;
  c->table_dirty = true;
  return NEO_OK;
}

int neo_esdf_build_3d(neo_ctx *c, int scene_id, const uint8_t *occ, int occ_is_device, int nx, int ny, int nz,
                      double res, const double origin[3], int store_dtype, int layout, float *out_dist) {
  if (!c || !occ || !origin || nx < 2 || ny < 2 || nz < 2 || !(res > 0.0)) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (store_dtype != NEO_F32 && store_dtype != NEO_F16) return fail(c, NEO_ERR_INVALID, "store_dtype must be f32 or f16");
  if (nx > 4096 || ny > 4096 || nz > 4096) return fail(c, NEO_ERR_INVALID, "3-D ESDF build: at most 4096 voxels per axis");
  const size_t nvox = (size_t)nx * ny * nz;
  // the passes' intermediates and the fp32 distances live in the context's scratch buffer (kept between calls: a map
  // update at sensor rate then allocates nothing but the field itself)
  float *d_dist_p = nullptr;
  {
    hipSetDevice(c->device);
    DevBuf d_occ;
    const uint8_t *src = occ;
    if (!occ_is_device) {
      HIPCHK(c, d_occ.alloc(nvox));
      HIPCHK(c, hipMemcpyAsync(d_occ.p, occ, nvox, hipMemcpyHostToDevice, c->stream));
      src = d_occ.as<uint8_t>();
    }
    int rc = ensure_scratch(c, nvox * (sizeof(uint16_t) + sizeof(uint32_t) + sizeof(float)) + 4 * 256);
    if (rc) return rc;
    Carver cv(c->scratch);
    uint16_t *d_gx = cv.take<uint16_t>(nvox);
    uint32_t *d_sq = cv.take<uint32_t>(nvox);
    d_dist_p = cv.take<float>(nvox);
    {
      ProfScope ps(c, NEO_KERNEL_ESDF_BUILD);
      esdf_edt_3d(c, src, nx, ny, nz, res, d_gx, d_sq, d_dist_p);
    }
    HIPCHK(c, hipGetLastError());
    if (out_dist) HIPCHK(c, hipMemcpyAsync(out_dist, d_dist_p, nvox * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  const int rc_up = neo_esdf_upload_3d(c, scene_id, d_dist_p, NEO_F32, 1, nx, ny, nz, res, origin, store_dtype, layout);
  // the intermediates stay in the context's scratch for the next update of a scene of this size -- up to 512 MB (a 300^3
  // scene: 270 MB); beyond that (600^3: 2.2 GB, 1000^3: 10 GB) they are released, a map build does not pin gigabytes of
  // HBM for the lifetime of the context
  if (c->scratch_bytes > ((size_t)512 << 20)) {
    hipStreamSynchronize(c->stream);
    hipFree(c->scratch);
    c->scratch = nullptr;
    c->scratch_bytes = 0;
  }
  return rc_up;
}

int neo_esdf_query(neo_ctx *c, int scene_id, int n, const double *pts, double *dist, double *grad) {
  if (!c || n < 0 || !pts || !dist) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  auto it = c->maps.find(scene_id);
  if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "no ESDF for this scene");
  if (n == 0) return NEO_OK;
  const MapEntry &e = it->second;
  const int dm = e.kind == 0 ? 2 : 3;
  HostStage st(c, 0);
  const auto f_p = st.in(pts, (size_t)n * dm);
  const auto f_d = st.out(dist, (size_t)n), f_g = st.out(grad, (size_t)n * dm);
  int rc = st.upload();
  if (rc) return rc;
  double *d_p = st.dev(f_p), *d_d = st.dev(f_d), *d_g = st.dev(f_g);
  esdf_query(c, e, n, d_p, d_d, d_g);
  return st.download();
}

int neo_cost_grad_batch_dev(neo_ctx *c, int scene_id, int B, int M, int D, const double *x, const double *head,
                            const double *tail, double *cost, double *costs4, double *grad, double *coeffs,
                            int32_t *status) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x || !head || !tail || !cost || !costs4 || !grad) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  auto it = c->maps.find(scene_id);
  if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "no ESDF for this scene");
  if (B == 0) return NEO_OK;
  ProfScope ps(c, NEO_KERNEL_EVAL);
  const EvalArgs ea{B, M, x, head, tail, cost, costs4, grad, coeffs, status};
  return launched(c, dispatch_eval(c, it->second, D, ea));
}

int neo_cost_grad_batch(neo_ctx *c, int scene_id, int B, int M, int D, const double *x, const double *head,
                        const double *tail, double *cost, double *costs4, double *grad, double *coeffs,
                        int32_t *status) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x || !head || !tail || !cost || !costs4 || !grad) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  HostStage st(c, kStagedUpTo);  // (get_cost / get_grad of one trajectory: one copy each way)
  const auto fx = st.in(x, bs * n), fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  const auto fc = st.out(cost, bs), fc4 = st.out(costs4, bs * 4), fg = st.out(grad, bs * n);
  const auto fco = st.out(coeffs, bs * 6 * M * D);
  const auto fst = st.out(status, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_cost_grad_batch_dev(c, scene_id, B, M, D, st.dev(fx), st.dev(fh), st.dev(ft), st.dev(fc), st.dev(fc4), st.dev(fg),
                               coeffs ? st.dev(fco) : nullptr, st.dev(fst));
  if (rc) return rc;
  return st.download();
}

// IO32: coeffs / grad_C / grad_T are floats (the _f32 entry points; fp32 sampling only)
static int sampled_terms_dev(neo_ctx *c, int scene_id, int B, int M, int D, const void *coeffs, const double *ts, double *costs2,
                             void *grad_C, void *grad_T, bool io32) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!coeffs || !ts || !costs2 || !grad_C || !grad_T) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (((uintptr_t)coeffs | (uintptr_t)grad_C) & (io32 ? 7 : 15))
    return fail_locked(c, NEO_ERR_INVALID, io32 ? "coeffs and grad_C must be 8-byte aligned" : "coeffs and grad_C must be 16-byte aligned");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  auto it = c->maps.find(scene_id);
  if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "no ESDF for this scene");
  if (B == 0) return NEO_OK;
  ProfScope ps(c, NEO_KERNEL_ESDF_SAMPLE);
  SampleArgs sa{B, M, coeffs, ts, costs2, grad_C, grad_T};
  sa.io32 = io32;
  return launched(c, dispatch_sample(c, it->second, D, sa));
}

int neo_sampled_terms_batch_dev(neo_ctx *c, int scene_id, int B, int M, int D, const double *coeffs,
                                const double *ts, double *costs2, double *grad_C, double *grad_T) {
  return sampled_terms_dev(c, scene_id, B, M, D, coeffs, ts, costs2, grad_C, grad_T, false);
}

int neo_sampled_terms_batch_f32_dev(neo_ctx *c, int scene_id, int B, int M, int D, const float *coeffs,
                                    const double *ts, double *costs2, float *grad_C, float *grad_T) {
  return sampled_terms_dev(c, scene_id, B, M, D, coeffs, ts, costs2, grad_C, grad_T, true);
}

static int sampled_terms_host(neo_ctx *c, int scene_id, int B, int M, int D, const void *coeffs, const double *ts, double *costs2,
                              void *grad_C, void *grad_T, bool io32) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!coeffs || !ts || !costs2 || !grad_C || !grad_T) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B, nc = (size_t)6 * M * D, es = io32 ? sizeof(float) : sizeof(double);
  // coeffs / grad_C / grad_T as bytes: floats or doubles on the wire, sized for doubles either way
  HostStage st(c, 0);
  const auto fco = st.in(static_cast<const char *>(coeffs), bs * nc * es, bs * nc * sizeof(double));
  const auto fts = st.in(ts, bs * M);
  const auto fc2 = st.out(costs2, bs * 2);
  const auto fgc = st.out(static_cast<char *>(grad_C), bs * nc * es, bs * nc * sizeof(double));
  const auto fgt = st.out(static_cast<char *>(grad_T), bs * M * es, bs * M * sizeof(double));
  rc = st.upload();
  if (rc) return rc;
  rc = sampled_terms_dev(c, scene_id, B, M, D, st.dev(fco), st.dev(fts), st.dev(fc2), st.dev(fgc), st.dev(fgt), io32);
  if (rc) return rc;
  return st.download();
}

int neo_sampled_terms_batch(neo_ctx *c, int scene_id, int B, int M, int D, const double *coeffs, const double *ts,
                            double *costs2, double *grad_C, double *grad_T) {
  return sampled_terms_host(c, scene_id, B, M, D, coeffs, ts, costs2, grad_C, grad_T, false);
}

int neo_sampled_terms_batch_f32(neo_ctx *c, int scene_id, int B, int M, int D, const float *coeffs, const double *ts,
                                double *costs2, float *grad_C, float *grad_T) {
  return sampled_terms_host(c, scene_id, B, M, D, coeffs, ts, costs2, grad_C, grad_T, true);
}

// the L-BFGS pairs (2 * maxcor * n doubles per trajectory) live in LDS: no HBM workspace
size_t neo_optimize_workspace_bytes(int, int, int) { return 0; }

// the maps of a `_dev` call (neo_optimize_batch_from_dev, neo_audit_traj_batch_dev): with slots, the whole table of the
// reference scene's kind -- one kernel instantiation serves the whole call, so every map a slot can name (all maps of
// that kind in this context) must share its element type and layout; without, the one map of scene_id.
// Call with the context locked and the tables rebuilt.
struct CallMaps {
  int kind = 0, elem = 0, layout = 0, nmaps = 1;
  const void *table = nullptr;
};
static int resolve_call_maps(neo_ctx *c, int scene_id, bool with_slots, CallMaps &cm) {
  if (with_slots) {
    auto it = c->maps.find(scene_id);
    if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "no ESDF for the reference scene");
    cm.kind = it->second.kind;
    cm.elem = it->second.elem;
    cm.layout = it->second.m3.layout;
    for (const auto &kv : c->maps)
      if (kv.second.kind == cm.kind && (kv.second.elem != cm.elem || (cm.kind == 1 && kv.second.m3.layout != cm.layout)))
        return fail(c, NEO_ERR_INVALID, "multi-scene call: the context holds maps of this kind with different element "
                                        "types or layouts");
    cm.table = cm.kind == 0 ? c->table2d : c->table3d;
    cm.nmaps = cm.kind == 0 ? c->n2d : c->n3d;
  } else {
    auto it = c->maps.find(scene_id);
    if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "no ESDF for this scene");
    cm.kind = it->second.kind;
    cm.elem = it->second.elem;
    cm.layout = it->second.m3.layout;
    const char *base = static_cast<const char *>(cm.kind == 0 ? c->table2d : c->table3d);
    cm.table = base + (size_t)it->second.slot * (cm.kind == 0 ? sizeof(Map2D) : sizeof(Map3D));
    cm.nmaps = 1;
  }
  return NEO_OK;
}

int neo_optimize_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, int M, int D, double *x,
                           const double *head, const double *tail, double *costs4, double *costs4_last, int32_t *nit,
                           int32_t *nfev, int32_t *status) {
  return neo_optimize_batch_from_dev(c, scene_id, scene_ids, B, M, D, x, x, head, tail, costs4, costs4_last, nit, nfev,
                                     status);
}

int neo_optimize_batch_from_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, int M, int D, const double *x0,
                                double *x, const double *head, const double *tail, double *costs4, double *costs4_last,
                                int32_t *nit, int32_t *nfev, int32_t *status) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x0 || !x || !head || !tail || !costs4 || !nit || !nfev || !status)
    return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (B == 0) return NEO_OK;
  rc = rebuild_tables(c);
  if (rc) return rc;
  // scene_ids (device array) holds map-table SLOTS when given; a single scene_id is looked up here
  CallMaps cm;
  rc = resolve_call_maps(c, scene_id, scene_ids != nullptr, cm);
  if (rc) return rc;
  const int kind = cm.kind, elem = cm.elem, layout = cm.layout, nmaps = cm.nmaps;
  const void *table = cm.table;
  const int *slots = scene_ids;
  const OptArgs oa{B, M, table, slots, nmaps, x0, x, head, tail, costs4, costs4_last, nit, nfev, status};
  // the lane-group kernel records no evaluations and counts no finished trajectories: refuse instead of leaving the
  // caller's trace zero-filled and its progress counter still
  if (lane_group_launch(c, kind, layout, D, oa) && (c->trace || c->trace_xg || c->progress))
    return fail(c, NEO_ERR_INVALID, "lane-group launch (NEO_FLAG_LANE_GROUPS): neo_optimize_trace, neo_optimize_trace_xg "
                                    "and neo_optimize_progress_counter are not supported");
  ProfScope ps(c, NEO_KERNEL_OPTIMIZE);
  return launched(c, dispatch_opt(c, kind, elem, layout, D, oa));
}

size_t neo_optimize_state_bytes(int M, int D) {
  if (M < 1 || D < 1) return 0;
  return opt_state_doubles(D * (M - 1) + M, NEO_LBFGS_M) * sizeof(double);
}

int neo_optimize_batch_budget_dev(neo_ctx *c, int scene_id, int B, int M, int D, const double *x0, double *x, const double *head,
                                  const double *tail, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                                  int32_t *status, void *state, int eval_budget, const int32_t *subset, int n_subset,
                                  int resume) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x0 || !x || !head || !tail || !costs4 || !nit || !nfev || !status || !state)
    return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (eval_budget < 1) return fail_locked(c, NEO_ERR_INVALID, "eval_budget < 1");
  if (subset && (n_subset < 0 || n_subset > B)) return fail_locked(c, NEO_ERR_INVALID, "bad subset size");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (B == 0 || (subset && n_subset == 0)) return NEO_OK;
  rc = rebuild_tables(c);
  if (rc) return rc;
  auto it = c->maps.find(scene_id);
  if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "no ESDF for this scene");
  if (it->second.kind == 0 || D != 3) return fail(c, NEO_ERR_INVALID, "budgeted launches: 3-D fields, D = 3");
  if (c->trace || c->trace_xg) return fail(c, NEO_ERR_INVALID, "budgeted launches do not record traces");
  if (c->progress)
    return fail(c, NEO_ERR_INVALID, "budgeted launches do not count finished trajectories (neo_optimize_progress_counter)");
  const char *base = static_cast<const char *>(c->table3d);
  const void *table = base + (size_t)it->second.slot * sizeof(Map3D);
  ProfScope ps(c, NEO_KERNEL_OPTIMIZE);
  OptArgs oa{B, M, table, nullptr, 1, x0, x, head, tail, costs4, costs4_last, nit, nfev, status};
  oa.state = static_cast<double *>(state);
  oa.state_doubles = (int)opt_state_doubles(D * (M - 1) + M, NEO_LBFGS_M);
  oa.budget = eval_budget;
  oa.resume = resume ? 1 : 0;
  oa.subset = subset;
  oa.n_subset = subset ? n_subset : 0;
  oa.traj_total = B;
  return launched(c, launch_opt_3d_budget(c, it->second.elem, it->second.m3.layout, oa));
}

int neo_scene_slot(neo_ctx *c, int scene_id) {
  if (!c) return -1;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (rebuild_tables(c)) return -1;
  auto it = c->maps.find(scene_id);
  return it == c->maps.end() ? -1 : it->second.slot;
}

int neo_optimize_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, int M, int D, double *x,
                       const double *head, const double *tail, double *costs4, double *costs4_last, int32_t *nit,
                       int32_t *nfev, int32_t *status) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x || !head || !tail || !costs4 || !nit || !nfev || !status) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  std::vector<int> slots;
  if (scene_ids) {
    rc = scene_slots(c, scene_ids, bs, false, slots);
    if (rc) return rc;
  }
  // the inputs are one contiguous range ending with x, the outputs one starting with it
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  const auto fs = st.in(scene_ids ? slots.data() : nullptr, bs);
  const auto fx = st.inout(x, bs * n);
  const auto fc4 = st.out(costs4, bs * 4), fc4l = st.out(costs4_last, bs * 4);
  const auto fnit = st.out(nit, bs), fnfev = st.out(nfev, bs), fst = st.out(status, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_optimize_batch_dev(c, scene_ids ? scene_ids[0] : scene_id, scene_ids ? st.dev(fs) : nullptr, B, M, D, st.dev(fx),
                              st.dev(fh), st.dev(ft), st.dev(fc4), st.dev(fc4l), st.dev(fnit), st.dev(fnfev), st.dev(fst));
  if (rc) return rc;
  return st.download();
}

int neo_eval_traj_batch(neo_ctx *c, int B, int M, int D, const double *x, const double *head, const double *tail,
                        double hz, int K, double *state, int32_t *count) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x || !head || !tail || !state || !count || K < 0 || !(hz > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "bad argument");
  if (B == 0 || K == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  HostStage st(c, kStagedUpTo);
  const auto fx = st.in(x, bs * n), fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  const auto fs = st.out(state, bs * K * 3 * D);
  const auto fcnt = st.out(count, bs);
  rc = st.upload();
  if (rc) return rc;
  double *dx = st.dev(fx), *dh = st.dev(fh), *dt = st.dev(ft), *ds = st.dev(fs);
  int *dcnt = st.dev(fcnt);
  if (D == 2)
    hipLaunchKernelGGL((traj_state_kernel<2>), dim3(B), dim3(kWave), 0, c->stream, B, M, c->dev, dx, dh, dt, hz, K, ds,
                       dcnt);
  else
    hipLaunchKernelGGL((traj_state_kernel<3>), dim3(B), dim3(kWave), 0, c->stream, B, M, c->dev, dx, dh, dt, hz, K, ds,
                       dcnt);
  HIPCHK(c, hipGetLastError());
  return st.download();
}

// ---- trajectory audit (ros_node/traj_planner_node.py:333-363; kernel: neo_audit.hpp)
// the argument checks both forms make before anything is copied or launched (context unlocked)
static int audit_check(neo_ctx *c, int B, int M, int D, const double *x, const double *head, const double *tail, double hz,
                       const double *audit, const int32_t *count, const int32_t *flags) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x || !head || !tail || !audit || !count || !flags) return fail_locked(c, NEO_ERR_INVALID, "audit: null buffer");
  if (!std::isfinite(hz) || !(hz > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "audit: hz must be finite and > 0");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  // a trajectory lasts at most M * T_max: its sample count must fit the kernel's int range with room to spare
  if (!((double)M * c->params.T_max * hz < (double)(1 << 30)))
    return fail(c, NEO_ERR_INVALID, "audit: hz too large (M * T_max * hz must stay below 2^30 samples)");
  return NEO_OK;
}

int neo_audit_traj_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, int M, int D, const double *x,
                             const double *head, const double *tail, double hz, const double *weights3, double *audit,
                             int32_t *count, int32_t *flags) {
  int rc = audit_check(c, B, M, D, x, head, tail, hz, audit, count, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  rc = rebuild_tables(c);
  if (rc) return rc;
  CallMaps cm;
  rc = resolve_call_maps(c, scene_id, scene_ids != nullptr, cm);
  if (rc) return rc;
  if (cm.kind == 1 && D != 3) return fail(c, NEO_ERR_INVALID, "audit: a 3-D map needs D = 3");
  if (B == 0) return NEO_OK;
  AuditArgs aa{B, M, {cm.table, scene_ids, cm.nmaps}, x, head, tail, hz, {1.0, 1.0, 100.0}, audit, count, flags};
  if (weights3)
    for (int k = 0; k < 3; ++k) aa.w[k] = weights3[k];
  return launched(c, dispatch_audit(c, cm.kind, cm.elem, cm.layout, D, aa));
}

int neo_audit_traj_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, int M, int D, const double *x,
                         const double *head, const double *tail, double hz, const double *weights3, double *audit,
                         int32_t *count, int32_t *flags) {
  int rc = audit_check(c, B, M, D, x, head, tail, hz, audit, count, flags);
  if (rc) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  std::vector<int> slots;
  if (scene_ids) {
    rc = scene_slots(c, scene_ids, bs, false, slots);
    if (rc) return rc;
  }
  HostStage st(c, 0);
  const auto fx = st.in(x, bs * n), fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  const auto fs = st.in(scene_ids ? slots.data() : nullptr, bs);
  const auto fa = st.out(audit, bs * NEO_AUDIT_FIELDS);
  const auto fcnt = st.out(count, bs), ffl = st.out(flags, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_audit_traj_batch_dev(c, scene_ids ? scene_ids[0] : scene_id, scene_ids ? st.dev(fs) : nullptr, B, M, D, st.dev(fx),
                                st.dev(fh), st.dev(ft), hz, weights3, st.dev(fa), st.dev(fcnt), st.dev(ffl));
  if (rc) return rc;
  return st.download();
}

// ---- batched depth camera (neo_planner_amd/initializer.py raycast_depth for B requests; kernels: neo_depth.hpp)
// the argument checks both forms make before anything is copied or launched (context unlocked)
static int depth_check(neo_ctx *c, int width, int height, double focal_px, double max_range, const double *boxes,
                       const int32_t *box_begin, int n_scenes, int B, const double *pose, const float *depth_m) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 1) return fail_locked(c, NEO_ERR_INVALID, "depth: B must be >= 1");
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    return fail_locked(c, NEO_ERR_INVALID, "depth: width and height must be in 1..4096");
  if (!std::isfinite(focal_px) || !(focal_px > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "depth: focal_px must be finite and > 0");
  if (!std::isfinite(max_range) || !(max_range > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "depth: max_range must be finite and > 0");
  if (n_scenes < 1) return fail_locked(c, NEO_ERR_INVALID, "depth: n_scenes must be >= 1");
  if (!boxes || !box_begin || !pose || !depth_m) return fail_locked(c, NEO_ERR_INVALID, "depth: null buffer");
  return NEO_OK;
}

int neo_depth_render_batch_dev(neo_ctx *c, int width, int height, double focal_px, double max_range, const double *boxes,
                               const int32_t *box_begin, int n_scenes, const int32_t *scene_index, int B,
                               const double *pose, float *depth_m, uint8_t *depth_u8, float *depth_max) {
  int rc = depth_check(c, width, height, focal_px, max_range, boxes, box_begin, n_scenes, B, pose, depth_m);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return depth_render(c, DepthCall{width, height, focal_px, max_range, boxes, box_begin, n_scenes, scene_index, B, pose,
                                   depth_m, depth_u8, depth_max});
}

int neo_depth_render_batch(neo_ctx *c, int width, int height, double focal_px, double max_range, const double *boxes,
                           const int32_t *box_begin, int n_scenes, const int32_t *scene_index, int B, const double *pose,
                           float *depth_m, uint8_t *depth_u8, float *depth_max) {
  int rc = depth_check(c, width, height, focal_px, max_range, boxes, box_begin, n_scenes, B, pose, depth_m);
  if (rc) return rc;
  // what the device form cannot read on the host
  if (box_begin[0] != 0) return fail_locked(c, NEO_ERR_INVALID, "depth: box_begin must start at 0");
  for (int s = 0; s < n_scenes; ++s) {
    if (box_begin[s + 1] < box_begin[s]) return fail_locked(c, NEO_ERR_INVALID, "depth: box_begin must be non-decreasing");
    if (box_begin[s + 1] - box_begin[s] > NEO_DEPTH_MAX_BOXES)
      return fail_locked(c, NEO_ERR_INVALID, "depth: a scene has more than NEO_DEPTH_MAX_BOXES boxes");
  }
  if (scene_index)
    for (int b = 0; b < B; ++b)
      if (scene_index[b] < 0 || scene_index[b] >= n_scenes)
        return fail_locked(c, NEO_ERR_INVALID, "depth: a scene_index is outside 0 .. n_scenes - 1");
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B, hw = (size_t)width * height, nbox = (size_t)box_begin[n_scenes];
  HostStage st(c, 0);
  const auto fb = st.in(nbox ? boxes : nullptr, nbox * 6, 6);  // (without any box: a valid pointer nothing is read from)
  const auto fbb = st.in(box_begin, (size_t)n_scenes + 1);
  const auto fsi = st.in(scene_index, bs);
  const auto fp = st.in(pose, bs * 5);
  const auto fm = st.out(depth_m, bs * hw);
  const auto fu = st.out(depth_u8, depth_u8 ? bs * hw : 0);
  const auto fx = st.out(depth_max, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_depth_render_batch_dev(c, width, height, focal_px, max_range, st.dev(fb), st.dev(fbb), n_scenes,
                                  scene_index ? st.dev(fsi) : nullptr, B, st.dev(fp), st.dev(fm),
                                  depth_u8 ? st.dev(fu) : nullptr, st.dev(fx));
  if (rc) return rc;
  return st.download();
}

int neo_depth_box_test_counter(neo_ctx *c, uint64_t *dev_count) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->depth.box_tests = reinterpret_cast<unsigned long long *>(dev_count);
  return NEO_OK;
}

// ---- onboard mapping (launch/map_server_onboard.launch: octomap_server's scan insertion projected to 2-D; kernel:
// neo_onboard.hpp).  The checks both forms make before anything is copied or launched (context unlocked); N and half
// are the samples a ray and the window's reach in cells.
static int onboard_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *depth_m, const double *pose,
                         int width, int height, double focal_px, double max_range, int grid_w, int grid_h, double res,
                         const double *origins, double sensor_range, double z_lo, double z_hi, int l_hit, int l_miss,
                         int l_lo, int l_hi, const int8_t *logodds, const int8_t *occupancy, const int32_t *changed, int &N,
                         int &half) {
  int rc = list_check(c, "onboard", B, 1, 1 << 20, subset, n_subset);
  if (rc) return rc;
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: width and height must be in 1..4096");
  if (!std::isfinite(focal_px) || !(focal_px > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "onboard: focal_px must be finite and > 0");
  if (!std::isfinite(res) || !(res > 0.0)) return fail_locked(c, NEO_ERR_INVALID, "onboard: resolution must be finite and > 0");
  if (!std::isfinite(sensor_range) || !(sensor_range > 0.0))
    return fail_locked(c, NEO_ERR_INVALID, "onboard: sensor_range must be finite and > 0");
  if (!(max_range >= sensor_range))
    return fail_locked(c, NEO_ERR_INVALID, "onboard: the camera's max_range must reach sensor_range (a depth clipped below "
                                           "it would read as a hit)");
  if (!std::isfinite(z_lo) || !std::isfinite(z_hi) || !(z_lo <= z_hi))
    return fail_locked(c, NEO_ERR_INVALID, "onboard: the band needs finite z_lo <= z_hi");
  if (grid_w < 1 || grid_h < 1 || (size_t)grid_w * grid_h > (size_t)1 << 30)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: grid width and height >= 1, at most 2^30 cells");
  if (l_lo < -127 || l_hi > 127 || l_lo > l_hi || l_hit < 0 || l_hit > 127 || l_miss > 0 || l_miss < -127)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: log-odds need -127 <= lo <= hi <= 127, 0 <= hit <= 127, -127 <= miss <= 0");
  if (!depth_m || !pose || !origins || !logodds || !occupancy || !changed)
    return fail_locked(c, NEO_ERR_INVALID, "onboard: null buffer");
  const double nd = std::ceil(sensor_range / (res / 2.0));
  half = onboard_window_half(width, focal_px, sensor_range, res);
  if (!(nd <= 32767.0) || half > 4096 || onboard_lds_need(half, (int)nd, height) > onboard_lds_limit())
    return fail_locked(c, NEO_ERR_INVALID, "onboard: the window a scan can touch (sensor_range against the resolution and "
                                           "the camera's field of view) does not fit the 64 KB of LDS a workgroup has");
  N = (int)nd;
  return NEO_OK;
}

int neo_onboard_integrate_batch_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *depth_m,
                                    const double *pose, int width, int height, double focal_px, double max_range, int grid_w,
                                    int grid_h, double res, const double *origins, double sensor_range, double z_lo,
                                    double z_hi, int l_hit, int l_miss, int l_lo, int l_hi, int8_t *logodds,
                                    int8_t *occupancy, int32_t *changed) {
  int N = 0, half = 0;
  int rc = onboard_check(c, B, subset, n_subset, depth_m, pose, width, height, focal_px, max_range, grid_w, grid_h, res,
                         origins, sensor_range, z_lo, z_hi, l_hit, l_miss, l_lo, l_hi, logodds, occupancy, changed, N, half);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return onboard_integrate(c, OnboardCall{list, depth_m, pose, width, height, focal_px, grid_w, grid_h, res,
                                          origins, sensor_range, z_lo, z_hi, l_hit, l_miss, l_lo, l_hi, N, half, logodds,
                                          occupancy, changed});
}

int neo_onboard_integrate_batch(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *depth_m,
                                const double *pose, int width, int height, double focal_px, double max_range, int grid_w,
                                int grid_h, double res, const double *origins, double sensor_range, double z_lo, double z_hi,
                                int l_hit, int l_miss, int l_lo, int l_hi, int8_t *logodds, int8_t *occupancy,
                                int32_t *changed) {
  int N = 0, half = 0;
  int rc = onboard_check(c, B, subset, n_subset, depth_m, pose, width, height, focal_px, max_range, grid_w, grid_h, res,
                         origins, sensor_range, z_lo, z_hi, l_hit, l_miss, l_lo, l_hi, logodds, occupancy, changed, N, half);
  if (rc) return rc;
  if (subset) {
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n_subset; ++i) {
      if (subset[i] < 0 || subset[i] >= B) return fail_locked(c, NEO_ERR_INVALID, "onboard: a subset entry is outside 0 .. B - 1");
      if (seen[subset[i]]) return fail_locked(c, NEO_ERR_INVALID, "onboard: a mission is listed twice in the subset");
      seen[subset[i]] = 1;
    }
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B, nl = (size_t)launch_list(B, subset, n_subset).n, hw = (size_t)width * height;
  const size_t ncell = (size_t)grid_w * grid_h;
  if (nl == 0) return NEO_OK;
  HostStage st(c, 0);
  const auto fsub = st.in_optional(subset, nl);
  const auto fd = st.in(depth_m, nl * hw);
  const auto fp = st.in(pose, nl * 5);
  const auto fo = st.in(origins, bs * 2);
  const auto fl = st.inout(logodds, bs * ncell);    // (missions outside the subset keep their grids)
  const auto fc = st.inout(occupancy, bs * ncell);
  const auto fg = st.inout(changed, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_onboard_integrate_batch_dev(c, B, st.dev(fsub), n_subset, st.dev(fd), st.dev(fp), width, height,
                                       focal_px, max_range, grid_w, grid_h, res, st.dev(fo), sensor_range, z_lo, z_hi, l_hit,
                                       l_miss, l_lo, l_hi, st.dev(fl), st.dev(fc), st.dev(fg));
  if (rc) return rc;
  return st.download();
}

// ---- fleet replan loop (ros_node/traj_planner_node.py:390-578; kernels: neo_fleet.hpp)
static bool fleet_positive(double v) { return std::isfinite(v) && v > 0.0; }

// the 2-D maps of a fleet call (context locked)
static int fleet_maps(neo_ctx *c, int scene_id, const int32_t *slots, MapRef &m) {
  int rc = rebuild_tables(c);
  if (rc) return rc;
  CallMaps cm;
  rc = resolve_call_maps(c, scene_id, slots != nullptr, cm);
  if (rc) return rc;
  if (cm.kind != 0) return fail(c, NEO_ERR_INVALID, "fleet: the 2-D reference map only (a 3-D map was given)");
  m = {cm.table, slots, cm.nmaps};
  return NEO_OK;
}

static int fleet_target_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cur_pos,
                              const double *goal, const double *jitter, double longitu, double lateral, double move_vel,
                              const double *tail, const int32_t *near_goal, const int32_t *lateral_steps,
                              const int32_t *flags) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!cur_pos || !goal || !jitter || !tail || !near_goal || !lateral_steps || !flags)
    return fail_locked(c, NEO_ERR_INVALID, "fleet target: null buffer");
  if (!fleet_positive(longitu) || !fleet_positive(lateral) || !std::isfinite(move_vel))
    return fail_locked(c, NEO_ERR_INVALID, "fleet target: longitu_step_dis and lateral_step_length must be finite and > 0, "
                                           "move_vel finite");
  return NEO_OK;
}

int neo_fleet_target_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset,
                               int n_subset, const double *cur_pos, const double *goal, const double *jitter,
                               double longitu_step_dis, double lateral_step_length, double move_vel, double *tail,
                               int32_t *near_goal, int32_t *lateral_steps, int32_t *flags) {
  int rc = fleet_target_check(c, B, subset, n_subset, cur_pos, goal, jitter, longitu_step_dis, lateral_step_length,
                              move_vel, tail, near_goal, lateral_steps, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  MapRef maps;
  rc = fleet_maps(c, scene_id, scene_ids, maps);
  if (rc) return rc;
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_target(c, list, maps, {cur_pos, goal, jitter, longitu_step_dis, lateral_step_length, move_vel,
                                                  tail, near_goal, lateral_steps, flags}));
}

int neo_fleet_target_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset, int n_subset,
                           const double *cur_pos, const double *goal, const double *jitter, double longitu_step_dis,
                           double lateral_step_length, double move_vel, double *tail, int32_t *near_goal,
                           int32_t *lateral_steps, int32_t *flags) {
  int rc = fleet_target_check(c, B, subset, n_subset, cur_pos, goal, jitter, longitu_step_dis, lateral_step_length,
                              move_vel, tail, near_goal, lateral_steps, flags);
  if (rc) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  std::vector<int> slots;
  if (scene_ids) {
    rc = scene_slots(c, scene_ids, bs, false, slots);
    if (rc) return rc;
  }
  // all arrays small: the pinned mirror.  The outputs go up too: missions outside the subset keep their rows
  HostStage st(c, kStagedUpTo);
  const auto fp = st.in(cur_pos, bs * 2), fg = st.in(goal, bs * 2), fj = st.in(jitter, bs * 2);
  const auto fs = st.in(scene_ids ? slots.data() : nullptr, bs);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto ft = st.inout(tail, bs * 6);
  const auto fn = st.inout(near_goal, bs), fl = st.inout(lateral_steps, bs), ff = st.inout(flags, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_fleet_target_batch_dev(c, scene_ids ? scene_ids[0] : scene_id, scene_ids ? st.dev(fs) : nullptr, B,
                                  st.dev(fsub), n_subset, st.dev(fp), st.dev(fg), st.dev(fj), longitu_step_dis, lateral_step_length, move_vel, st.dev(ft), st.dev(fn), st.dev(fl),
                                  st.dev(ff));
  if (rc) return rc;
  return st.download();
}

static int fleet_jitter_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int tick, int target,
                              const double *jitter) {
  int rc = list_check(c, "fleet jitter", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!jitter) return fail_locked(c, NEO_ERR_INVALID, "fleet jitter: null buffer");
  if (tick < 0 || target < 0) return fail_locked(c, NEO_ERR_INVALID, "fleet jitter: tick and target must be >= 0");
  return NEO_OK;
}

int neo_fleet_jitter_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, uint64_t seed, int tick, int target,
                         const int32_t *mission_ids, double *jitter) {
  int rc = fleet_jitter_check(c, B, subset, n_subset, tick, target, jitter);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_jitter(c, list, seed, tick, target, mission_ids, jitter));
}

int neo_fleet_jitter(neo_ctx *c, int B, const int32_t *subset, int n_subset, uint64_t seed, int tick, int target,
                     const int32_t *mission_ids, double *jitter) {
  int rc = fleet_jitter_check(c, B, subset, n_subset, tick, target, jitter);
  if (rc) return rc;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  // the rows go up too: missions outside the subset keep theirs
  HostStage st(c, kStagedUpTo);
  const auto fi = st.in_optional(mission_ids, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fj = st.inout(jitter, bs * 2);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_fleet_jitter_dev(c, B, st.dev(fsub), n_subset, seed, tick, target, st.dev(fi), st.dev(fj));
  if (rc) return rc;
  return st.download();
}

static int fleet_cmd_check(neo_ctx *c, const char *who, const double *cmd, int cap, const int32_t *cmd_len,
                           const int32_t *cmd_index, const int32_t *future_index) {
  if (!cmd || !cmd_len || !cmd_index || !future_index)
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": null buffer").c_str());
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": cap must be > 0").c_str());
  return NEO_OK;
}

int neo_fleet_advance_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                          const int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int step, int ahead,
                          double *cur_pos, double *head) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_cmd_check(c, "fleet advance", cmd, cap, cmd_len, cmd_index, future_index);
  if (rc) return rc;
  if (!cur_pos || !head) return fail_locked(c, NEO_ERR_INVALID, "fleet advance: null buffer");
  if (step < 0 || step > (1 << 30) || ahead < 0 || ahead > (1 << 30))
    return fail_locked(c, NEO_ERR_INVALID, "fleet advance: step and ahead must be in 0 .. 2^30");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_advance(c, list, {const_cast<double *>(cmd), cap, const_cast<int32_t *>(cmd_len), cmd_index,
                                             future_index}, step, ahead, cur_pos, head));
}

int neo_fleet_pose_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                       const int32_t *cmd_len, const int32_t *cmd_index, const double *cur_pos, const double *goal,
                       double eye_z, double *pose) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!cmd || !cmd_len || !cmd_index || !cur_pos || !goal || !pose) return fail_locked(c, NEO_ERR_INVALID, "fleet pose: null buffer");
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet pose: cap must be > 0");
  if (!std::isfinite(eye_z)) return fail_locked(c, NEO_ERR_INVALID, "fleet pose: eye_z must be finite");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_pose(c, list, {const_cast<double *>(cmd), cap, const_cast<int32_t *>(cmd_len),
                                          const_cast<int32_t *>(cmd_index), nullptr}, cur_pos, goal, eye_z, pose));
}

int neo_fleet_splice_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *x, const double *head,
                         const double *tail, const int32_t *solved, double hz, int first, double *cmd, int cap,
                         int32_t *cmd_len, int32_t *cmd_index, int32_t *future_index, int32_t *flags) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = check_shape(c, B, M, 2);
  if (rc) return rc;
  rc = fleet_cmd_check(c, "fleet splice", cmd, cap, cmd_len, cmd_index, future_index);
  if (rc) return rc;
  if (!x || !head || !tail || !flags) return fail_locked(c, NEO_ERR_INVALID, "fleet splice: null buffer");
  if (!fleet_positive(hz)) return fail_locked(c, NEO_ERR_INVALID, "fleet splice: hz must be finite and > 0");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_splice(c, list, {cmd, cap, cmd_len, cmd_index, future_index},
                                  {M, x, head, tail, solved, hz, first ? 1 : 0, flags}));
}

// mode "warmstart": the state a mission carries from one plan to the next
static int fleet_warm_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M) {
  int rc = list_check(c, who, B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (M < 2 || M > NEO_MAX_PIECES) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": M must be in 2 .. 64").c_str());
  return NEO_OK;
}

int neo_fleet_warm_guess_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *head,
                             const double *wpts_local, const double *ts_carry, double *x0) {
  int rc = fleet_warm_check(c, "fleet warm guess", B, subset, n_subset, M);
  if (rc) return rc;
  if (!head || !wpts_local || !ts_carry || !x0) return fail_locked(c, NEO_ERR_INVALID, "fleet warm guess: null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_warm_guess(c, list, M, head, wpts_local, ts_carry, x0));
}

int neo_fleet_warm_carry_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *x,
                             const double *head, const int32_t *solved, const int32_t *status, const int32_t *attempts,
                             const double *init_ts, double *wpts_local, double *ts_carry) {
  int rc = fleet_warm_check(c, "fleet warm carry", B, subset, n_subset, M);
  if (rc) return rc;
  if (!x || !head || !solved || !status || !attempts || !init_ts || !wpts_local || !ts_carry)
    return fail_locked(c, NEO_ERR_INVALID, "fleet warm carry: null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_warm_carry(c, list, {M, x, head, solved, status, attempts, init_ts, wpts_local, ts_carry}));
}

static int fleet_audit_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                             const int32_t *n_flown, int stride, double cmd_hz, const double *audit, const int32_t *count,
                             const int32_t *flags) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!cmd || !n_flown || !audit || !count || !flags) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: null buffer");
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: cap must be > 0");
  if (stride <= 0) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: stride must be > 0");
  if (!fleet_positive(cmd_hz)) return fail_locked(c, NEO_ERR_INVALID, "fleet audit: cmd_hz must be finite and > 0");
  return NEO_OK;
}

int neo_fleet_audit_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset, int n_subset,
                              const double *cmd, int cap, const int32_t *n_flown, int stride, double cmd_hz,
                              const double *weights3, double *audit, int32_t *count, int32_t *flags) {
  int rc = fleet_audit_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, audit, count, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  MapRef maps;
  rc = fleet_maps(c, scene_id, scene_ids, maps);
  if (rc) return rc;
  if (list.n == 0) return NEO_OK;
  FleetAuditArgs aa{cmd, cap, n_flown, stride, cmd_hz, {1.0, 1.0, 100.0}, audit, count, flags};
  if (weights3)
    for (int k = 0; k < 3; ++k) aa.w[k] = weights3[k];
  return launched(c, fleet_audit(c, list, maps, aa));
}

int neo_fleet_audit_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const int32_t *subset, int n_subset,
                          const double *cmd, int cap, const int32_t *n_flown, int stride, double cmd_hz,
                          const double *weights3, double *audit, int32_t *count, int32_t *flags) {
  int rc = fleet_audit_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, audit, count, flags);
  if (rc) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  std::vector<int> slots;
  if (scene_ids) {
    rc = scene_slots(c, scene_ids, bs, false, slots);
    if (rc) return rc;
  }
  HostStage st(c, 0);
  const auto fc = st.in(cmd, bs * cap * 6);
  const auto fnf = st.in(n_flown, bs);
  const auto fs = st.in(scene_ids ? slots.data() : nullptr, bs);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fa = st.inout(audit, bs * NEO_AUDIT_FIELDS);  // (missions outside the subset keep their records)
  const auto fcnt = st.inout(count, bs), ffl = st.inout(flags, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_fleet_audit_batch_dev(c, scene_ids ? scene_ids[0] : scene_id, scene_ids ? st.dev(fs) : nullptr, B,
                                 st.dev(fsub), n_subset, st.dev(fc), cap, st.dev(fnf), stride, cmd_hz,
                                 weights3, st.dev(fa), st.dev(fcnt), st.dev(ffl));
  if (rc) return rc;
  return st.download();
}

// ---- fleet goal routes (ros_node/tracker_planner_node.py; kernels: neo_track.hpp)
static int fleet_routes_check(neo_ctx *c, const char *who, const double *vertices, int n_vertices,
                              const int32_t *route_begin, const double *speed) {
  if (!vertices || !route_begin || !speed)
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": null buffer").c_str());
  if (n_vertices < 0) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": n_vertices must be >= 0").c_str());
  return NEO_OK;
}

static int fleet_goal_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *vertices, int n_vertices,
                            const int32_t *route_begin, const double *speed, double t, const double *goal) {
  int rc = list_check(c, "fleet goal", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_routes_check(c, "fleet goal", vertices, n_vertices, route_begin, speed);
  if (rc) return rc;
  if (!goal) return fail_locked(c, NEO_ERR_INVALID, "fleet goal: null buffer");
  if (!std::isfinite(t)) return fail_locked(c, NEO_ERR_INVALID, "fleet goal: t must be finite");
  return NEO_OK;
}

int neo_fleet_goal_route_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *vertices, int n_vertices,
                             const int32_t *route_begin, const double *speed, const int32_t *closed, double t,
                             double *goal) {
  int rc = fleet_goal_check(c, B, subset, n_subset, vertices, n_vertices, route_begin, speed, t, goal);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_goal(c, list, {vertices, n_vertices, route_begin, speed, closed}, t, goal));
}

int neo_fleet_goal_route(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *vertices, int n_vertices,
                         const int32_t *route_begin, const double *speed, const int32_t *closed, double t, double *goal) {
  int rc = fleet_goal_check(c, B, subset, n_subset, vertices, n_vertices, route_begin, speed, t, goal);
  if (rc) return rc;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  // the rows go up too: missions outside the subset keep theirs
  HostStage st(c, kStagedUpTo);
  const auto fv = st.in(vertices, (size_t)n_vertices * 2, 2), fs = st.in(speed, bs);
  const auto fb = st.in(route_begin, bs + 1);
  const auto fc = st.in_optional(closed, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fg = st.inout(goal, bs * 2);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_fleet_goal_route_dev(c, B, st.dev(fsub), n_subset, st.dev(fv), n_vertices, st.dev(fb), st.dev(fs), st.dev(fc), t,
                                st.dev(fg));
  if (rc) return rc;
  return st.download();
}

int neo_fleet_hold_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, double *cmd, int cap, int32_t *cmd_len,
                       const int32_t *cmd_index, int step, int32_t *flags) {
  int rc = list_check(c, "fleet hold", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!cmd || !cmd_len || !cmd_index || !flags) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: null buffer");
  if (cap < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: cap must be >= 1");
  if (step < 1 || step > (1 << 30)) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: step must be in 1 .. 2^30");
  if (reinterpret_cast<uintptr_t>(cmd) & 15) return fail_locked(c, NEO_ERR_INVALID, "fleet hold: cmd must be 16-byte aligned");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_hold(c, list, {cmd, cap, cmd_len, const_cast<int32_t *>(cmd_index), nullptr}, step, flags));
}

static int fleet_track_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                             const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                             const int32_t *route_begin, const double *speed, double radius, const double *track,
                             const int32_t *count, const int32_t *flags) {
  int rc = list_check(c, "fleet track audit", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = fleet_routes_check(c, "fleet track audit", vertices, n_vertices, route_begin, speed);
  if (rc) return rc;
  if (!cmd || !n_flown || !track || !count || !flags) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: null buffer");
  if (cap < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: cap must be >= 1");
  if (stride < 1) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: stride must be >= 1");
  if (!fleet_positive(cmd_hz)) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: cmd_hz must be finite and > 0");
  if (!std::isfinite(radius)) return fail_locked(c, NEO_ERR_INVALID, "fleet track audit: radius must be finite");
  return NEO_OK;
}

int neo_fleet_track_audit_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                              const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                              const int32_t *route_begin, const double *speed, const int32_t *closed, double radius,
                              double *track, int32_t *count, int32_t *flags) {
  int rc = fleet_track_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, vertices, n_vertices, route_begin,
                             speed, radius, track, count, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fleet_track_audit(c, list, {vertices, n_vertices, route_begin, speed, closed},
                                       {cmd, cap, n_flown, stride, cmd_hz, radius, track, count, flags}));
}

int neo_fleet_track_audit(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                          const int32_t *n_flown, int stride, double cmd_hz, const double *vertices, int n_vertices,
                          const int32_t *route_begin, const double *speed, const int32_t *closed, double radius,
                          double *track, int32_t *count, int32_t *flags) {
  int rc = fleet_track_check(c, B, subset, n_subset, cmd, cap, n_flown, stride, cmd_hz, vertices, n_vertices, route_begin,
                             speed, radius, track, count, flags);
  if (rc) return rc;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t bs = (size_t)B;
  HostStage st(c, 0);
  const auto fc = st.in(cmd, bs * cap * 6);
  const auto fnf = st.in(n_flown, bs);
  const auto fv = st.in(vertices, (size_t)n_vertices * 2, 2), fs = st.in(speed, bs);
  const auto fb = st.in(route_begin, bs + 1);
  const auto fcl = st.in_optional(closed, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto ft = st.inout(track, bs * NEO_TRACK_FIELDS);  // (missions outside the subset keep their records)
  const auto fcnt = st.inout(count, bs), ffl = st.inout(flags, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_fleet_track_audit_dev(c, B, st.dev(fsub), n_subset, st.dev(fc), cap, st.dev(fnf), stride, cmd_hz, st.dev(fv),
                                 n_vertices, st.dev(fb), st.dev(fs), st.dev(fcl), radius, st.dev(ft), st.dev(fcnt),
                                 st.dev(ffl));
  if (rc) return rc;
  return st.download();
}

// ---- the fleet's record mode (traj_planner/record_planner.py:13-72; kernels: neo_record.hpp)
int neo_record_state_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *cmd, int cap,
                         const int32_t *cmd_len, const int32_t *cmd_index, const double *head, double *cur_vel) {
  int rc = list_check(c, "record", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!cmd || !cmd_len || !cmd_index || !head || !cur_vel) return fail_locked(c, NEO_ERR_INVALID, "record state: null buffer");
  if (cap <= 0) return fail_locked(c, NEO_ERR_INVALID, "record state: cap must be > 0");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, record_state(c, list, cmd, cap, cmd_len, cmd_index, head, cur_vel));
}

int neo_record_commit_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, const double *x, const double *head,
                          const double *tail, const int32_t *solved, const double *pose, const double *cur_vel,
                          const uint8_t *staging, int width, int height, const int32_t *mission_ids, int tick, int round,
                          int capacity, double *motion, double *wpts_local, double *tau, double *pose_rows, int32_t *meta,
                          uint8_t *images, int32_t *row_of, int32_t *n_rows, int32_t *dropped) {
  int rc = list_check(c, "record", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (M < 2 || M > NEO_MAX_PIECES) return fail_locked(c, NEO_ERR_INVALID, "record commit: M must be in 2 .. 64");
  if (capacity < 1) return fail_locked(c, NEO_ERR_INVALID, "record commit: capacity must be >= 1");
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    return fail_locked(c, NEO_ERR_INVALID, "record commit: width and height must be in 1 .. 4096");
  if (!x || !head || !tail || !pose || !cur_vel || !staging || !motion || !wpts_local || !tau || !pose_rows || !meta ||
      !images || !row_of || !n_rows || !dropped)
    return fail_locked(c, NEO_ERR_INVALID, "record commit: null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, record_commit(c, list, RecordCommitArgs{M, x, head, tail, solved, pose, cur_vel, staging, width, height,
                                                             mission_ids, tick, round, capacity, motion, wpts_local, tau,
                                                             pose_rows, meta, images, row_of, n_rows, dropped}));
}

// ---- the learned warm start on resident arrays (traj_planner/neo_planner.py:10-51; kernels: neo_init.hpp)
int neo_init_motion_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const double *pose, const double *cur_vel,
                        const double *head, const double *tail, float *motion) {
  int rc = list_check(c, "init motion", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!pose || !cur_vel || !head || !tail || !motion) return fail_locked(c, NEO_ERR_INVALID, "init motion: null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, init_motion(c, list, pose, cur_vel, head, tail, motion));
}

int neo_init_head_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *weights, size_t n_weights,
                      const float *feature, int feature_rows, const float *motion, float *out) {
  int rc = list_check(c, "init head", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!weights || !feature || !motion || !out) return fail_locked(c, NEO_ERR_INVALID, "init head: null buffer");
  if (n_weights != (size_t)NEO_INIT_HEAD_FLOATS)
    return fail_locked(c, NEO_ERR_INVALID, "init head: n_weights must be NEO_INIT_HEAD_FLOATS (20817)");
  if (feature_rows != 1 && feature_rows != B)
    return fail_locked(c, NEO_ERR_INVALID, "init head: feature_rows must be 1 or B");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, init_head(c, list, weights, feature, feature_rows, motion, out));
}

int neo_init_guess_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const float *out, const double *pose,
                       double *x0) {
  int rc = list_check(c, "init guess", B, 1, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (!out || !pose || !x0) return fail_locked(c, NEO_ERR_INVALID, "init guess: null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, init_guess(c, list, out, pose, x0));
}

// ---- the `batch` planner mode on resident arrays (traj_planner/expert_planner.py:103-168; kernels: neo_batch.hpp)
static const double kBatchOffset = 0.6;  // :135
static int batch_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M, int D, int K) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  if (D != 2) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": D must be 2 (the reference's lateral candidates are 2-D)").c_str());
  if (K < 1 || K > NEO_BATCH_MAX_CANDIDATES)
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": K must be in 1 .. 8").c_str());
  rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (M < 2) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": M must be >= 2 (at least one waypoint)").c_str());
  if ((long long)launch_list(B, subset, n_subset).n * K > (long long)INT32_MAX)
    return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": more than 2^31 - 1 candidate rows").c_str());
  return NEO_OK;
}
// the reference's offsets 0, +0.6, -0.6, +0.6, ... (lateral_dir[(k - 1) % 2], :131-137)
static void batch_default_offsets(int K, double *off) {
  for (int k = 0; k < K; ++k) off[k] = k == 0 ? 0.0 : (k % 2 ? kBatchOffset : -kBatchOffset);
}

int neo_batch_candidates_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *head,
                             const double *tail, const int32_t *slots, const double *tau, const double *lateral_offsets,
                             double *x0, double *head_k, double *tail_k, int32_t *slots_k) {
  int rc = batch_check(c, "batch candidates", B, subset, n_subset, M, D, K);
  if (rc) return rc;
  if (!head || !tail || !tau || !x0 || !head_k || !tail_k)
    return fail_locked(c, NEO_ERR_INVALID, "batch candidates: null buffer");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  double off[NEO_BATCH_MAX_CANDIDATES];
  batch_default_offsets(K, off);
  if (lateral_offsets)
    for (int k = 0; k < K; ++k) off[k] = lateral_offsets[k];
  return launched(c, batch_candidates(c, list, {M, K, head, tail, slots, tau, off, x0, head_k, tail_k, slots_k}));
}

int neo_batch_candidates(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *head,
                         const double *tail, const int32_t *slots, const double *tau, const double *lateral_offsets,
                         double *x0, double *head_k, double *tail_k, int32_t *slots_k) {
  int rc = batch_check(c, "batch candidates", B, subset, n_subset, M, D, K);
  if (rc) return rc;
  if (!head || !tail || !tau || !x0 || !head_k || !tail_k)
    return fail_locked(c, NEO_ERR_INVALID, "batch candidates: null buffer");
  const size_t bs = (size_t)B, rows = (size_t)launch_list(B, subset, n_subset).n * K, n = (size_t)D * (M - 1) + M;
  if (rows == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the packed outputs go up too: the rows of a skipped index come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * 6), ft = st.in(tail, bs * 6);
  const auto fs = st.in_optional(slots, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fx = st.inout(x0, rows * n), fhk = st.inout(head_k, rows * 6), ftk = st.inout(tail_k, rows * 6);
  const auto fsk = st.inout_optional(slots_k, rows);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_batch_candidates_dev(c, B, st.dev(fsub), n_subset, M, D, K, st.dev(fh), st.dev(ft), st.dev(fs), tau,
                                lateral_offsets, st.dev(fx), st.dev(fhk), st.dev(ftk), st.dev(fsk));
  if (rc) return rc;
  return st.download();
}

static int batch_select_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const BatchSelectArgs &a) {
  int rc = batch_check(c, "batch select", B, subset, n_subset, M, D, a.K);
  if (rc) return rc;
  const RunRowsIn &k = a.packed;
  const RunRows &o = a.out;
  if (!k.x || !k.costs4 || !k.costs4_last || !k.nit || !k.status || !a.chosen || !a.cand_cost || !a.solved || !o.x ||
      !o.costs4 || !o.costs4_last || !o.status || !a.nit_total || !a.opt_runs || !a.fallback || !a.n_fallback)
    return fail_locked(c, NEO_ERR_INVALID, "batch select: null buffer");
  if (o.nfev && !k.nfev) return fail_locked(c, NEO_ERR_INVALID, "batch select: nfev without nfev_k");
  return NEO_OK;
}

int neo_batch_select_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *x_k,
                         const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                         const int32_t *status_k, const double *weights4, int32_t *chosen, double *cand_cost,
                         int32_t *solved, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                         int32_t *status, int32_t *nit_total, int32_t *opt_runs, int32_t *fallback, int32_t *n_fallback) {
  BatchSelectArgs a{D * (M - 1) + M, K, {x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k}, weights4, chosen, cand_cost,
                    solved, {x, costs4, costs4_last, nit, nfev, status}, nit_total, opt_runs, fallback, n_fallback};
  int rc = batch_select_check(c, B, subset, n_subset, M, D, a);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) {
    HIPCHK(c, hipMemsetAsync(n_fallback, 0, sizeof(int32_t), c->stream));
    return NEO_OK;
  }
  if (!a.w) a.w = c->params.weights;
  return launched(c, batch_select(c, list, a));
}

int neo_batch_select(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int K, const double *x_k,
                     const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                     const int32_t *status_k, const double *weights4, int32_t *chosen, double *cand_cost, int32_t *solved,
                     double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status,
                     int32_t *nit_total, int32_t *opt_runs, int32_t *fallback, int32_t *n_fallback) {
  const BatchSelectArgs a{D * (M - 1) + M, K, {x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k}, weights4, chosen,
                          cand_cost, solved, {x, costs4, costs4_last, nit, nfev, status}, nit_total, opt_runs, fallback,
                          n_fallback};
  int rc = batch_select_check(c, B, subset, n_subset, M, D, a);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) {
    *n_fallback = 0;
    return NEO_OK;
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the request-indexed outputs go up too: requests outside the subset, and x of a request without a choice, stay
  HostStage st(c, kStagedUpTo);
  const RowRefs fk = stage_rows_in(st, a.packed, P * K, (size_t)a.n);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto och = st.inout(chosen, bs);
  const auto occ = st.inout(cand_cost, bs * K);
  const auto oso = st.inout(solved, bs);
  const RowRefs fo = stage_rows_inout(st, a.out, bs, (size_t)a.n);
  const auto ont = st.inout(nit_total, bs), oru = st.inout(opt_runs, bs);
  // (the whole list comes back; its entries from n_fallback on are scratch)
  const auto ofb = st.out(fallback, P), onb = st.out(n_fallback, 1);
  rc = st.upload();
  if (rc) return rc;
  const RunRowsIn k = as_const(staged_rows(st, fk));
  const RunRows o = staged_rows(st, fo);
  rc = neo_batch_select_dev(c, B, st.dev(fsub), n_subset, M, D, K, k.x, k.costs4, k.costs4_last, k.nit, k.nfev, k.status,
                            weights4, st.dev(och), st.dev(occ), st.dev(oso), o.x, o.costs4, o.costs4_last, o.nit, o.nfev,
                            o.status, st.dev(ont), st.dev(oru), st.dev(ofb), st.dev(onb));
  if (rc) return rc;
  return st.download();
}

// ---- BatchPlanner.plan's retry chain on resident arrays (traj_planner/expert_planner.py:186-203; kernels: neo_plan.hpp)
static int plan_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M, int D) {
  int rc = list_check(c, "fleet", B, 0, INT32_MAX, subset, n_subset);
  if (rc) return rc;
  rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (M < 2) return fail_locked(c, NEO_ERR_INVALID, (std::string(who) + ": M must be >= 2 (at least one waypoint)").c_str());
  return NEO_OK;
}

static int plan_guess_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const void *head,
                            const void *tail, const void *x_init, const void *frac, const void *tau, const void *x0,
                            const void *head_k, const void *tail_k) {
  int rc = plan_check(c, "plan guess", B, subset, n_subset, M, D);
  if (rc) return rc;
  if (!head || !tail || !x0 || !head_k || !tail_k) return fail_locked(c, NEO_ERR_INVALID, "plan guess: null buffer");
  if (!x_init && (!frac || !tau)) return fail_locked(c, NEO_ERR_INVALID, "plan guess: frac and tau are needed without x_init");
  return NEO_OK;
}

int neo_plan_guess_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const double *head,
                       const double *tail, const int32_t *slots, const double *x_init, const double *noise,
                       const double *frac, const double *tau, double *x0, double *head_k, double *tail_k,
                       int32_t *slots_k) {
  int rc = plan_guess_check(c, B, subset, n_subset, M, D, head, tail, x_init, frac, tau, x0, head_k, tail_k);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, plan_guess(c, list, D, {M, head, tail, slots, x_init, noise, frac, tau, x0, head_k, tail_k, slots_k}));
}

int neo_plan_guess(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, const double *head,
                   const double *tail, const int32_t *slots, const double *x_init, const double *noise, const double *frac,
                   const double *tau, double *x0, double *head_k, double *tail_k, int32_t *slots_k) {
  int rc = plan_guess_check(c, B, subset, n_subset, M, D, head, tail, x_init, frac, tau, x0, head_k, tail_k);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n, n = (size_t)D * (M - 1) + M, hd = (size_t)3 * D;
  if (P == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the packed outputs go up too: the rows of a skipped index come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * hd), ft = st.in(tail, bs * hd);
  const auto fs = st.in_optional(slots, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fxi = st.in_optional(x_init, bs * n), fno = st.in_optional(noise, P * (size_t)D * (M - 1));
  const auto fx = st.inout(x0, P * n), fhk = st.inout(head_k, P * hd), ftk = st.inout(tail_k, P * hd);
  const auto fsk = st.inout_optional(slots_k, P);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_plan_guess_dev(c, B, st.dev(fsub), n_subset, M, D, st.dev(fh), st.dev(ft), st.dev(fs), st.dev(fxi), st.dev(fno),
                          frac, tau, st.dev(fx), st.dev(fhk), st.dev(ftk), st.dev(fsk));
  if (rc) return rc;
  return st.download();
}

static int plan_jitter_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int attempt,
                             const double *noise) {
  int rc = plan_check(c, "plan jitter", B, subset, n_subset, M, D);
  if (rc) return rc;
  if (!noise) return fail_locked(c, NEO_ERR_INVALID, "plan jitter: null buffer");
  if (attempt < 0) return fail_locked(c, NEO_ERR_INVALID, "plan jitter: attempt must be >= 0");
  return NEO_OK;
}

int neo_plan_jitter_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, uint64_t seed, int attempt,
                        const int32_t *stream_ids, double *noise) {
  int rc = plan_jitter_check(c, B, subset, n_subset, M, D, attempt, noise);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, plan_jitter(c, list, M, D, seed, attempt, stream_ids, noise));
}

int neo_plan_jitter(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, uint64_t seed, int attempt,
                    const int32_t *stream_ids, double *noise) {
  int rc = plan_jitter_check(c, B, subset, n_subset, M, D, attempt, noise);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the packed rows go up too: the rows of a skipped index come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fi = st.in_optional(stream_ids, bs), fsub = st.in_optional(subset, (size_t)n_subset);
  const auto fno = st.inout(noise, P * (size_t)D * (M - 1));
  rc = st.upload();
  if (rc) return rc;
  rc = neo_plan_jitter_dev(c, B, st.dev(fsub), n_subset, M, D, seed, attempt, st.dev(fi), st.dev(fno));
  if (rc) return rc;
  return st.download();
}

// the arrays of the three merge entry points as the launcher takes them (x in rows of n), their one check -- `compacts`:
// n_failed is needed -- and the body of the two device ones: the merge, then with n_failed the compaction
static PlanMergeArgs plan_merge_args(int M, int D, int reset, const double *x_k, const double *costs4_k, const double *costs4_last_k,
                                     const int32_t *nit_k, const int32_t *nfev_k, const int32_t *status_k, double *x, double *costs4,
                                     double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status, int32_t *attempts,
                                     int64_t *nit_total, int32_t *solved, int32_t *failed, int32_t *n_failed, int32_t *bad_scene) {
  static_assert(sizeof(long long) == sizeof(int64_t), "nit_total is a 64-bit integer on both sides");
  const int n = D * (M - 1) + M;
  return {n, n, reset ? 1 : 0, {x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k}, {x, costs4, costs4_last, nit, nfev, status},
          attempts, reinterpret_cast<long long *>(nit_total), solved, failed, n_failed, bad_scene};
}

static int plan_merge_check(neo_ctx *c, const std::string &who, int B, const int32_t *subset, int n_subset, int M, int D,
                            const PlanMergeArgs &a, bool compacts) {
  int rc = plan_check(c, who.c_str(), B, subset, n_subset, M, D);
  if (rc) return rc;
  if (a.ldx < a.n) return fail_locked(c, NEO_ERR_INVALID, (who + ": x_stride must be >= n = D (M - 1) + M").c_str());
  const RunRowsIn &k = a.packed;
  const RunRows &o = a.out;
  if (!k.x || !k.costs4 || !k.costs4_last || !k.nit || !k.nfev || !k.status || !o.x || !o.costs4 || !o.costs4_last || !o.nit ||
      !o.nfev || !o.status || !a.attempts || !a.nit_total || !a.solved || !a.failed || !a.bad_scene || (compacts && !a.n_failed))
    return fail_locked(c, NEO_ERR_INVALID, (who + ": null buffer").c_str());
  return NEO_OK;
}

static int plan_merge_dev(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset, int M, int D,
                          const PlanMergeArgs &a, bool compacts, bool clear_bad) {
  if (int rc = plan_merge_check(c, who, B, subset, n_subset, M, D, a, compacts)) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (clear_bad) HIPCHK(c, hipMemsetAsync(a.bad_scene, 0, sizeof(int32_t), c->stream));
  if (list.n > 0) return launched(c, plan_merge(c, list, a));
  if (compacts) HIPCHK(c, hipMemsetAsync(a.n_failed, 0, sizeof(int32_t), c->stream));
  return NEO_OK;
}

int neo_plan_merge_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int reset, const double *x_k,
                       const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                       const int32_t *status_k, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                       int32_t *status, int32_t *attempts, int64_t *nit_total, int32_t *solved, int32_t *failed,
                       int32_t *n_failed, int32_t *bad_scene) {
  const PlanMergeArgs a = plan_merge_args(M, D, reset, x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k, x, costs4, costs4_last,
                                          nit, nfev, status, attempts, nit_total, solved, failed, n_failed, bad_scene);
  return plan_merge_dev(c, "plan merge", B, subset, n_subset, M, D, a, true, true);
}

int neo_plan_merge(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int reset, const double *x_k,
                   const double *costs4_k, const double *costs4_last_k, const int32_t *nit_k, const int32_t *nfev_k,
                   const int32_t *status_k, double *x, double *costs4, double *costs4_last, int32_t *nit, int32_t *nfev,
                   int32_t *status, int32_t *attempts, int64_t *nit_total, int32_t *solved, int32_t *failed,
                   int32_t *n_failed, int32_t *bad_scene) {
  const PlanMergeArgs a = plan_merge_args(M, D, reset, x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k, x, costs4, costs4_last,
                                          nit, nfev, status, attempts, nit_total, solved, failed, n_failed, bad_scene);
  int rc = plan_merge_check(c, "plan merge", B, subset, n_subset, M, D, a, true);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) {
    *n_failed = 0;
    *bad_scene = 0;
    return NEO_OK;
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the request-indexed arrays go up too: requests outside the subset stay, attempts and nit_total accumulate
  HostStage st(c, kStagedUpTo);
  const RowRefs fk = stage_rows_in(st, a.packed, P, (size_t)a.n);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const RowRefs fo = stage_rows_inout(st, a.out, bs, (size_t)a.n);
  const auto oat = st.inout(attempts, bs);
  const auto ont = st.inout(nit_total, bs);
  const auto oso = st.inout(solved, bs);
  // (the whole list comes back; its entries from n_failed on are scratch)
  const auto ofl = st.out(failed, P), onl = st.out(n_failed, 1), obs = st.out(bad_scene, 1);
  rc = st.upload();
  if (rc) return rc;
  const RunRowsIn k = as_const(staged_rows(st, fk));
  const RunRows o = staged_rows(st, fo);
  rc = neo_plan_merge_dev(c, B, st.dev(fsub), n_subset, M, D, reset, k.x, k.costs4, k.costs4_last, k.nit, k.nfev, k.status, o.x,
                          o.costs4, o.costs4_last, o.nit, o.nfev, o.status, st.dev(oat), st.dev(ont), st.dev(oso), st.dev(ofl),
                          st.dev(onl), st.dev(obs));
  if (rc) return rc;
  return st.download();
}

// ---- adaptive waypoint counts and the plan chain over groups of one count (expert_planner.py:86-88; kernels:
// neo_adaptive.hpp)
static int adaptive_list_check(neo_ctx *c, const char *who, int B, const int32_t *subset, int n_subset) {
  return list_check(c, who, B, 1, INT32_MAX, subset, n_subset);
}

static int adaptive_count_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, int D, const double *head,
                                const double *tail, double seg_len, int max_waypoints, const int32_t *counts,
                                const int32_t *clamped) {
  int rc = adaptive_list_check(c, "adaptive count", B, subset, n_subset);
  if (rc) return rc;
  if (D < 2 || D > NEO_MAX_DIM) return fail_locked(c, NEO_ERR_INVALID, "adaptive count: D must be 2 or 3");
  if (max_waypoints < 1 || max_waypoints > NEO_MAX_PIECES - 1)
    return fail_locked(c, NEO_ERR_INVALID, "adaptive count: max_waypoints must be in 1 .. NEO_MAX_PIECES - 1");
  if (!std::isfinite(seg_len) || !(seg_len > 0.0))
    return fail_locked(c, NEO_ERR_INVALID, "adaptive count: seg_len must be finite and > 0");
  if (!head || !tail || !counts || !clamped) return fail_locked(c, NEO_ERR_INVALID, "adaptive count: null buffer");
  return NEO_OK;
}

int neo_adaptive_count_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int D, const double *head,
                           const double *tail, double seg_len, int max_waypoints, int32_t *counts, int32_t *clamped) {
  int rc = adaptive_count_check(c, B, subset, n_subset, D, head, tail, seg_len, max_waypoints, counts, clamped);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, adaptive_count(c, list, D, head, tail, seg_len, max_waypoints, counts, clamped));
}

int neo_adaptive_count(neo_ctx *c, int B, const int32_t *subset, int n_subset, int D, const double *head,
                       const double *tail, double seg_len, int max_waypoints, int32_t *counts, int32_t *clamped) {
  int rc = adaptive_count_check(c, B, subset, n_subset, D, head, tail, seg_len, max_waypoints, counts, clamped);
  if (rc) return rc;
  const size_t bs = (size_t)B, hd = (size_t)3 * D;
  if (launch_list(B, subset, n_subset).n == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the results go up too: the rows of requests not launched come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * hd), ft = st.in(tail, bs * hd);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto oc = st.inout(counts, bs), ocl = st.inout(clamped, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_adaptive_count_dev(c, B, st.dev(fsub), n_subset, D, st.dev(fh), st.dev(ft), seg_len, max_waypoints, st.dev(oc),
                              st.dev(ocl));
  if (rc) return rc;
  return st.download();
}

static int adaptive_bucket_check(neo_ctx *c, int B, const int32_t *subset, int n_subset, const int32_t *counts,
                                 const int32_t *order, const int32_t *bucket_begin, const int32_t *total) {
  int rc = adaptive_list_check(c, "adaptive bucket", B, subset, n_subset);
  if (rc) return rc;
  if (!counts || !order || !bucket_begin || !total) return fail_locked(c, NEO_ERR_INVALID, "adaptive bucket: null buffer");
  if (subset && order == subset) return fail_locked(c, NEO_ERR_INVALID, "adaptive bucket: order must not be the subset");
  return NEO_OK;
}

int neo_adaptive_bucket_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, const int32_t *counts, int32_t *order,
                            int32_t *bucket_begin, int32_t *total) {
  int rc = adaptive_bucket_check(c, B, subset, n_subset, counts, order, bucket_begin, total);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) {
    HIPCHK(c, hipMemsetAsync(bucket_begin, 0, (NEO_MAX_PIECES + 1) * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(total, 0, sizeof(int32_t), c->stream));
    return NEO_OK;
  }
  return launched(c, adaptive_bucket(c, list, counts, order, bucket_begin, total));
}

int neo_adaptive_bucket(neo_ctx *c, int B, const int32_t *subset, int n_subset, const int32_t *counts, int32_t *order,
                        int32_t *bucket_begin, int32_t *total) {
  int rc = adaptive_bucket_check(c, B, subset, n_subset, counts, order, bucket_begin, total);
  if (rc) return rc;
  const size_t bs = (size_t)B, P = (size_t)launch_list(B, subset, n_subset).n;
  if (P == 0) {
    std::memset(bucket_begin, 0, (NEO_MAX_PIECES + 1) * sizeof(int32_t));
    *total = 0;
    return NEO_OK;
  }
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  // the order goes up too: its entries from total on come back as they were
  HostStage st(c, kStagedUpTo);
  const auto fc = st.in(counts, bs);
  const auto fsub = st.in_optional(subset, (size_t)n_subset);
  const auto oo = st.inout(order, P);
  const auto ob = st.out(bucket_begin, (size_t)NEO_MAX_PIECES + 1), ot = st.out(total, 1);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_adaptive_bucket_dev(c, B, st.dev(fsub), n_subset, st.dev(fc), st.dev(oo), st.dev(ob), st.dev(ot));
  if (rc) return rc;
  return st.download();
}

int neo_adaptive_merge_dev(neo_ctx *c, int B, const int32_t *subset, int n_subset, int M, int D, int x_stride, int reset,
                           int clear_bad, const double *x_k, const double *costs4_k, const double *costs4_last_k,
                           const int32_t *nit_k, const int32_t *nfev_k, const int32_t *status_k, double *x, double *costs4,
                           double *costs4_last, int32_t *nit, int32_t *nfev, int32_t *status, int32_t *attempts,
                           int64_t *nit_total, int32_t *solved, int32_t *pending, int32_t *bad_scene) {
  if (int rc = adaptive_list_check(c, "adaptive merge", B, subset, n_subset)) return rc;
  PlanMergeArgs a = plan_merge_args(M, D, reset, x_k, costs4_k, costs4_last_k, nit_k, nfev_k, status_k, x, costs4, costs4_last,
                                    nit, nfev, status, attempts, nit_total, solved, pending, nullptr, bad_scene);
  a.ldx = x_stride;
  return plan_merge_dev(c, "adaptive merge", B, subset, n_subset, M, D, a, false, clear_bad != 0);
}

static int adaptive_compact_check(neo_ctx *c, const int32_t *seg_begin, const int32_t *seg_len, long long rows,
                                  const int32_t *pending, const int32_t *n_failed) {
  if (!c) return NEO_ERR_INVALID;
  if (!seg_begin || !seg_len || !pending || !n_failed) return fail_locked(c, NEO_ERR_INVALID, "adaptive compact: null buffer");
  for (int g = 0; g < NEO_MAX_PIECES; ++g)
    if (seg_begin[g] < 0 || seg_len[g] < 0 || (rows >= 0 && (long long)seg_begin[g] + seg_len[g] > rows))
      return fail_locked(c, NEO_ERR_INVALID, "adaptive compact: a segment is negative or ends beyond pending");
  return NEO_OK;
}

int neo_adaptive_compact_dev(neo_ctx *c, const int32_t *seg_begin, const int32_t *seg_len, int32_t *pending,
                             int32_t *n_failed) {
  int rc = adaptive_compact_check(c, seg_begin, seg_len, -1, pending, n_failed);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  return launched(c, adaptive_compact(c, seg_begin, seg_len, pending, n_failed));
}

int neo_adaptive_compact(neo_ctx *c, const int32_t *seg_begin, const int32_t *seg_len, int rows, int32_t *pending,
                         int32_t *n_failed) {
  if (c && rows < 0) return fail_locked(c, NEO_ERR_INVALID, "adaptive compact: rows must be >= 0");
  int rc = adaptive_compact_check(c, seg_begin, seg_len, rows, pending, n_failed);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  HostStage st(c, kStagedUpTo);
  const auto fp = st.inout(pending, (size_t)rows);
  const auto on = st.out(n_failed, (size_t)NEO_MAX_PIECES);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_adaptive_compact_dev(c, seg_begin, seg_len, st.dev(fp), st.dev(on));
  if (rc) return rc;
  return st.download();
}

// ---- geo warm start (traj_planner/astar_planner.py, geo_planner.py:19-101; kernels: neo_geo.hpp)
static int geo_check(neo_ctx *c, int B, const double *start, const double *target, int max_expansions, int path_cap,
                     const double *key_pts, const double *path, const int32_t *path_len, const double *path_cost,
                     const int32_t *expansions, const int32_t *flags) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 1) return fail_locked(c, NEO_ERR_INVALID, "geo: B must be >= 1");
  if (max_expansions < 0 || path_cap < 0 || (path && path_cap < 1))
    return fail_locked(c, NEO_ERR_INVALID, "geo: max_expansions and path_cap must be >= 0 (path_cap >= 1 with a path)");
  if (!start || !target || !key_pts || !path_len || !path_cost || !expansions || !flags)
    return fail_locked(c, NEO_ERR_INVALID, "geo: null buffer");
  return NEO_OK;
}

// the reference scene of a call: it must exist and be 2-D (the reference's A* is 2-D only)
static int geo_scene_kind(neo_ctx *c, int scene_id) {
  auto it = c->maps.find(scene_id);
  if (it == c->maps.end()) return fail(c, NEO_ERR_NO_MAP, "geo: no ESDF for this scene");
  if (it->second.kind != 0) return fail(c, NEO_ERR_UNSUPPORTED, "geo: the A* warm start needs a 2-D map");
  return NEO_OK;
}

int neo_geo_search_batch_dev(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const double *start,
                             const double *target, int max_expansions, int path_cap, double *key_pts, double *path,
                             int32_t *path_len, double *path_cost, int32_t *expansions, int32_t *flags) {
  int rc = geo_check(c, B, start, target, max_expansions, path_cap, key_pts, path, path_len, path_cost, expansions, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  rc = rebuild_tables(c);
  if (rc) return rc;
  rc = geo_scene_kind(c, scene_id);
  if (rc) return rc;
  const GeoArgs ga{B, scene_ids, start, target, max_expansions, path ? path_cap : 0, key_pts, path, path_cost,
                   path_len, expansions, flags};
  return geo_search(c, scene_id, ga);
}

int neo_geo_search_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const double *start,
                         const double *target, int max_expansions, int path_cap, double *key_pts, double *path,
                         int32_t *path_len, double *path_cost, int32_t *expansions, int32_t *flags) {
  int rc = geo_check(c, B, start, target, max_expansions, path_cap, key_pts, path, path_len, path_cost, expansions, flags);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  rc = rebuild_tables(c);
  if (rc) return rc;
  const size_t bs = (size_t)B, pc = path ? (size_t)path_cap : 0;
  std::vector<int> slots;
  rc = scene_ids ? scene_slots(c, scene_ids, bs, true, slots) : geo_scene_kind(c, scene_id);
  if (rc) return rc;
  HostStage st(c, 0);
  const auto fs = st.in(start, 2 * bs), ft = st.in(target, 2 * bs);
  const auto fsl = st.in(scene_ids ? slots.data() : nullptr, bs);
  const auto fk = st.out(key_pts, 8 * bs), fc = st.out(path_cost, bs), fp = st.out(path, 2 * bs * pc);
  const auto fl = st.out(path_len, bs), fe = st.out(expansions, bs), ff = st.out(flags, bs);
  rc = st.upload();
  if (rc) return rc;
  rc = neo_geo_search_batch_dev(c, scene_ids ? scene_ids[0] : scene_id, scene_ids ? st.dev(fsl) : nullptr, B, st.dev(fs),
                                st.dev(ft), max_expansions, path_cap, st.dev(fk), path ? st.dev(fp) : nullptr, st.dev(fl),
                                st.dev(fc), st.dev(fe), st.dev(ff));
  if (rc) return rc;
  return st.download();
}

int neo_geo_prune_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const double *paths,
                        const int32_t *path_len, int path_stride, double *key_pts) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 1 || path_stride < 1) return fail_locked(c, NEO_ERR_INVALID, "geo prune: B and path_stride must be >= 1");
  if (!paths || !path_len || !key_pts) return fail_locked(c, NEO_ERR_INVALID, "geo prune: null buffer");
  for (int i = 0; i < B; ++i)
    if (path_len[i] < 1 || path_len[i] > path_stride)
      return fail_locked(c, NEO_ERR_INVALID, "geo prune: path_len must be in [1, path_stride]");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc = rebuild_tables(c);
  if (rc) return rc;
  const size_t bs = (size_t)B, ps = (size_t)path_stride;
  std::vector<int> slots;
  rc = scene_ids ? scene_slots(c, scene_ids, bs, true, slots) : geo_scene_kind(c, scene_id);
  if (rc) return rc;
  HostStage st(c, 0);
  const auto fp = st.in(paths, 2 * bs * ps);
  const auto fl = st.in(path_len, bs), fsl = st.in(scene_ids ? slots.data() : nullptr, bs);
  const auto fk = st.out(key_pts, 8 * bs);
  rc = st.upload();
  if (rc) return rc;
  rc = geo_prune(c, scene_ids ? scene_ids[0] : scene_id, B, scene_ids ? st.dev(fsl) : nullptr, st.dev(fp), st.dev(fl),
                 path_stride, st.dev(fk));
  if (rc) return rc;
  return st.download();
}

int neo_geo_workspace_budget(neo_ctx *c, size_t bytes) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->geo.budget = bytes;
  return NEO_OK;
}

int neo_optimize_progress_counter(neo_ctx *c, int32_t *counter) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->progress = counter;
  return NEO_OK;
}

int neo_optimize_sample_counter(neo_ctx *c, int64_t *dev_counts) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->sample_counter = reinterpret_cast<long long *>(dev_counts);
  return NEO_OK;
}

int neo_optimize_trace(neo_ctx *c, double *dev_trace, int cap) {
  if (!c || cap < 0) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (dev_trace && cap > 0 && c->trace_xg && c->trace_cap != cap)
    return fail(c, NEO_ERR_INVALID, "neo_optimize_trace: cap differs from neo_optimize_trace_xg's");
  c->trace = (dev_trace && cap > 0) ? dev_trace : nullptr;
  if (c->trace) c->trace_cap = cap;
  if (!c->trace_xg && !c->trace) c->trace_cap = 0;
  return NEO_OK;
}

int neo_optimize_trace_xg(neo_ctx *c, double *dev_xg, int cap) {
  if (!c || cap < 0) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (dev_xg && cap > 0 && c->trace && c->trace_cap != cap)
    return fail(c, NEO_ERR_INVALID, "neo_optimize_trace_xg: cap differs from neo_optimize_trace's");
  c->trace_xg = (dev_xg && cap > 0) ? dev_xg : nullptr;
  if (c->trace_xg) c->trace_cap = cap;
  if (!c->trace_xg && !c->trace) c->trace_cap = 0;
  return NEO_OK;
}

int neo_optimize_dispatch_order(neo_ctx *c, const int32_t *dev_order, int B) {
  if (!c || B < 0) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->dispatch_order = (dev_order && B > 0) ? dev_order : nullptr;
  c->order_B = c->dispatch_order ? B : 0;
  return NEO_OK;
}

int neo_optimize_dispatch_order_host(neo_ctx *c, const int32_t *host_order, int B) {
  if (!c || B < 0) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (!host_order || B == 0) {
    c->dispatch_order = nullptr;
    c->order_B = 0;
    return NEO_OK;
  }
  if ((size_t)B > c->order_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->order_buf) hipFree(c->order_buf);
    c->order_buf = nullptr;
    c->order_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->order_buf, (size_t)B * sizeof(int)));
    c->order_cap = (size_t)B;
  }
  HIPCHK(c, hipMemcpyAsync(c->order_buf, host_order, (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the host array may go away after the call
  c->dispatch_order = c->order_buf;
  c->order_B = B;
  return NEO_OK;
}

namespace neo {
// rows [x (n) | total cost | 4 cost terms] in fp32 for the result gather (neo_planner_amd/sharding.py)
__global__ void pack_results_kernel(int B, int n, const double *__restrict__ x, const double *__restrict__ costs4, double w0, double w1,
                                    double w2, double w3, float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t row = i / (size_t)(n + 5);
  if (row >= (size_t)B) return;
  const int col = (int)(i - row * (size_t)(n + 5));
  const double *c4 = costs4 + row * 4;
  double v;
  if (col < n)
    v = x[row * (size_t)n + col];
  else if (col == n)
    v = ((c4[0] * w0 + c4[1] * w1) + c4[2] * w2) + c4[3] * w3;  // (costs * weights).sum(dim=1), left to right
  else
    v = c4[col - n - 1];
  out[i] = (float)v;
}
}  // namespace neo

int neo_pack_results_dev(neo_ctx *c, int B, int n, const double *x, const double *costs4, const double *weights4, float *out) {
  if (!c || B < 0 || n < 1) return NEO_ERR_INVALID;
  if (!x || !costs4 || !weights4 || !out) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t total = (size_t)B * (size_t)(n + 5);
  hipLaunchKernelGGL(neo::pack_results_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, B, n, x, costs4,
                     weights4[0], weights4[1], weights4[2], weights4[3], out);
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

namespace neo {
// ---- the expected-effort dispatch order on the device (round 6; host form: BatchPlanner.expected_effort_order)
// key = time slack of the initial guess, sum(T) v_max / |goal - start| (a guess that is far too slow sheds duration over many
// iterations: rank correlation 0.5 with the evaluation count at cfg2); a non-finite key -> 0 so that the keys are totally ordered
__global__ void effort_keys_kernel(int B, int M, int D, double T_min, double T_max, double v_max, const double *__restrict__ x0,
                                   const double *__restrict__ head, const double *__restrict__ tail, double *__restrict__ keys,
                                   int *__restrict__ idx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  idx[b] = b;
  const int nq = D * (M - 1), n = nq + M;
  double sum = 0.0;
  for (int p = 0; p < M; ++p) sum += (T_max - T_min) / (1.0 + exp(-x0[(size_t)b * n + nq + p])) + T_min;  // map_tau2T (:477-483)
  double d2 = 0.0;
  for (int d = 0; d < D; ++d) {
    const double e = tail[(size_t)b * 3 * D + d] - head[(size_t)b * 3 * D + d];
    d2 += e * e;
  }
  // (fmax drops a NaN distance: it must reach the key, which then is non-finite like the host's -> 0)
  const double dist = sqrt(d2);
  const double k = dist == dist ? sum * v_max / fmax(dist, 1e-9) : NAN;
  keys[b] = isfinite(k) ? k : 0.0;
}
}  // namespace neo

// The order itself: a stable descending sort of (key, index) -- rocPRIM's radix sort on the doubles (LSD radix: equal keys
// keep index order).  Round 6 first ranked by B^2 comparisons (one thread per element: 45 us at 4096 on 16 CUs; tiled over a
// 2-D grid with integer partial counts: three launches, fine at 4096, 0.6 ms at cfg3's 65 536).
static size_t effort_sort_temp_bytes(int B) {
  size_t tb = 0;
  (void)rocprim::radix_sort_pairs_desc(nullptr, tb, (const double *)nullptr, (double *)nullptr, (const int *)nullptr, (int *)nullptr,
                                       (unsigned)B, 0, 64, (hipStream_t)0);
  return (tb + 255) / 256 * 256;
}

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

size_t neo_effort_order_scratch_bytes(int B) {
  if (B <= 0) return 0;
  // keys in, keys out (doubles), indices in (ints), the sort's temporary storage: every part 256-byte aligned
  return align256((size_t)B * 16) + align256((size_t)B * 4) + effort_sort_temp_bytes(B);
}

int neo_effort_order_dev(neo_ctx *c, int B, int M, int D, const double *x0, const double *head, const double *tail, void *scratch,
                         int32_t *order) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if (!x0 || !head || !tail || !scratch || !order) return fail_locked(c, NEO_ERR_INVALID, "null buffer");
  if (((uintptr_t)scratch) & 255) return fail_locked(c, NEO_ERR_INVALID, "scratch must be 256-byte aligned");
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  double *keys = static_cast<double *>(scratch), *keys_out = keys + B;
  int *idx = reinterpret_cast<int *>(reinterpret_cast<char *>(scratch) + align256((size_t)B * 16));
  void *temp = reinterpret_cast<char *>(idx) + align256((size_t)B * 4);
  size_t tb = effort_sort_temp_bytes(B);
  hipLaunchKernelGGL(neo::effort_keys_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, B, M, D, c->params.T_min,
                     c->params.T_max, c->params.v_max, x0, head, tail, keys, idx);
  HIPCHK(c, rocprim::radix_sort_pairs_desc(temp, tb, (const double *)keys, keys_out, (const int *)idx, (int *)order, (unsigned)B, 0, 64,
                                           c->stream));
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

int neo_sampled_terms_dispatch_order(neo_ctx *c, const int32_t *order, int on_device, int B) {
  if (!c || B < 0) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  if (!order || B == 0) {
    c->sample_order_B = 0;
    return NEO_OK;
  }
  if ((size_t)B > c->sample_order_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (launches that read the old copy have finished)
    if (c->sample_order) hipFree(c->sample_order);
    c->sample_order = nullptr;
    c->sample_order_cap = 0;
    c->sample_order_B = 0;
    HIPCHK(c, hipMalloc((void **)&c->sample_order, (size_t)B * sizeof(int)));
    c->sample_order_cap = (size_t)B;
  }
  // copied into the context's own buffer before the call returns: the caller's array may go away right after it
  HIPCHK(c, hipMemcpyAsync(c->sample_order, order, (size_t)B * sizeof(int),
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sample_order_B = B;
  return NEO_OK;
}

int neo_esdf_build_config(neo_ctx *c, int flags) {
  if (!c || (flags & ~NEO_EDT_GENERIC_LINES)) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->edt_flags = flags;
  return NEO_OK;
}

int neo_optimize_plan_launches(neo_ctx *c, int64_t *fixed_plan, int64_t *dynamic_plan) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (fixed_plan) *fixed_plan = c->opt_plan_launches[0];
  if (dynamic_plan) *dynamic_plan = c->opt_plan_launches[1];
  return NEO_OK;
}

int neo_profile_enable(neo_ctx *c, int on) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->profile = on != 0;
  return NEO_OK;
}

int neo_profile_read(neo_ctx *c, int kernel, int64_t *launches, double *total_ms) {
  if (!c || kernel < 0 || kernel >= NEO_KERNEL_COUNT) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  drain_profile(c);
  if (launches) *launches = c->prof[kernel].launches;
  if (total_ms) *total_ms = c->prof[kernel].ms;
  return NEO_OK;
}

int neo_profile_reset(neo_ctx *c) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  drain_profile(c);
  for (int k = 0; k < NEO_KERNEL_COUNT; ++k) {
    c->prof[k].launches = 0;
    c->prof[k].ms = 0.0;
  }
  return NEO_OK;
}

}  // extern "C"
