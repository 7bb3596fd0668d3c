// neo_abi_util.hpp -- what the units of the C ABI (neo_abi.hip, neo_abi_fleet.hip, neo_abi_plan.hip) share and no kernel
// unit sees: the scratch layout and host copies (Carver, HostStage), the map bookkeeping, the argument checks, and the
// skeleton of each kind of entry point, once: list_launch (the `_dev` form of a list launch), null_check, HostStage::run
// (the host twin's upload / `_dev` call / download) and SceneList (the scene_ids of a host twin).
#pragma once
#include <initializer_list>

#include "neo_host.hpp"

namespace neo {
namespace abi {
namespace {  // (internal to each ABI unit, as when one unit held them: the library exports the C entry points only)

inline int ensure_scratch(neo_ctx *c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return NEO_OK;
  if (c->scratch) hipFree(c->scratch);
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  HIPCHK(c, hipMalloc(&c->scratch, bytes));
  c->scratch_bytes = bytes;
  return NEO_OK;
}

inline int ensure_pinned(neo_ctx *c, size_t bytes) {
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
// inout(), then out(), each 256-byte aligned -- then run() the `_dev` form on dev() pointers between the copies.
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

  // the body of a host twin: upload(), then `fn` (the `_dev` form on dev() pointers, valid by then), then download()
  template <typename Fn>
  __attribute__((always_inline)) int run(Fn &&fn) {
    int rc = upload();
    if (!rc) rc = fn();
    return rc ? rc : download();
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

inline int rebuild_tables(neo_ctx *c) {
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
inline int check_shape(neo_ctx *c, int B, int M, int D) {
  if (!c) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (B < 0 || M < 1 || M > NEO_MAX_PIECES || D < 2 || D > NEO_MAX_DIM)
    return fail(c, NEO_ERR_INVALID, "shape out of range (1 <= M <= 64, D in {2,3})");
  if (D * (M - 1) + M > kSlots * kWave) return fail(c, NEO_ERR_INVALID, "n = D(M-1)+M exceeds 256");
  return NEO_OK;
}

// host scene ids of a multi-scene call -> map-table slots (context locked).  The maps must all be of one kind, or, for
// the geo warm start (`geo`: the reference's A* is 2-D only), all 2-D.
inline int scene_slots(neo_ctx *c, const int32_t *scene_ids, size_t B, bool geo, std::vector<int> &slots) {
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

inline int fail_locked(neo_ctx *c, int code, const char *msg) {
  std::lock_guard<std::recursive_mutex> g(c->mu);
  return fail(c, code, msg);
}

// the end of a `_dev` entry point: the launcher's return code, then the launch's own error
inline int launched(neo_ctx *c, int rc) {
  if (rc) return rc;
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

// the (B, subset, n_subset) of the entry points that take a launch list (context unlocked): B_min <= B, B <= B_max
// where there is a bound (a power of two), at most B entries
inline int list_check(neo_ctx *c, const char *who, int B, int B_min, int B_max, const int32_t *subset, int n_subset) {
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
inline RowRefs stage_rows_in(HostStage &st, const RunRowsIn &r, size_t rows, size_t n) {
  return {st.in(r.x, rows * n), st.in(r.costs4, rows * 4), st.in(r.costs4_last, rows * 4), st.in(r.nit, rows),
          st.in_optional(r.nfev, rows), st.in(r.status, rows)};
}
inline RowRefs stage_rows_inout(HostStage &st, const RunRows &r, size_t rows, size_t n) {
  return {st.inout(r.x, rows * n), st.inout(r.costs4, rows * 4), st.inout(r.costs4_last, rows * 4),
          st.inout_optional(r.nit, rows), st.inout_optional(r.nfev, rows), st.inout(r.status, rows)};
}
inline RunRows staged_rows(const HostStage &st, const RowRefs &f) {
  return {st.dev(f.x), st.dev(f.costs4), st.dev(f.costs4_last), st.dev(f.nit), st.dev(f.nfev), st.dev(f.status)};
}
inline RunRowsIn as_const(const RunRows &r) { return {r.x, r.costs4, r.costs4_last, r.nit, r.nfev, r.status}; }

// the maps of a `_dev` call (neo_optimize_batch_from_dev, neo_audit_traj_batch_dev): with slots, the whole table of the
// reference scene's kind -- one kernel instantiation serves the whole call, so every map a slot can name (all maps of
// that kind in this context) must share its element type and layout; without, the one map of scene_id.
// Call with the context locked and the tables rebuilt.
struct CallMaps {
  int kind = 0, elem = 0, layout = 0, nmaps = 1;
  const void *table = nullptr;
};
inline int resolve_call_maps(neo_ctx *c, int scene_id, bool with_slots, CallMaps &cm) {
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

// the 2-D maps of a fleet call (context locked)
inline int fleet_maps(neo_ctx *c, int scene_id, const int32_t *slots, MapRef &m) {
  int rc = rebuild_tables(c);
  if (rc) return rc;
  CallMaps cm;
  rc = resolve_call_maps(c, scene_id, slots != nullptr, cm);
  if (rc) return rc;
  if (cm.kind != 0) return fail(c, NEO_ERR_INVALID, "fleet: the 2-D reference map only (a 3-D map was given)");
  m = {cm.table, slots, cm.nmaps};
  return NEO_OK;
}

// ---- the skeletons of the entry points
// a null among `ptrs`, or `also_bad` (what an entry checks in the same breath), refuses the call with `msg`
// (context unlocked)
inline int null_check(neo_ctx *c, const char *msg, std::initializer_list<const void *> ptrs, bool also_bad = false) {
  for (const void *p : ptrs) also_bad = also_bad || !p;
  return also_bad ? fail_locked(c, NEO_ERR_INVALID, msg) : NEO_OK;
}

// the `_dev` form of a list launch, after its checks: lock, form the list, launch nothing for an empty one, else
// `fn(list)` -- the family's launcher -- and the launch's own error
template <typename Fn>
__attribute__((always_inline)) inline int list_launch(neo_ctx *c, int B, const int32_t *subset, int n_subset, Fn &&fn) {
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const LaunchList list = launch_list(B, subset, n_subset);
  if (list.n == 0) return NEO_OK;
  return launched(c, fn(list));
}

// the scene_ids of a host twin (NULL: the one scene_id): resolve() them to map-table slots (context locked), stage()
// the slots where the twin's layout has them, then scene() and slots() are what the `_dev` form takes
struct SceneList {
  const int32_t *ids;
  std::vector<int> table_slots;
  HostStage::Ref<int> ref{-1};
  explicit SceneList(const int32_t *scene_ids) : ids(scene_ids) {}
  int resolve(neo_ctx *c, size_t B, bool geo = false) { return ids ? scene_slots(c, ids, B, geo, table_slots) : NEO_OK; }
  void stage(HostStage &st, size_t B) { ref = st.in(ids ? table_slots.data() : nullptr, B); }
  int scene(int scene_id) const { return ids ? ids[0] : scene_id; }
  const int *slots(const HostStage &st) const { return ids ? st.dev(ref) : nullptr; }
};

}  // namespace
}  // namespace abi
}  // namespace neo
