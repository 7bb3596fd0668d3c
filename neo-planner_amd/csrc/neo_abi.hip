// neo_abi.hip -- C ABI of libneo_planner_hip.so (include/neo_planner.h), first of three units: the context, the
// parameters, the maps, cost-grad, the sampled terms, the optimiser, the trajectory states and audit, the geo warm start
// and the trace / counter / order / profile calls.  neo_abi_fleet.hip has the depth camera, onboard maps, the fleet,
// record and init entry points, neo_abi_plan.hip the batch, plan and adaptive ones.  Argument checks, locking, scratch
// layout and host copies and the map bookkeeping are shared (neo_abi_util.hpp); every entry point makes one call into
// the kernel family's unit (neo_disp_*.hip).  No device header is included here: the kernels this unit still holds are
// rocPRIM's sort of the dispatch order with pack_results_kernel and effort_keys_kernel around it.
//
// The map kernels are in neo_esdf.hpp (launched from neo_disp_esdf.hip); traj_state_kernel (neo_pieces.hpp) and
// audit_kernel (neo_audit.hpp) are launched from neo_disp_audit.hip; the fused kernels (eval / optimize / sample) are
// templates in neo_kernels.hpp, instantiated per family in the neo_disp_*.hip translation units.
#include <cstring>
#include "neo_abi_util.hpp"
#include <rocprim/device/device_radix_sort.hpp>

// =================================================================== host side
using namespace neo;
using namespace neo::abi;

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

// From this batch size on the kernels take the two-wavefronts-per-SIMD register allocation (three in the all-fp32
// mode, always).  Measured in round 3, one launch at a time, two waves against one: fp64 mode +4 % at 1024, +9 % at 2048,
// +23 % at 3072 trajectories; mixed mode +2 %, +5 %, +23 % (round 2 had found one wave faster up to 2048: 9.1 against
// 10.1 ms -- before the per-evaluation loads and the spills of the two-waves kernels were gone).
constexpr int kTwoWavesFromBatch = 1024;
bool two_waves_wanted(const neo_ctx *c, int B) {
  const int fl = c->params.flags;
  return (B >= kTwoWavesFromBatch && !(fl & NEO_FLAG_ONE_WAVE_PER_SIMD)) || (fl & NEO_FLAG_TWO_WAVES_PER_SIMD);
}

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
  if (int rc = null_check(c, "batch build: null buffer", {scene_ids, occ, origins})) return rc;
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
  return st.run([&]() -> int {
    esdf_query(c, e, n, st.dev(f_p), st.dev(f_d), st.dev(f_g));
    return NEO_OK;
  });
}

int neo_cost_grad_batch_dev(neo_ctx *c, int scene_id, int B, int M, int D, const double *x, const double *head,
                            const double *tail, double *cost, double *costs4, double *grad, double *coeffs,
                            int32_t *status) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if ((rc = null_check(c, "null buffer", {x, head, tail, cost, costs4, grad}))) return rc;
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
  if ((rc = null_check(c, "null buffer", {x, head, tail, cost, costs4, grad}))) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  HostStage st(c, kStagedUpTo);  // (get_cost / get_grad of one trajectory: one copy each way)
  const auto fx = st.in(x, bs * n), fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  const auto fc = st.out(cost, bs), fc4 = st.out(costs4, bs * 4), fg = st.out(grad, bs * n);
  const auto fco = st.out(coeffs, bs * 6 * M * D);
  const auto fst = st.out(status, bs);
  return st.run([&] {
    return neo_cost_grad_batch_dev(c, scene_id, B, M, D, st.dev(fx), st.dev(fh), st.dev(ft), st.dev(fc), st.dev(fc4),
                                   st.dev(fg), coeffs ? st.dev(fco) : nullptr, st.dev(fst));
  });
}

// IO32: coeffs / grad_C / grad_T are floats (the _f32 entry points; fp32 sampling only)
static int sampled_terms_dev(neo_ctx *c, int scene_id, int B, int M, int D, const void *coeffs, const double *ts, double *costs2,
                             void *grad_C, void *grad_T, bool io32) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if ((rc = null_check(c, "null buffer", {coeffs, ts, costs2, grad_C, grad_T}))) return rc;
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
  if ((rc = null_check(c, "null buffer", {coeffs, ts, costs2, grad_C, grad_T}))) return rc;
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
  return st.run([&] {
    return sampled_terms_dev(c, scene_id, B, M, D, st.dev(fco), st.dev(fts), st.dev(fc2), st.dev(fgc), st.dev(fgt), io32);
  });
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
  if ((rc = null_check(c, "null buffer", {x0, x, head, tail, costs4, nit, nfev, status}))) return rc;
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
  if ((rc = null_check(c, "null buffer", {x0, x, head, tail, costs4, nit, nfev, status, state}))) return rc;
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
  if ((rc = null_check(c, "null buffer", {x, head, tail, costs4, nit, nfev, status}))) return rc;
  if (B == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);  // scratch buffers stay ours until the copies back are done
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  SceneList scenes(scene_ids);
  if ((rc = scenes.resolve(c, bs))) return rc;
  // the inputs are one contiguous range ending with x, the outputs one starting with it
  HostStage st(c, kStagedUpTo);
  const auto fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  scenes.stage(st, bs);
  const auto fx = st.inout(x, bs * n);
  const auto fc4 = st.out(costs4, bs * 4), fc4l = st.out(costs4_last, bs * 4);
  const auto fnit = st.out(nit, bs), fnfev = st.out(nfev, bs), fst = st.out(status, bs);
  return st.run([&] {
    return neo_optimize_batch_dev(c, scenes.scene(scene_id), scenes.slots(st), B, M, D, st.dev(fx), st.dev(fh), st.dev(ft),
                                  st.dev(fc4), st.dev(fc4l), st.dev(fnit), st.dev(fnfev), st.dev(fst));
  });
}

int neo_eval_traj_batch(neo_ctx *c, int B, int M, int D, const double *x, const double *head, const double *tail,
                        double hz, int K, double *state, int32_t *count) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if ((rc = null_check(c, "bad argument", {x, head, tail, state, count}, K < 0 || !(hz > 0.0)))) return rc;
  if (B == 0 || K == 0) return NEO_OK;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t n = (size_t)D * (M - 1) + M, bs = (size_t)B;
  HostStage st(c, kStagedUpTo);
  const auto fx = st.in(x, bs * n), fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  const auto fs = st.out(state, bs * K * 3 * D);
  const auto fcnt = st.out(count, bs);
  return st.run([&]() -> int {
    return launched(c, dispatch_traj_state(c, D, {B, M, st.dev(fx), st.dev(fh), st.dev(ft), hz, K, st.dev(fs), st.dev(fcnt)}));
  });
}

// ---- trajectory audit (ros_node/traj_planner_node.py:333-363; kernel: neo_audit.hpp)
// the argument checks both forms make before anything is copied or launched (context unlocked)
static int audit_check(neo_ctx *c, int B, int M, int D, const double *x, const double *head, const double *tail, double hz,
                       const double *audit, const int32_t *count, const int32_t *flags) {
  int rc = check_shape(c, B, M, D);
  if (rc) return rc;
  if ((rc = null_check(c, "audit: null buffer", {x, head, tail, audit, count, flags}))) return rc;
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
  SceneList scenes(scene_ids);
  if ((rc = scenes.resolve(c, bs))) return rc;
  HostStage st(c, 0);
  const auto fx = st.in(x, bs * n), fh = st.in(head, bs * 3 * D), ft = st.in(tail, bs * 3 * D);
  scenes.stage(st, bs);
  const auto fa = st.out(audit, bs * NEO_AUDIT_FIELDS);
  const auto fcnt = st.out(count, bs), ffl = st.out(flags, bs);
  return st.run([&] {
    return neo_audit_traj_batch_dev(c, scenes.scene(scene_id), scenes.slots(st), B, M, D, st.dev(fx), st.dev(fh), st.dev(ft),
                                    hz, weights3, st.dev(fa), st.dev(fcnt), st.dev(ffl));
  });
}

// ---- geo warm start (traj_planner/astar_planner.py, geo_planner.py:19-101; kernels: neo_geo.hpp)
static int geo_check(neo_ctx *c, int B, const double *start, const double *target, int max_expansions, int path_cap,
                     const double *key_pts, const double *path, const int32_t *path_len, const double *path_cost,
                     const int32_t *expansions, const int32_t *flags) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 1) return fail_locked(c, NEO_ERR_INVALID, "geo: B must be >= 1");
  if (max_expansions < 0 || path_cap < 0 || (path && path_cap < 1))
    return fail_locked(c, NEO_ERR_INVALID, "geo: max_expansions and path_cap must be >= 0 (path_cap >= 1 with a path)");
  return null_check(c, "geo: null buffer", {start, target, key_pts, path_len, path_cost, expansions, flags});
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
  const GeoArgs ga{launch_list(B, nullptr, 0), scene_ids, start, target, 2, max_expansions, path ? path_cap : 0, key_pts,
                   path, path_cost, path_len, expansions, flags, nullptr, nullptr, false};
  return geo_search(c, scene_id, ga);
}

int neo_geo_guess_dev(neo_ctx *c, int scene_id, const int32_t *slots, int B, const int32_t *subset, int count,
                      const double *head, const double *tail, const double *tau3, int max_expansions, int direct,
                      double *x0, double *key_pts, int32_t *path_len, double *path_cost, int32_t *expansions,
                      int32_t *flags) {
  int rc = list_check(c, "geo guess", B, 1, INT32_MAX, subset, count);
  if (rc) return rc;
  if (max_expansions < 0) return fail_locked(c, NEO_ERR_INVALID, "geo guess: max_expansions must be >= 0");
  rc = null_check(c, "geo guess: null buffer", {head, tail, tau3, x0, key_pts, path_len, path_cost, expansions, flags});
  if (rc) return rc;
  return list_launch(c, B, subset, count, [&](const LaunchList &list) {
    int rc2 = rebuild_tables(c);
    if (rc2) return rc2;
    rc2 = geo_scene_kind(c, scene_id);
    if (rc2) return rc2;
    const GeoArgs ga{list, slots, head, tail, 6, max_expansions, 0, key_pts, nullptr, path_cost, path_len, expansions,
                     flags, x0, tau3, direct != 0};
    return geo_search(c, scene_id, ga);
  });
}

int neo_geo_mask_builds(neo_ctx *c, int64_t *count) {
  if (!c || !count) return NEO_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  *count = c->geo.mask_builds;
  return NEO_OK;
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
  SceneList scenes(scene_ids);
  rc = scene_ids ? scenes.resolve(c, bs, true) : geo_scene_kind(c, scene_id);
  if (rc) return rc;
  HostStage st(c, 0);
  const auto fs = st.in(start, 2 * bs), ft = st.in(target, 2 * bs);
  scenes.stage(st, bs);
  const auto fk = st.out(key_pts, 8 * bs), fc = st.out(path_cost, bs), fp = st.out(path, 2 * bs * pc);
  const auto fl = st.out(path_len, bs), fe = st.out(expansions, bs), ff = st.out(flags, bs);
  return st.run([&] {
    return neo_geo_search_batch_dev(c, scenes.scene(scene_id), scenes.slots(st), B, st.dev(fs), st.dev(ft), max_expansions,
                                    path_cap, st.dev(fk), path ? st.dev(fp) : nullptr, st.dev(fl), st.dev(fc), st.dev(fe),
                                    st.dev(ff));
  });
}

int neo_geo_prune_batch(neo_ctx *c, int scene_id, const int32_t *scene_ids, int B, const double *paths,
                        const int32_t *path_len, int path_stride, double *key_pts) {
  if (!c) return NEO_ERR_INVALID;
  if (B < 1 || path_stride < 1) return fail_locked(c, NEO_ERR_INVALID, "geo prune: B and path_stride must be >= 1");
  if (int rc = null_check(c, "geo prune: null buffer", {paths, path_len, key_pts})) return rc;
  for (int i = 0; i < B; ++i)
    if (path_len[i] < 1 || path_len[i] > path_stride)
      return fail_locked(c, NEO_ERR_INVALID, "geo prune: path_len must be in [1, path_stride]");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc = rebuild_tables(c);
  if (rc) return rc;
  const size_t bs = (size_t)B, ps = (size_t)path_stride;
  SceneList scenes(scene_ids);
  rc = scene_ids ? scenes.resolve(c, bs, true) : geo_scene_kind(c, scene_id);
  if (rc) return rc;
  HostStage st(c, 0);
  const auto fp = st.in(paths, 2 * bs * ps);
  const auto fl = st.in(path_len, bs);
  scenes.stage(st, bs);
  const auto fk = st.out(key_pts, 8 * bs);
  return st.run([&] {
    return geo_prune(c, scenes.scene(scene_id), B, scenes.slots(st), st.dev(fp), st.dev(fl), path_stride, st.dev(fk));
  });
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
  if (int rc = null_check(c, "null buffer", {x, costs4, weights4, out})) return rc;
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
  if ((rc = null_check(c, "null buffer", {x0, head, tail, scratch, order}))) return rc;
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
