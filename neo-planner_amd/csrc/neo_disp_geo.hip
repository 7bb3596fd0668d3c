// neo_disp_geo.hip -- geo_mask_kernel / geo_search_kernel / geo_prune_kernel (neo_geo.hpp): the reference's geo warm
// start for a batch of requests, and the device state it keeps (blocked masks, the slot workspace, the scene table)
#include "neo_host.hpp"
#include "neo_geo.hpp"

namespace neo {

constexpr int kGeoMaxSlots = 1024;

// the expanded grid of astar_planner.py:36-42
static void geo_grid(const Map2D &m, int &We, int &He, double &oxe, double &oye) {
  const int grow = (int)(kGeoExpand / m.res);
  We = m.W + grow;
  He = m.H + grow;
  oxe = m.ox - kGeoExpand / 2;
  oye = m.oy - kGeoExpand / 2;
}

// the scene's blocked mask, built (stream-ordered) when missing or older than the map
static int geo_mask(neo_ctx *c, int scene_id, const MapEntry &e, const unsigned *&bits) {
  GeoMask &gm = c->geo.masks[scene_id];
  if (gm.bits && gm.version == e.version) {
    bits = static_cast<const unsigned *>(gm.bits);
    return NEO_OK;
  }
  int We, He;
  double oxe, oye;
  geo_grid(e.m2, We, He, oxe, oye);
  const size_t words = ((size_t)We * He + 31) / 32;
  if (gm.bits) {
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (a launch in flight may still read the old mask)
    hipFree(gm.bits);
    gm.bits = nullptr;
  }
  HIPCHK(c, hipMalloc(&gm.bits, words * sizeof(unsigned)));
  hipLaunchKernelGGL(geo_mask_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, c->stream, e.m2, We, He,
                     e.m2.res, oxe, oye, static_cast<unsigned *>(gm.bits));
  HIPCHK(c, hipGetLastError());
  gm.version = e.version;
  bits = static_cast<const unsigned *>(gm.bits);
  return NEO_OK;
}

// the call's scene table on the device: every 2-D map by map-table slot (with slots), or the one map of scene_id
static int geo_table(neo_ctx *c, int scene_id, bool with_slots, int &nscenes, size_t &max_cells) {
  std::vector<GeoScene> t;
  for (auto &kv : c->maps) {
    const MapEntry &e = kv.second;
    if (e.kind != 0 || (!with_slots && kv.first != scene_id)) continue;
    GeoScene g{};
    int rc = geo_mask(c, kv.first, e, g.mask);
    if (rc) return rc;
    g.m = e.m2;
    geo_grid(e.m2, g.We, g.He, g.oxe, g.oye);
    g.res = e.m2.res;
    const size_t idx = with_slots ? (size_t)e.slot : 0;
    if (t.size() <= idx) t.resize(idx + 1);
    t[idx] = g;
  }
  nscenes = (int)t.size();
  max_cells = 0;
  for (const GeoScene &g : t) max_cells = std::max(max_cells, (size_t)g.We * g.He);
  const size_t bytes = t.size() * sizeof(GeoScene);
  GeoState &gs = c->geo;
  if (gs.table_host.size() != bytes || memcmp(gs.table_host.data(), t.data(), bytes) != 0) {
    if (gs.table) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      hipFree(gs.table);
      gs.table = nullptr;
    }
    gs.table_host.assign(reinterpret_cast<const char *>(t.data()), reinterpret_cast<const char *>(t.data()) + bytes);
    HIPCHK(c, hipMalloc(&gs.table, bytes));
    HIPCHK(c, hipMemcpyAsync(gs.table, gs.table_host.data(), bytes, hipMemcpyHostToDevice, c->stream));
  }
  return NEO_OK;
}

static void geo_free_workspace(GeoState &gs) {
  if (gs.cells) hipFree(gs.cells);
  if (gs.heap) hipFree(gs.heap);
  if (gs.epochs) hipFree(gs.epochs);
  if (gs.work) hipFree(gs.work);
  gs.cells = gs.heap = nullptr;
  gs.epochs = nullptr;
  gs.work = nullptr;
  gs.cells_cap = 0;
  gs.nslots = 0;
}

// slots of `cells` cells each, as many as the byte budget holds (at most kGeoMaxSlots), stamps cleared
static int geo_workspace(neo_ctx *c, size_t cells, int B) {
  GeoState &gs = c->geo;
  const size_t per_slot = cells * (sizeof(GeoCell) + sizeof(GeoHeapEnt));
  const size_t fit = per_slot ? gs.budget / per_slot : 0;
  const int want = (int)std::min<size_t>(fit, kGeoMaxSlots);
  if (want < 1)
    return fail(c, NEO_ERR_HIP, "geo: the workspace budget (" + std::to_string(gs.budget) + " bytes) holds no slot of " +
                                    std::to_string(per_slot) + " bytes");
  const bool wrap = gs.searches + (unsigned long long)B >= kGeoEpochMax;
  if (gs.cells && gs.cells_cap >= cells && gs.nslots == want && !wrap) return NEO_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!(gs.cells && gs.cells_cap >= cells && gs.nslots == want)) {
    geo_free_workspace(gs);
    const size_t nc = cells * (size_t)want;
    if (hipMalloc(&gs.cells, nc * sizeof(GeoCell)) != hipSuccess ||
        hipMalloc(&gs.heap, nc * sizeof(GeoHeapEnt)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&gs.epochs), (size_t)want * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&gs.work), sizeof(int)) != hipSuccess) {
      (void)hipGetLastError();
      geo_free_workspace(gs);
      return fail(c, NEO_ERR_HIP, "geo: could not allocate the workspace (" + std::to_string(want) + " slots of " +
                                      std::to_string(per_slot) + " bytes)");
    }
    gs.cells_cap = cells;
    gs.nslots = want;
  }
  // every stamp back to 0: the epochs restart (and a fresh buffer holds no stale stamp)
  HIPCHK(c, hipMemsetAsync(gs.cells, 0, gs.cells_cap * (size_t)gs.nslots * sizeof(GeoCell), c->stream));
  HIPCHK(c, hipMemsetAsync(gs.epochs, 0, (size_t)gs.nslots * sizeof(unsigned), c->stream));
  gs.searches = 0;
  return NEO_OK;
}

int geo_search(neo_ctx *c, int scene_id, const GeoArgs &a) {
  int nscenes;
  size_t cells;
  int rc = geo_table(c, scene_id, a.slots != nullptr, nscenes, cells);
  if (rc) return rc;
  rc = geo_workspace(c, cells, a.B);
  if (rc) return rc;
  GeoState &gs = c->geo;
  HIPCHK(c, hipMemsetAsync(gs.work, 0, sizeof(int), c->stream));
  const GeoOut o{a.key_pts, a.path, a.path_cost, a.path_len, a.expansions, a.flags, a.path_cap};
  const int grid = std::min(gs.nslots, a.B);
  hipLaunchKernelGGL(geo_search_kernel, dim3(grid), dim3(kWave), 0, c->stream, static_cast<const GeoScene *>(gs.table),
                     a.slots, nscenes, a.B, a.start, a.target, a.max_exp, o, static_cast<GeoCell *>(gs.cells),
                     static_cast<GeoHeapEnt *>(gs.heap), gs.cells_cap, gs.epochs, gs.work);
  HIPCHK(c, hipGetLastError());
  gs.searches += (unsigned long long)a.B;
  return NEO_OK;
}

int geo_prune(neo_ctx *c, int scene_id, int B, const int *slots, const double *paths, const int *path_len, int stride,
              double *key_pts) {
  int nscenes;
  size_t cells;
  int rc = geo_table(c, scene_id, slots != nullptr, nscenes, cells);
  if (rc) return rc;
  hipLaunchKernelGGL(geo_prune_kernel, dim3(B), dim3(kWave), 0, c->stream, static_cast<const GeoScene *>(c->geo.table),
                     slots, nscenes, B, paths, path_len, stride, key_pts);
  HIPCHK(c, hipGetLastError());
  return NEO_OK;
}

void geo_forget(neo_ctx *c, int scene_id) {
  auto it = c->geo.masks.find(scene_id);
  if (it == c->geo.masks.end()) return;
  if (it->second.bits) hipFree(it->second.bits);  // (the caller has synchronised the device)
  c->geo.masks.erase(it);
}

void geo_release(neo_ctx *c) {
  GeoState &gs = c->geo;
  for (auto &kv : gs.masks)
    if (kv.second.bits) hipFree(kv.second.bits);
  gs.masks.clear();
  geo_free_workspace(gs);
  if (gs.table) hipFree(gs.table);
  gs.table = nullptr;
  gs.table_host.clear();
}

}  // namespace neo
