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
  ++c->geo.mask_builds;
  gm.version = e.version;
  bits = static_cast<const unsigned *>(gm.bits);
  return NEO_OK;
}

// the call's scene table on the device: every 2-D map by map-table slot (with slots), or the one map of scene_id.
// direct: the scenes carry no mask (GeoScene::mask NULL) and none is built, whichever scenes the table holds; the two
// forms keep a table each, so that calls of both kinds do not evict one another's.
static int geo_table(neo_ctx *c, int scene_id, bool with_slots, bool direct, int &nscenes, size_t &max_cells) {
  std::vector<GeoScene> t;
  for (auto &kv : c->maps) {
    const MapEntry &e = kv.second;
    if (e.kind != 0 || (!with_slots && kv.first != scene_id)) continue;
    GeoScene g{};
    if (!direct) {
      int rc = geo_mask(c, kv.first, e, g.mask);
      if (rc) return rc;
    }
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
  void *&table = c->geo.table[direct];
  std::vector<char> &host = c->geo.table_host[direct];
  if (host.size() != bytes || memcmp(host.data(), t.data(), bytes) != 0) {
    if (table) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      hipFree(table);
      table = nullptr;
    }
    host.assign(reinterpret_cast<const char *>(t.data()), reinterpret_cast<const char *>(t.data()) + bytes);
    HIPCHK(c, hipMalloc(&table, bytes));
    HIPCHK(c, hipMemcpyAsync(table, host.data(), bytes, hipMemcpyHostToDevice, c->stream));
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
static int geo_workspace(neo_ctx *c, size_t cells, int n) {
  GeoState &gs = c->geo;
  const size_t per_slot = cells * (sizeof(GeoCell) + sizeof(GeoHeapEnt));
  const size_t fit = per_slot ? gs.budget / per_slot : 0;
  const int want = (int)std::min<size_t>(fit, kGeoMaxSlots);
  if (want < 1)
    return fail(c, NEO_ERR_HIP, "geo: the workspace budget (" + std::to_string(gs.budget) + " bytes) holds no slot of " +
                                    std::to_string(per_slot) + " bytes");
  const bool wrap = gs.searches + (unsigned long long)n >= kGeoEpochMax;
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
  const int n = a.list.size();  // the searches of this launch: what the epochs are charged
  int rc = geo_table(c, scene_id, a.slots != nullptr, a.direct, nscenes, cells);
  if (rc) return rc;
  rc = geo_workspace(c, cells, n);
  if (rc) return rc;
  GeoState &gs = c->geo;
  HIPCHK(c, hipMemsetAsync(gs.work, 0, sizeof(int), c->stream));
  const GeoOut o{a.key_pts, a.path, a.path_cost, a.path_len, a.expansions, a.flags, a.path_cap};
  GeoIn in{a.list, a.start, a.target, a.stride, a.x0, {0.0, 0.0, 0.0}};
  if (a.x0)
    for (int k = 0; k < 3; ++k) in.tau[k] = a.tau[k];
  const int grid = std::min(gs.nslots, n);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWave), 0, c->stream, static_cast<const GeoScene *>(gs.table[a.direct]),
                       a.slots, nscenes, in, a.max_exp, o, static_cast<GeoCell *>(gs.cells),
                       static_cast<GeoHeapEnt *>(gs.heap), gs.cells_cap, gs.epochs, gs.work);
  };
  if (a.direct) launch(geo_search_kernel<true>);
  else launch(geo_search_kernel<false>);
  HIPCHK(c, hipGetLastError());
  gs.searches += (unsigned long long)n;
  return NEO_OK;
}

int geo_prune(neo_ctx *c, int scene_id, int B, const int *slots, const double *paths, const int *path_len, int stride,
              double *key_pts) {
  int nscenes;
  size_t cells;
  int rc = geo_table(c, scene_id, slots != nullptr, false, nscenes, cells);
  if (rc) return rc;
  hipLaunchKernelGGL(geo_prune_kernel, dim3(B), dim3(kWave), 0, c->stream, static_cast<const GeoScene *>(c->geo.table[0]),
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
  for (int k = 0; k < 2; ++k) {
    if (gs.table[k]) hipFree(gs.table[k]);
    gs.table[k] = nullptr;
    gs.table_host[k].clear();
  }
}

}  // namespace neo
