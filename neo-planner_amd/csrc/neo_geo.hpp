// neo_geo.hpp -- the reference's `geo` warm start on the GPU (traj_planner/astar_planner.py, geo_planner.py:19-101):
// the blocked mask of a scene's expanded A* grid, the A* search of a batch of requests and the pruning of their paths
// to four key nodes (include/neo_planner.h, neo_geo_search_batch / neo_geo_prune_batch).  Included by
// neo_disp_geo.hip only.
//
// Exactness.  Every position is the reference's fp64 value: calc_real_pos rounds the product and the sum separately
// (__dmul_rn / __dadd_rn: the units compile with -ffp-contract=on, which would fuse `o + i * res`), cell indices
// truncate toward zero like int(), and distances are neo_esdf_query's nearest-cell lookup (Lookup2D).  The open set is
// a binary heap ordered by (f, seq): f = g + hypot(dx, dy) in fp64 (a correctly rounded square root of an exact
// integer), seq the counter of the node's FIRST insertion.  That is the order in which the reference's
// min(open_set, key=...) over an insertion-ordered dict selects nodes, a decrease-key keeping the entry's place.
//
// Search (geo_search_kernel): one wavefront per request, persistent -- the launch has one workgroup per workspace slot
// and each takes requests from a counter until none is left.  The search itself is sequential; lane 0 runs it, with
// the eight neighbour gathers of an expansion issued together before the first is used.  The heap lives in LDS and
// moves, whole, into the slot's global heap once it outgrows kGeoHeapLds entries.  Per-cell state (g, heap position,
// epoch | state | parent direction) lives in the slot's global workspace; the epoch stamp of a search makes every cell
// of earlier searches "unvisited", so nothing is cleared between requests.  After the search the whole wavefront prunes
// the path, which lane 0 has written into the slot's (then unused) global heap.
//
// Two forms of one kernel.  geo_search_kernel<false> reads a cell's blocked bit from the scene's mask;
// geo_search_kernel<true> (the DIRECT form) evaluates geo_cell_blocked, the expression the mask is built from, on the
// map's records where it needs a cell: no mask has to exist, which is what a map that changes every tick wants.  The two
// give equal results by construction.  The requests of a launch are a LaunchList (neo_launch_list.hpp) over rows of
// caller arrays with a row stride (GeoIn): the dense (B, 2) starts and targets, or head / tail [B][3][2] where they
// lie; with GeoIn::x0 the lanes that write the key nodes also write the optimiser's first guess.
#pragma once
#include <climits>
#include "neo_map.hpp"
#include "neo_launch_list.hpp"

namespace neo {

constexpr int kGeoHeapLds = 2048;            // heap entries kept in LDS (32 KiB)
constexpr double kGeoSafeDis = 0.5;          // esdf.py SAFE_DIS: has_collision
constexpr double kGeoSegDis = 0.4;           // geo_planner.py:55 seg_feasible_check
constexpr double kGeoExpand = 10.0;          // astar_planner.py:37 map_expand_radius
constexpr unsigned kGeoOpen = 1u, kGeoClosed = 2u;
constexpr unsigned kGeoEpochMax = (1u << 27) - 1u;  // tag = epoch << 5 | state << 3 | dir

// a scene as the search sees it: the mask of its expanded grid and the map itself (the prune's lookups)
struct GeoScene {
  const unsigned *mask;  // bit k of word k >> 5: the expanded cell of key k = x + y * We is blocked
  Map2D m;
  int We, He;
  double res, oxe, oye;  // origin of the expanded grid
};

struct GeoCell {
  double g;
  int hpos;      // position in the heap while open
  unsigned tag;  // epoch << 5 | state << 3 | direction of the move that reached it (get_motion_model order)
};

struct GeoHeapEnt {
  double f;
  int seq, key;
};

// get_motion_model (astar_planner.py:105-116)
__device__ __forceinline__ int geo_mdx(int j) { return j == 0 ? 1 : j == 2 ? -1 : (j == 1 || j == 3) ? 0 : (j < 6 ? -1 : 1); }
__device__ __forceinline__ int geo_mdy(int j) {
  return j == 1 ? 1 : j == 3 ? -1 : (j == 0 || j == 2) ? 0 : ((j == 4 || j == 6) ? -1 : 1);
}

// calc_real_pos: o + i * res, rounded twice like Python
__device__ __forceinline__ double geo_real(double o, double i, double res) { return __dadd_rn(o, __dmul_rn(i, res)); }

// calc_xy_index: int((p - o) / res); `ok` false when the value is beyond any grid (and int() of it is not an int here)
__device__ __forceinline__ double geo_index(double p, double o, double res, bool &ok) {
  const double v = (p - o) / res;
  ok = fabs(v) < 1.0e9;
  return trunc(v);
}

__device__ __forceinline__ bool geo_less(const GeoHeapEnt &a, const GeoHeapEnt &b) {
  return a.f < b.f || (a.f == b.f && a.seq < b.seq);
}

// math.hypot of integer differences (|dx|, |dy| < 2^26): the exact sum of squares, correctly rounded square root
__device__ __forceinline__ double geo_hypot(long long dx, long long dy) { return __dsqrt_rn((double)(dx * dx + dy * dy)); }

// ---------------------------------------------------------------- blocked cells
// has_collision of the expanded cell (x, y): the map's nearest-cell distance at its position is below kGeoSafeDis.
// Split like the lookup itself -- geo_cell_addr (index arithmetic), Lookup2D::load (the gather), geo_blocked_from -- so
// that the direct search can put the eight gathers of an expansion in flight together; geo_cell_blocked is the three in
// a row, what the mask holds a bit of.  `on` false: no cell (the address of a point outside the map: record 0, ignored).
using GeoLookup = Lookup2D<double>;
__device__ __forceinline__ GeoLookup::Addr geo_cell_addr(const GeoLookup &lk, double oxe, double oye, double res, int x,
                                                         int y, bool on = true) {
  const double pos[2] = {geo_real(oxe, (double)x, res), geo_real(oye, (double)y, res)};
  return lk.prepare<2>(pos, on);
}
__device__ __forceinline__ bool geo_blocked_from(const GeoLookup &lk, const GeoLookup::Addr &a, const GeoLookup::Raw &q) {
  double g[2];
  return lk.finish<2>(a, q, g) < kGeoSafeDis;
}
__device__ __forceinline__ bool geo_cell_blocked(const GeoLookup &lk, double oxe, double oye, double res, int x, int y) {
  const GeoLookup::Addr a = geo_cell_addr(lk, oxe, oye, res, x, y);
  return geo_blocked_from(lk, a, lk.load(a));
}

// the blocked mask: one thread per 32-cell word
__global__ void __launch_bounds__(256) geo_mask_kernel(Map2D m, int We, int He, double res, double oxe, double oye,
                                                       unsigned *mask) {
  const long long ncell = (long long)We * He;
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= ncell) return;
  const GeoLookup lk(m);
  unsigned bits = 0;
  for (int b = 0; b < 32; ++b) {
    const long long k = w * 32 + b;
    if (k >= ncell) break;
    if (geo_cell_blocked(lk, oxe, oye, res, (int)(k % We), (int)(k / We))) bits |= 1u << b;
  }
  mask[w] = bits;
}

// ---------------------------------------------------------------- prune (geo_planner.py:37-101), whole wavefront
// seg_feasible_check(path[a], path[b]): the np.linspace points against get_edt_dis < 0.4, 64 points a round, ending at
// the first round with an infeasible point
__device__ __forceinline__ bool geo_seg_feasible(const Map2D &m, double x0, double y0, double x1, double y1) {
  const double dx = x1 - x0, dy = y1 - y0;
  const double ax = fabs(dx), ay = fabs(dy);
  const double mx = ax >= ay ? ax : ay;
  const double sn = ceil(mx / 0.1) + 1.0;
  if (!(sn < 1.0e9)) return false;  // (a non-finite or absurd segment: treated as infeasible)
  const long long num = (long long)sn;
  const double div = (double)(num - 1);
  const double sx = num > 1 ? dx / div : 0.0, sy = num > 1 ? dy / div : 0.0;
  const Lookup2D<double> lk(m);
  for (long long base = 0; base < num; base += kWave) {
    const long long i = base + lane_id();
    bool bad = false;
    if (i < num) {
      double px, py;
      if (num > 1 && i == num - 1) {
        px = x1;
        py = y1;
      } else {
        // y = arange * step (or arange / div * delta where step == 0, numpy's denormal branch), then += start
        const double fi = (double)i;
        const double tx = sx == 0.0 && num > 1 ? __dmul_rn(fi / div, dx) : __dmul_rn(fi, sx);
        const double ty = sy == 0.0 && num > 1 ? __dmul_rn(fi / div, dy) : __dmul_rn(fi, sy);
        px = __dadd_rn(tx, x0);
        py = __dadd_rn(ty, y0);
      }
      const double pos[2] = {px, py};
      double g[2];
      bool inside;
      bad = lk.fetch<2>(pos, g, inside) < kGeoSegDis;
    }
    if (__any(bad)) return false;
  }
  return true;
}

// prune_path_nodes: the indices of the four key nodes of the n-node path (xy interleaved, `path` readable by all
// lanes).  Wave-uniform control flow; every lane returns the same indices.
__device__ __forceinline__ void geo_prune(const Map2D &m, const double *path, int n, int (&out)[4]) {
  const int last = n >= 2 ? n - 1 : 0;  // the last key index is always the last node
  const double aL = (1.0 / 3.0) * (double)last, aR = (2.0 / 3.0) * (double)last;
  int kv[4] = {0, 0, 0, 0};
  int count = 0, bestL = 0, bestR = 0;
  double dL = INFINITY, dR = INFINITY;
  auto add = [&](int k) {
    if (count < 4) kv[count] = k;
    ++count;
    const double eL = fabs((double)k - aL), eR = fabs((double)k - aR);
    if (eL < dL) { dL = eL; bestL = k; }  // min(): the first occurrence of the minimum
    if (eR < dR) { dR = eR; bestR = k; }
  };
  add(0);
  int head = 0, tail = 1;
  while (tail < n) {
    while (tail - head == 1 ||
           geo_seg_feasible(m, path[2 * head], path[2 * head + 1], path[2 * tail], path[2 * tail + 1])) {
      ++tail;
      if (tail == n) break;
    }
    add(tail - 1);
    head = tail - 1;
  }
  if (count == 2) {  // np.linspace(k0, k1, 4).astype(int)
    const double st = (double)(kv[1] - kv[0]) / 3.0;
    out[0] = kv[0];
    out[1] = (int)__dadd_rn(__dmul_rn(1.0, st), (double)kv[0]);
    out[2] = (int)__dadd_rn(__dmul_rn(2.0, st), (double)kv[0]);
    out[3] = kv[1];
  } else if (count == 3) {
    if (kv[1] - kv[0] > kv[2] - kv[1]) {
      out[0] = kv[0]; out[1] = (kv[0] + kv[1]) / 2; out[2] = kv[1]; out[3] = kv[2];
    } else {
      out[0] = kv[0]; out[1] = kv[1]; out[2] = (kv[1] + kv[2]) / 2; out[3] = kv[2];
    }
  } else if (count == 4) {
    for (int k = 0; k < 4; ++k) out[k] = kv[k];
  } else {
    out[0] = 0; out[1] = bestL; out[2] = bestR; out[3] = last;
  }
}

__device__ __forceinline__ void geo_write_keys(const double *path, const int (&idx)[4], double *key_pts) {
  if (lane_id() < 8) {
    const int k = lane_id() >> 1, d = lane_id() & 1;
    key_pts[lane_id()] = path[2 * idx[k] + d];
  }
}

// neo_geo_prune_batch: caller-given paths [B][stride][2]
__global__ void __launch_bounds__(kWave) geo_prune_kernel(const GeoScene *scenes, const int *slots, int nscenes, int B,
                                                          const double *paths, const int *path_len, int stride,
                                                          double *key_pts) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const int s = slots ? slots[b] : 0;
  double *kp = key_pts + (size_t)b * 8;
  const int n = path_len[b];
  if (s < 0 || s >= nscenes || n < 1 || n > stride) {
    if (lane_id() < 8) kp[lane_id()] = NAN;
    return;
  }
  const double *p = paths + (size_t)b * stride * 2;
  int idx[4];
  geo_prune(scenes[s].m, p, n, idx);
  geo_write_keys(p, idx, kp);
}

// ---------------------------------------------------------------- search
struct GeoOut {
  double *key_pts, *path, *path_cost;
  int *path_len, *expansions, *flags;
  int path_cap;
};

// the requests of a launch: position p of `list` works on request b, whose start is start[b * stride ..+2] and whose
// target is target[b * stride ..+2] (stride 2: dense arrays; 6: head / tail [B][3][2], the position rows).  x0 non-NULL:
// request b's row x0[b][7] = [k1.x, k2.x, k1.y, k2.y, tau[0], tau[1], tau[2]] is written with its key nodes.
struct GeoIn {
  LaunchList list;
  const double *start, *target;
  int stride;
  double *x0;
  double tau[3];
};

// the key nodes of a request (lanes 0 - 7: node k = lane >> 1, coordinate d = lane & 1; `v` the lane's value) and, with
// x0, its first guess: the inner nodes' lanes write the waypoints, lanes 0, 1 and 6 the three tau
__device__ __forceinline__ void geo_write_result(const GeoIn &in, const GeoOut &o, int b, double v) {
  const int lane = lane_id();
  if (lane >= 8) return;
  o.key_pts[(size_t)b * 8 + lane] = v;
  if (!in.x0) return;
  double *x0 = in.x0 + (size_t)b * 7;
  const int k = lane >> 1, d = lane & 1;
  if (k == 1 || k == 2) x0[2 * d + (k - 1)] = v;
  else if (lane != 7) x0[4 + (lane == 6 ? 2 : lane)] = lane == 0 ? in.tau[0] : lane == 1 ? in.tau[1] : in.tau[2];
}

template <bool kDirect>
__global__ void __launch_bounds__(kWave) geo_search_kernel(const GeoScene *scenes, const int *slots, int nscenes, GeoIn in,
                                                           int max_exp, GeoOut o, GeoCell *cells_all, GeoHeapEnt *heap_all,
                                                           size_t cells_cap, unsigned *epochs, int *work) {
  __shared__ GeoHeapEnt lheap[kGeoHeapLds];
  __shared__ int sh_b;
  __shared__ int sh_res[4];  // path length, flags, expansions
  __shared__ double sh_cost;
  GeoCell *cells = cells_all + (size_t)blockIdx.x * cells_cap;
  GeoHeapEnt *gheap = heap_all + (size_t)blockIdx.x * cells_cap;
  double *pbuf = reinterpret_cast<double *>(gheap);  // the path, xy interleaved, once the search is over
  const bool lead = lane_id() == 0;
  unsigned epoch = epochs[blockIdx.x];
  for (;;) {
    if (lead) sh_b = atomicAdd(work, 1);
    __syncthreads();
    const int p = sh_b;
    __syncthreads();
    if (p >= in.list.n) break;
    // (both exits below come after the fetch's barriers and are taken by the whole workgroup: p is the same in every lane)
    const int b = in.list.request(p);
    if (b < 0) continue;  // an index outside 0 .. B - 1: skipped, its rows stay
    const int s = slots ? slots[b] : 0;
    if (s < 0 || s >= nscenes) {
      if (lead) {
        o.path_len[b] = 0;
        o.path_cost[b] = NAN;
        o.expansions[b] = 0;
        o.flags[b] = NEO_GEO_FLAG_BAD_SCENE;
      }
      geo_write_result(in, o, b, NAN);
      continue;
    }
    const GeoScene sc = scenes[s];
    if (lead) {
      const int We = sc.We, He = sc.He;
      const long long ncell = (long long)We * He;
      const GeoLookup lk(sc.m);
      const double *from = in.start + (size_t)b * in.stride, *to = in.target + (size_t)b * in.stride;
      bool oks, okt;
      const double sxd = geo_index(from[0], sc.oxe, sc.res, oks);
      const double syd = geo_index(from[1], sc.oye, sc.res, okt);
      const bool s_ok = oks && okt;
      bool okx, oky;
      const double txd = geo_index(to[0], sc.oxe, sc.res, okx);
      const double tyd = geo_index(to[1], sc.oye, sc.res, oky);
      const bool t_ok = okx && oky;
      const int sx = s_ok ? (int)sxd : 0, sy = s_ok ? (int)syd : 0;
      const int tx = t_ok ? (int)txd : 0, ty = t_ok ? (int)tyd : 0;
      const long long skey = (long long)sx + (long long)sy * We;
      const long long tkey = (long long)tx + (long long)ty * We;
      const bool t_in = t_ok && tx >= 0 && tx < We && ty >= 0 && ty < He;
      int flags = 0, len = 1, nexp = 0;
      double cost = 0.0;
      bool found = false;
      if (s_ok && t_ok && sx == tx && sy == ty) {
        found = true;  // start == target: the path is the target cell, cost 0
      } else if (!s_ok || skey < 0 || skey >= ncell) {
        flags = NEO_GEO_FLAG_START_OUTSIDE;
      } else if (!t_in || (kDirect ? geo_cell_blocked(lk, sc.oxe, sc.oye, sc.res, tx, ty)
                                   : (((sc.mask[tkey >> 5] >> (tkey & 31)) & 1u) != 0))) {
        flags = NEO_GEO_FLAG_NO_PATH;  // unreachable: only in-range, free cells ever enter the open set
      } else {
        epoch = epoch + 1;
        const unsigned ep = epoch << 5;
        GeoHeapEnt *h = lheap;
        int n = 0, seq = 0;
        bool in_lds = true;
        auto set_pos = [&](int pos, const GeoHeapEnt &e) {
          h[pos] = e;
          cells[e.key].hpos = pos;
        };
        auto sift_up = [&](int pos, const GeoHeapEnt &e) {
          while (pos > 0) {
            const int p = (pos - 1) >> 1;
            const GeoHeapEnt pe = h[p];
            if (!geo_less(e, pe)) break;
            set_pos(pos, pe);
            pos = p;
          }
          set_pos(pos, e);
        };
        {
          const int k0 = (int)skey;
          cells[k0].g = 0.0;
          cells[k0].tag = ep | (kGeoOpen << 3);
          sift_up(n++, GeoHeapEnt{0.0 + geo_hypot((long long)sx - tx, (long long)sy - ty), seq++, k0});
        }
        bool first = true;
        for (;;) {
          if (n == 0) {
            flags = NEO_GEO_FLAG_NO_PATH;
            break;
          }
          const GeoHeapEnt top = h[0];
          const int cx = first ? sx : top.key % We, cy = first ? sy : top.key / We;
          first = false;
          if (cx == tx && cy == ty) {
            found = true;
            cost = cells[top.key].g;
            break;
          }
          if (max_exp > 0 && nexp >= max_exp) {
            flags = NEO_GEO_FLAG_CAPPED;
            break;
          }
          // pop
          {
            const GeoHeapEnt e = h[--n];
            if (n > 0) {
              int pos = 0;
              for (;;) {
                int ch = 2 * pos + 1;
                if (ch >= n) break;
                GeoHeapEnt ce = h[ch];
                if (ch + 1 < n) {
                  const GeoHeapEnt c2 = h[ch + 1];
                  if (geo_less(c2, ce)) { ce = c2; ++ch; }
                }
                if (!geo_less(ce, e)) break;
                set_pos(pos, ce);
                pos = ch;
              }
              set_pos(pos, e);
            }
          }
          GeoCell &cur = cells[top.key];
          const double gc = cur.g;
          cur.tag = ep | (kGeoClosed << 3) | (cur.tag & 7u);
          ++nexp;
          // the eight neighbours: all gathers first, then the updates in motion-model order
          // (masked: eight mask words; direct: eight map records)
          long long nk[8];
          bool ok[8];
          unsigned mw[8], tg[8];
          double gn[8];
          GeoLookup::Addr ma[8];
          GeoLookup::Raw mq[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int nx = cx + geo_mdx(j), ny = cy + geo_mdy(j);
            ok[j] = nx >= 0 && nx < We && ny >= 0 && ny < He;
            nk[j] = ok[j] ? (long long)nx + (long long)ny * We : 0;
            if constexpr (kDirect) {
              ma[j] = geo_cell_addr(lk, sc.oxe, sc.oye, sc.res, nx, ny, ok[j]);
              mq[j] = lk.load(ma[j]);
            } else {
              mw[j] = sc.mask[nk[j] >> 5];
            }
            tg[j] = cells[nk[j]].tag;
            gn[j] = cells[nk[j]].g;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            bool blocked;
            if constexpr (kDirect) blocked = geo_blocked_from(lk, ma[j], mq[j]);
            else blocked = ((mw[j] >> (nk[j] & 31)) & 1u) != 0;
            if (!ok[j] || blocked) continue;
            const bool cur_ep = (tg[j] >> 5) == epoch;
            const unsigned st = cur_ep ? (tg[j] >> 3) & 3u : 0u;
            if (st == kGeoClosed) continue;
            const double ng = gc + (j < 4 ? 1.0 : 1.4142135623730951);  // math.sqrt(2)
            const int k = (int)nk[j];
            const double f = ng + geo_hypot((long long)(k % We) - tx, (long long)(k / We) - ty);
            if (st != kGeoOpen) {
              if (in_lds && n == kGeoHeapLds) {  // outgrown its LDS share: the heap moves to the slot's global heap
                for (int i = 0; i < n; ++i) gheap[i] = lheap[i];
                h = gheap;
                in_lds = false;
              }
              cells[k].g = ng;
              cells[k].tag = ep | (kGeoOpen << 3) | (unsigned)j;
              sift_up(n++, GeoHeapEnt{f, seq++, k});
            } else if (gn[j] > ng) {  // decrease-key: the entry keeps its seq
              cells[k].g = ng;
              cells[k].tag = ep | (kGeoOpen << 3) | (unsigned)j;
              const int pos = cells[k].hpos;
              sift_up(pos, GeoHeapEnt{f, h[pos].seq, k});
            }
          }
        }
      }
      // the path into pbuf: the target cell, then its parents back to the start (retrieve_final_path)
      if (found && !(sx == tx && sy == ty)) {
        int x = tx, y = ty;
        len = 1;
        // (a path visits distinct cells: at most ncell nodes, which pbuf holds; the bounds only guard the buffers)
        while (!(x == sx && y == sy) && len < ncell && x >= 0 && x < We && y >= 0 && y < He) {
          const unsigned d = cells[(long long)x + (long long)y * We].tag & 7u;
          x -= geo_mdx((int)d);
          y -= geo_mdy((int)d);
          ++len;
        }
        x = tx;
        y = ty;
        for (int i = len - 1; i >= 0; --i) {
          pbuf[2 * i] = geo_real(sc.oxe, (double)x, sc.res);
          pbuf[2 * i + 1] = geo_real(sc.oye, (double)y, sc.res);
          if (i > 0 && x >= 0 && x < We && y >= 0 && y < He) {
            const unsigned d = cells[(long long)x + (long long)y * We].tag & 7u;
            x -= geo_mdx((int)d);
            y -= geo_mdy((int)d);
          }
        }
      } else {
        len = 1;  // start == target, or no path: [calc_real_pos(target cell)], cost 0
        pbuf[0] = geo_real(sc.oxe, txd, sc.res);
        pbuf[1] = geo_real(sc.oye, tyd, sc.res);
        cost = 0.0;
      }
      if (o.path) {
        const int nc = len < o.path_cap ? len : o.path_cap;
        for (int i = 0; i < 2 * nc; ++i) o.path[(size_t)b * o.path_cap * 2 + i] = pbuf[i];
        if (len > o.path_cap) flags |= NEO_GEO_FLAG_PATH_TRUNCATED;
      }
      sh_res[0] = len;
      sh_res[1] = flags;
      sh_res[2] = nexp;
      sh_cost = cost;
      __threadfence();  // pbuf: lane 0's stores before the other lanes' loads
    }
    __syncthreads();
    __threadfence();
    const int len = sh_res[0];
    int idx[4];
    geo_prune(sc.m, pbuf, len, idx);
    geo_write_result(in, o, b, lane_id() < 8 ? pbuf[2 * idx[lane_id() >> 1] + (lane_id() & 1)] : 0.0);
    if (o.path)  // rows past the path: NaN
      for (int i = 2 * len + lane_id(); i < 2 * o.path_cap; i += kWave) o.path[(size_t)b * o.path_cap * 2 + i] = NAN;
    if (lead) {
      o.path_len[b] = len;
      o.flags[b] = sh_res[1];
      o.expansions[b] = sh_res[2];
      o.path_cost[b] = sh_cost;
    }
    __syncthreads();
  }
  if (lead) epochs[blockIdx.x] = epoch;
}

}  // namespace neo
