// rtmi_accel_build.cpp — the CPU half of the RTIOW acceleration structures:
// everything rt_ctx_set_scene (rtmi_device.hip) uploads for a scene is built
// here (build_accel: the float and double records, the big / small split, the
// BVH, the uniform grid, the tile lists' table, the grid's global-memory
// image), and the validation entry points rt_debug_grid_*, rt_debug_tile_* and
// rt_debug_accel_digest run the same builders without a device.  No HIP call:
// the file is plain C++ (rtmi_accel.h holds what it shares with the kernels),
// so tests/native/host_sanitize.cpp drives it under ASan + UBSan.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rtmi_internal.h"

namespace rtmi {
namespace {

// The records of the scene's spheres and materials (AccelBuild g .. s164)
int scene_records(const rt_scene *scene, AccelBuild &out) {
  const int n = scene->n;
  out.g.assign(size_t(n) + kGeomPad, Rec4{0.f, 0.f, 0.f, 0.f});
  out.s0.resize(n); out.s1.resize(n);
  out.g64.resize(n); out.s064.resize(n); out.s164.resize(n);
  for (int k = 0; k < n; k++) {
    const double *c = scene->center_radius + 4 * k;
    const double *m = scene->mat_params + 4 * k;
    const int kind = scene->mat_kind[k];
    if (kind < RT_MAT_LAMBERTIAN || kind > RT_MAT_DIELECTRIC)
      return set_error(RT_EUNSUPPORTED, "object %d: unsupported material kind %d", k, kind);
    const double fuzz = m[3] < 1 ? m[3] : 1;  // metal ctor material.h:39
    const float r = float(c[3]), ir = float(m[3]);
    // S = |c|^2 - r^2 of the float-rounded sphere, in double then rounded
    // (the oracle computes the identical expression)
    const float cx = float(c[0]), cy = float(c[1]), cz = float(c[2]);
    const float S = float(double(cx) * cx + double(cy) * cy + double(cz) * cz - double(r) * r);
    out.g[k] = Rec4{cx, cy, cz, S};
    out.s0[k] = Rec4{1.0f / r, float(m[0]), float(m[1]), float(m[2])};
    out.s1[k] = Rec4{float(kind), float(fuzz), ir, 1.0f / ir};
    if (kind == RT_MAT_DIELECTRIC) {
      // Schlick's r0 for both faces (material.h:91-96), in the float
      // arithmetic the kernels would repeat per scatter: front (ratio 1/ir)
      // in shade1.y, back (ratio ir) in shade0.y — fields a dielectric does
      // not otherwise read (no albedo, no fuzz)
      auto r0_of = [](float x) {
        const float q = (1.0f - x) / (1.0f + x);
        return q * q;
      };
      out.s1[k].y = r0_of(1.0f / ir);
      out.s0[k].y = r0_of(ir);
    }
    out.g64[k] = Rec4d{c[0], c[1], c[2], c[3] * c[3]};
    out.s064[k] = Rec4d{1 / c[3], m[0], m[1], m[2]};
    out.s164[k] = Rec4d{double(kind), fuzz, m[3], 1.0 / m[3]};
  }
  return RT_OK;
}

// The box margins of the structures: sphere k's is 1e-3 of its own coordinate
// scale (~100x the float error of its hit test) plus 1e-6 of the whole
// scene's (rays from far away)
struct Margins {
  const double *cr;
  double scene;
  double of(int32_t k) const {
    const double *c = cr + 4 * k;
    const double own = std::max(std::max(std::fabs(c[0]), std::fabs(c[1])), std::fabs(c[2])) + std::fabs(c[3]);
    return 1e-3 * (1.0 + own) + scene;
  }
  double grown(int32_t k) const { return std::fabs(cr[4 * k + 3]) + of(k); }  // the radius its boxes and cells use
};

// Spheres much larger than the typical one (the ground) stay brute force: the
// big / small split, the big spheres' padded slots (out.big_slots), and the
// margins from the whole scene's scale, big spheres included
Margins split_scene(const rt_scene *scene, std::vector<int32_t> &small, AccelBuild &out) {
  const int n = scene->n;
  std::vector<double> rad(n);
  for (int k = 0; k < n; k++) rad[k] = std::fabs(scene->center_radius[4 * k + 3]);
  std::vector<double> sorted_r = rad;
  std::nth_element(sorted_r.begin(), sorted_r.begin() + n / 2, sorted_r.end());
  const double med = sorted_r[n / 2];
  double scale = 0;
  out.big_slots.clear();
  for (int k = 0; k < n; k++) {
    (rad[k] > RTMI_BIG_FACTOR * med ? out.big_slots : small).push_back(k);  // ascending scene index
    for (int a = 0; a < 3; ++a) scale = std::max(scale, std::fabs(scene->center_radius[4 * k + a]) + rad[k]);
  }
  out.nbig = int32_t(out.big_slots.size());
  out.big_slots.resize((out.big_slots.size() + 2 * kBigGroup - 1) / (2 * kBigGroup) * (2 * kBigGroup), -1);
  return Margins{scene->center_radius, 1e-6 * scale};
}

// BVH over the small spheres: binary, SAH split (full sweep of the sorted
// centroids on each axis: the split minimising area(L)*|L| + area(R)*|R|),
// leaves of <= kLeafMax spheres, nodes in DFS order with skip links.  Boxes
// are the spheres' double-precision bounds, each grown by its own margin
// (Margins) and rounded outward to half precision, so every sphere the float
// test can report lies strictly inside its leaf's box.
uint16_t half_bits(_Float16 h) { return __builtin_bit_cast(uint16_t, h); }
// largest half <= v (-inf below the half range)
uint16_t half_down(double v) {
  _Float16 h = _Float16(v);
  while (double(h) > v) {
    uint16_t b = half_bits(h);
    if (b == 0x0000) b = 0x8001;          // +0 -> -min denormal
    else if (b & 0x8000) b = uint16_t(b + 1);  // negative: away from zero
    else b = uint16_t(b - 1);             // positive: toward zero
    h = __builtin_bit_cast(_Float16, b);
  }
  return half_bits(h);
}
uint16_t half_up(double v) { return uint16_t(half_down(-v) ^ 0x8000); }

struct BvhBuilder {
  const Margins m;
  const std::vector<Rec4> &g;
  std::vector<BvhNode> &nodes;
  std::vector<Rec4> &sph;
  std::vector<int32_t> &idx;

  struct Box {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void add(const double *c, double rr) {
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], c[a] - rr);
        hi[a] = std::max(hi[a], c[a] + rr);
      }
    }
    double area() const {
      const double e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
      return e0 * e1 + e1 * e2 + e0 * e2;
    }
  };
  void grow(Box &b, int32_t k) const { b.add(m.cr + 4 * k, m.grown(k)); }
  void sort_axis(int32_t *ids, int cnt, int ax) const {
    const double *cr = m.cr;
    std::sort(ids, ids + cnt, [&](int32_t x, int32_t y) {
      const double cx = cr[4 * x + ax], cy = cr[4 * y + ax];
      return cx < cy || (cx == cy && x < y);
    });
  }
  void build(int32_t *ids, int cnt) {
    const int me = int(nodes.size());
    nodes.push_back(BvhNode{});
    Box bb;
    for (int i = 0; i < cnt; ++i) grow(bb, ids[i]);
    BvhNode nd{};
    nd.x = uint32_t(half_down(bb.lo[0])) | uint32_t(half_up(bb.hi[0])) << 16;
    nd.y = uint32_t(half_down(bb.lo[1])) | uint32_t(half_up(bb.hi[1])) << 16;
    nd.z = uint32_t(half_down(bb.lo[2])) | uint32_t(half_up(bb.hi[2])) << 16;
    if (cnt <= kLeafMax) {
      nd.link = ~((int32_t(sph.size()) << 4) | cnt);
      for (int i = 0; i < cnt; ++i) {
        sph.push_back(g[ids[i]]);
        idx.push_back(ids[i]);
      }
    } else {
      // SAH sweep: prefix/suffix boxes over the centroid order of each axis
      double best = INFINITY;
      int best_ax = 0, best_mid = cnt / 2;
      std::vector<double> left_cost(cnt);
      for (int ax = 0; ax < 3; ++ax) {
        sort_axis(ids, cnt, ax);
        Box l;
        for (int i = 1; i < cnt; ++i) {
          grow(l, ids[i - 1]);
          left_cost[i] = l.area() * i;
        }
        Box r;
        for (int i = cnt - 1; i >= 1; --i) {
          grow(r, ids[i]);
          const double c = left_cost[i] + r.area() * (cnt - i);
          if (c < best) { best = c; best_ax = ax; best_mid = i; }
        }
      }
      sort_axis(ids, cnt, best_ax);
      build(ids, best_mid);
      build(ids + best_mid, cnt - best_mid);
      nd.link = int32_t(nodes.size());
    }
    nodes[me] = nd;
  }
};

// a double rounded up to float
float float_up(double v) {
  float f = float(v);
  if (double(f) < v) f = std::nextafter(f, INFINITY);
  return f;
}

// Uniform grid over the small spheres.  The box of their
// margin-grown boxes (the BVH's margins) is cut into cells of about
// RTMI_GRID_CELLS (default 0.3) cells per sphere, as near cubic as the box
// allows (the final scene's thin layer of spheres: 30 x 1 x 30 cells); every
// sphere is listed in every cell its grown box overlaps.  Cell boundaries are
// the float values g0 + c*h the device computes, so host and device agree to
// a rounding error far below the margins.  Fills out.grid, cells, refs and the
// tile table (out.big_slots: the slots before the cells'); false: no grid.
bool build_grid(const Margins &m, const std::vector<int32_t> &small, int32_t n, AccelBuild &out) {
  if (small.empty() || n > 65535) return false;  // references are 16-bit scene indices
  const int32_t nbig_slots = int32_t(out.big_slots.size());
  const char *env = std::getenv("RTMI_GRID_CELLS");
  // 0.3 cells per sphere: config 2 33.3 ms (0.2: 33.3, 0.5: 33.6, 1: 34.5,
  // 2: 35.2, 4: 38.0; round 2) and, on the record slots, 19.30 ms (0.2:
  // 19.38, 0.25: 19.33, 0.4: 19.33; profiles/r04/grid_density.txt)
  const double per_sphere = env && std::atof(env) > 0 ? std::atof(env) : 0.3;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int32_t k : small) {
    const double *c = m.cr + 4 * k, R = m.grown(k);
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], c[a] - R);
      hi[a] = std::max(hi[a], c[a] + R);
    }
  }
  double e[3], vol = 1;
  for (int a = 0; a < 3; ++a) {
    e[a] = std::max(hi[a] - lo[a], 1e-6 * (1 + std::fabs(lo[a])));
    vol *= e[a];
  }
  const double cell = std::cbrt(vol / (per_sphere * double(small.size())));
  // analysis knob: RTMI_GRID_ASPECT = x-cell / z-cell size ratio (1: cubic)
  const char *asp_env = std::getenv("RTMI_GRID_ASPECT");
  const double asp = asp_env && std::atof(asp_env) > 0 ? std::atof(asp_env) : 1.0;
  const double cell_a[3] = {cell * std::sqrt(asp), cell, cell / std::sqrt(asp)};
  GridDesc d{};
  int64_t total = 1;
  for (int a = 0; a < 3; ++a) {
    d.n[a] = int32_t(std::min<double>(128, std::max<double>(1, std::ceil(e[a] / cell_a[a]))));
    total *= d.n[a];
  }
  if (total > 16384) return false;
  for (int a = 0; a < 3; ++a) {
    // origin rounded down, cell size rounded up: the float cells cover the box
    float g0 = float(lo[a]);
    if (double(g0) > lo[a]) g0 = std::nextafter(g0, -INFINITY);
    float h = float(e[a] / d.n[a]);
    while (double(g0) + double(h) * d.n[a] < hi[a]) h = std::nextafter(h, INFINITY);
    d.g0[a] = g0;
    d.h[a] = h;
    d.inv_h[a] = 1.0f / h;
    d.g1[a] = std::fmaf(float(d.n[a]), h, g0);
  }
  d.ncells = int32_t(total);
  if (!grid_strides(d)) return false;  // (never at <= 128 cells per axis; the walk's 24-bit multiplies rest on it)
  std::vector<std::vector<uint16_t>> lists(static_cast<size_t>(total));
  for (int32_t k : small) {  // ascending scene index
    const double *c = m.cr + 4 * k, R = m.grown(k);
    int c0[3], c1[3];
    for (int a = 0; a < 3; ++a) {
      // cell c spans [g0 + c*h, g0 + (c+1)*h]: every cell the grown box touches
      const double g0 = d.g0[a], h = d.h[a];
      c0[a] = std::max(0, std::min(d.n[a] - 1, int(std::floor((c[a] - R - g0) / h))));
      c1[a] = std::max(0, std::min(d.n[a] - 1, int(std::floor((c[a] + R - g0) / h))));
    }
    for (int z = c0[2]; z <= c1[2]; ++z)
      for (int y = c0[1]; y <= c1[1]; ++y)
        for (int x = c0[0]; x <= c1[0]; ++x)
          lists[size_t(x + d.n[0] * (y + d.n[1] * z))].push_back(uint16_t(k));
  }
  out.cells.assign(size_t(total) + 1, 0);
  out.refs.clear();
  for (int64_t cidx = 0; cidx < total; ++cidx) {
    out.cells[size_t(cidx)] = uint32_t(out.refs.size());
    for (uint16_t k : lists[size_t(cidx)]) out.refs.push_back(uint32_t(k) * 16u);
  }
  out.cells[size_t(total)] = uint32_t(out.refs.size());
  d.nrefs = int32_t(out.refs.size());
  d.cells_off = 16u * uint32_t(nbig_slots + d.nrefs);  // grid_lds_bytes' layout
  d.idx_off = d.cells_off + 4u * uint32_t(d.ncells + 1);
  out.grid = d;
  // The tile lists' table: the sphere with the radius the grid's cells list it
  // by (its own margin, 1e-3 of its coordinate scale: the same distance from
  // float error), rounded up, and the first record slot that holds it.
  out.tile_tab.clear();
  out.ntile = out.ntile_big = 0;
  if (size_t(nbig_slots) + out.refs.size() <= 65536) {
    std::vector<uint32_t> first(size_t(n), UINT32_MAX);
    for (size_t p = out.refs.size(); p-- > 0;) first[out.refs[p] >> 4] = uint32_t(nbig_slots) + uint32_t(p);
    const size_t ns = small.size(), nk = (ns + 3) / 4, nb = out.nbig <= kTileBigMax ? size_t(out.nbig) : 0;
    out.tile_tab.assign(ns + nk + nb, Rec4{0.f, 0.f, 0.f, 0.f});
    for (size_t i = 0; i < ns; ++i) {
      const int32_t k = small[i];
      const double *c = m.cr + 4 * k;
      out.tile_tab[i] = Rec4{float(c[0]), float(c[1]), float(c[2]), float_up(m.grown(k))};
      std::memcpy(reinterpret_cast<char *>(&out.tile_tab[ns]) + 4 * i, &first[size_t(k)], 4);
    }
    // The big slots by the same rule on the sphere's own scale: 1e-3 of its
    // radius — 1 unit on the R = 1000 ground, where the cells' margin, which
    // counts the centre's distance too, gives 2 and lifts the horizon over
    // another 6 % of config 2's tiles — and 1e-5 of its centre's coordinates,
    // 100 times their float spacing, which is what the centre's rounding and
    // tile_may_hit's differences from it can be off by (on the ground 1e-4).
    for (size_t s = 0; s < nb; ++s) {  // ascending scene index: slot order
      const double *c = m.cr + 4 * out.big_slots[s];
      const double cmax = std::max(std::max(std::fabs(c[0]), std::fabs(c[1])), std::fabs(c[2]));
      const double R = std::fabs(c[3]) + 1e-3 * (1.0 + std::fabs(c[3])) + 1e-5 * cmax + m.scene;
      out.tile_tab[ns + nk + s] = Rec4{float(c[0]), float(c[1]), float(c[2]), float_up(R)};
    }
    out.ntile = int32_t(ns);
    out.ntile_big = int32_t(nb);
  }
  return true;
}

// record slot (offset from the first slot / 16) of tile-table sphere i
uint32_t tile_key(const AccelBuild &ab, size_t i) {
  uint32_t key;
  std::memcpy(&key, reinterpret_cast<const char *>(&ab.tile_tab[size_t(ab.ntile)]) + 4 * i, 4);
  return key;
}

// The grid rt_ctx_set_scene builds for a scene and its tile table, without
// the records and the BVH (false: the scene has none)
bool grid_only(const rt_scene *scene, AccelBuild &ab) {
  std::vector<int32_t> small;
  const Margins m = split_scene(scene, small, ab);
  return ab.has_grid = build_grid(m, small, scene->n, ab);
}

}  // namespace

int build_accel(const rt_scene *scene, AccelBuild &out) {
  out = AccelBuild{};
  if (int rc = scene_records(scene, out)) return rc;
  std::vector<int32_t> small;
  const Margins m = split_scene(scene, small, out);
  BvhBuilder b{m, out.g, out.nodes, out.bvh_sph, out.bvh_idx};
  if (!small.empty()) b.build(small.data(), int(small.size()));
  out.has_grid = build_grid(m, small, scene->n, out);
  return RT_OK;
}

std::vector<char> grid_image(const AccelBuild &ab) {
  // the slots (big spheres, then every cell's references as copies of their
  // spheres' records), the cell starts, the slots' scene indices
  const int32_t nbs = int32_t(ab.big_slots.size()), nrec = nbs + ab.grid.nrefs;
  std::vector<char> img(grid_lds_bytes(nbs, ab.grid.ncells, ab.grid.nrefs), 0);
  Rec4 *rec = reinterpret_cast<Rec4 *>(img.data());
  uint32_t *cst = reinterpret_cast<uint32_t *>(img.data() + ab.grid.cells_off);
  uint16_t *ix = reinterpret_cast<uint16_t *>(img.data() + ab.grid.idx_off);
  for (int32_t i = 0; i < nrec; ++i) {
    const int32_t k = i < nbs ? ab.big_slots[size_t(i)] : int32_t(ab.refs[size_t(i - nbs)] >> 4);  // dummies: -1
    rec[i] = k < 0 ? Rec4{0.f, 0.f, 0.f, 0.f} : ab.g[size_t(k)];
    ix[i] = uint16_t(k < 0 ? 0 : k);
  }
  for (int32_t i = 0; i <= ab.grid.ncells; ++i) cst[i] = 16u * (uint32_t(nbs) + ab.cells[size_t(i)]);
  return img;
}

}  // namespace rtmi

using namespace rtmi;

// Validation entry points (host only, no device): the cell-start strides
// grid_strides gives a grid of n3 cells per axis, or RT_EINVAL where it
// refuses the grid; and the cell counts and strides of the descriptor
// build_grid fills for a scene (the split into big and small spheres as in
// rt_ctx_set_scene), with its origin and cell size (box6, optional).
RTMI_EXPORT int rt_debug_grid_strides(const int32_t *n3, uint32_t *strides2) {
  if (!n3 || !strides2) return set_error(RT_EINVAL, "rt_debug_grid_strides: bad argument");
  GridDesc d{};
  for (int a = 0; a < 3; ++a) d.n[a] = n3[a];
  if (!grid_strides(d)) return set_error(RT_EINVAL, "grid of %d x %d x %d cells: over the walk's 24-bit bound", n3[0], n3[1], n3[2]);
  strides2[0] = d.row_bytes;
  strides2[1] = d.layer_bytes;
  return RT_OK;
}

RTMI_EXPORT int rt_debug_grid_layout(const rt_scene *scene, int32_t *dims3, uint32_t *strides2, float *box6) {
  if (!scene || scene->n <= 0 || !scene->center_radius || !dims3 || !strides2)
    return set_error(RT_EINVAL, "rt_debug_grid_layout: bad argument");
  AccelBuild ab;
  if (!grid_only(scene, ab)) return set_error(RT_EUNSUPPORTED, "no grid for this scene");
  for (int a = 0; a < 3; ++a) dims3[a] = ab.grid.n[a];
  strides2[0] = ab.grid.row_bytes;
  strides2[1] = ab.grid.layer_bytes;
  if (box6)  // the grid's origin and cell size, as the walk reads them
    for (int a = 0; a < 3; ++a) {
      box6[a] = ab.grid.g0[a];
      box6[3 + a] = ab.grid.h[a];
    }
  return RT_OK;
}

namespace {
// The argument checks and the tile loop of rt_debug_tile_list and
// rt_debug_tile_big: each(ab, tb, o) for tile `tile` (o = 0), or for every
// tile of the strip (tile -1; o the tile)
template <class Each>
int for_tiles(const char *who, const rt_scene *scene, const rt_camera *camera, int32_t W, int32_t H, int32_t row0,
              int32_t row_step, int32_t nrows, int32_t tile_w, int32_t tile, int32_t cap, const int32_t *out_indices,
              const int32_t *out_count, Each each) {
  if (!scene || scene->n <= 0 || !scene->center_radius || !camera || !out_indices || !out_count)
    return set_error(RT_EINVAL, "%s: bad argument", who);
  if (W < 2 || H < 2 || row0 < 0 || row0 >= H || row_step < 1 || nrows < 1 || cap < 1 || cap > kTileListCap ||
      (tile_w != 0 && tile_w != 8 && tile_w != 16 && tile_w != 32 && tile_w != 64))
    return set_error(RT_EINVAL, "%s: bad image, strip, tile shape or cap", who);
  const int32_t nvalid = int32_t(std::min<int64_t>(nrows, (int64_t(H) - row0 + row_step - 1) / row_step));
  const int32_t tw = tile_w ? tile_w : auto_tile_w(W, nvalid), th = 64 / tw;
  const int64_t tiles = int64_t((W + tw - 1) / tw) * ((nvalid + th - 1) / th);
  if (tile < -1 || tile >= tiles) return set_error(RT_EINVAL, "%s: tile %d of %lld", who, tile, (long long)tiles);
  AccelBuild ab;
  if (!grid_only(scene, ab) || ab.ntile == 0) return set_error(RT_EUNSUPPORTED, "no tile lists for this scene");
  const Cam<float> cam = cam_f(camera);
  for (int64_t t = tile < 0 ? 0 : tile, o = 0; t < (tile < 0 ? tiles : tile + 1); ++t, ++o) {
    int32_t x0, vw, j_lo, j_hi;
    tile_extent(W, row0, row_step, nvalid, tw, int32_t(t), x0, vw, j_lo, j_hi);
    each(ab, tile_bundle(cam, W, H, x0, vw, j_lo, j_hi), o);
  }
  return RT_OK;
}
}  // namespace

// Validation entry point (host only, no device): the tile lists render_kernel
// builds, by the same tile_bundle / tile_may_hit, for the
// strip of rows row0 + r row_step, r < nrows, of a W x H image in tiles of
// tile_w x 64 / tile_w (0: the automatic shape).  tile >= 0: that tile's list
// as scene indices in out_indices[cap] and its length in out_count[0]; tile
// -1: every tile's, cap entries and one count each.  A count of -1: more than
// cap spheres pass, the tile has no list (its batches walk the grid).
RTMI_EXPORT int rt_debug_tile_list(const rt_scene *scene, const rt_camera *camera, int32_t W, int32_t H, int32_t row0,
                                   int32_t row_step, int32_t nrows, int32_t tile_w, int32_t tile, int32_t cap,
                                   int32_t *out_indices, int32_t *out_count) {
  return for_tiles("rt_debug_tile_list", scene, camera, W, H, row0, row_step, nrows, tile_w, tile, cap, out_indices,
                   out_count, [&](const AccelBuild &ab, const TileBundle &tb, int64_t o) {
                     const uint32_t nbs = uint32_t(ab.big_slots.size());
                     int32_t cnt = 0;
                     for (size_t i = 0; i < size_t(ab.ntile); ++i) {
                       const Rec4 s = ab.tile_tab[i];
                       if (!tile_may_hit(tb, s.x, s.y, s.z, s.w)) continue;
                       // the key names a record slot; the slot's reference names the sphere
                       if (cnt < cap) out_indices[o * cap + cnt] = int32_t(ab.refs[tile_key(ab, i) - nbs] >> 4);
                       ++cnt;
                     }
                     out_count[o] = cnt <= cap ? cnt : -1;
                   });
}

// The same for the big spheres (the same host code; rt_debug_tile_list stays
// the small spheres alone): the big spheres the kernel appends to the tile's
// list, as scene indices in out_indices[kTileBigMax] per tile and their number
// in out_count.  A count of -1 for every tile: the scene has more than
// kTileBigMax big spheres and its lists name none (every batch runs hit_big).
// (The kernel appends them where the tile has a list and the list's 32
// entries hold both; RTMI_TILE_BIG is not read here.)
RTMI_EXPORT int rt_debug_tile_big(const rt_scene *scene, const rt_camera *camera, int32_t W, int32_t H, int32_t row0,
                                  int32_t row_step, int32_t nrows, int32_t tile_w, int32_t tile, int32_t *out_indices,
                                  int32_t *out_count) {
  return for_tiles("rt_debug_tile_big", scene, camera, W, H, row0, row_step, nrows, tile_w, tile, kTileBigMax,
                   out_indices, out_count, [&](const AccelBuild &ab, const TileBundle &tb, int64_t o) {
                     const Rec4 *big = ab.tile_tab.data() + ab.ntile + (ab.ntile + 3) / 4;
                     int32_t cnt = 0;
                     for (int32_t i = 0; i < ab.ntile_big; ++i)
                       if (tile_may_hit(tb, big[i].x, big[i].y, big[i].z, big[i].w))
                         out_indices[o * kTileBigMax + cnt++] = ab.big_slots[size_t(i)];
                     out_count[o] = ab.nbig > kTileBigMax ? -1 : cnt;
                   });
}

// Validation entry point (host only, no device): one FNV-1a-64 per array
// build_accel gives for the scene, so that a change of a builder shows as the
// array it moved (tests/test_accel_digest.py).  out[0] the big slots' index
// table, [1] the BVH nodes, [2] its leaf records then indices, [3] whether the
// scene has a grid and the descriptor's scalars field by field (the struct has
// pointers and padding), [4] cells, [5] refs, [6] the tile table, [7] the
// global-memory grid image; [4]-[7] of a scene without a grid, and [6] of one
// without a table, hash nothing.
RTMI_EXPORT int rt_debug_accel_digest(const rt_scene *scene, uint64_t *out) {
  if (!scene || scene->n <= 0 || !scene->center_radius || !scene->mat_kind || !scene->mat_params || !out)
    return set_error(RT_EINVAL, "rt_debug_accel_digest: bad argument");
  AccelBuild ab;
  if (int rc = build_accel(scene, ab)) return rc;
  auto hash = [](const auto &v) { return fnv1a(kFnvBasis, v.data(), v.size() * sizeof(v[0])); };
  out[0] = hash(ab.big_slots);
  out[1] = hash(ab.nodes);
  out[2] = fnv1a(hash(ab.bvh_sph), ab.bvh_idx.data(), ab.bvh_idx.size() * sizeof(int32_t));
  const int32_t ok = ab.has_grid;
  uint64_t h = fnv1a(kFnvBasis, &ok, sizeof ok);
  out[4] = out[5] = out[6] = out[7] = kFnvBasis;
  if (ok) {
    const GridDesc &d = ab.grid;
    h = fnv1a(h, d.g0, sizeof d.g0); h = fnv1a(h, d.h, sizeof d.h); h = fnv1a(h, d.inv_h, sizeof d.inv_h);
    h = fnv1a(h, d.g1, sizeof d.g1); h = fnv1a(h, d.n, sizeof d.n); h = fnv1a(h, &d.ncells, sizeof d.ncells);
    h = fnv1a(h, &d.nrefs, sizeof d.nrefs); h = fnv1a(h, &d.cells_off, sizeof d.cells_off);
    h = fnv1a(h, &d.idx_off, sizeof d.idx_off); h = fnv1a(h, &d.row_bytes, sizeof d.row_bytes);
    h = fnv1a(h, &d.layer_bytes, sizeof d.layer_bytes); h = fnv1a(h, d.nm1, sizeof d.nm1);
    out[4] = hash(ab.cells);
    out[5] = hash(ab.refs);
    out[6] = hash(ab.tile_tab);
    out[7] = hash(grid_image(ab));
  }
  out[3] = h;
  return RT_OK;
}
