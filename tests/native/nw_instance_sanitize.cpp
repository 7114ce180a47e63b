// nw_instance_sanitize.cpp — stand-alone driver of tests/test_nw_instance.py's
// sanitizer run: rt_nw_shared and the two-level build of build_device_scene
// (rtmi_nw_scene.cpp) under ASan + UBSan (host code only, no device), with the
// structure the gfx950 walk relies on checked link by link:
//  - every bottom-level node's box contains the vertices of the triangles
//    below it; every skip link and leaf range lies inside its mesh's ranges;
//  - every placement's top-level box contains the mesh's vertices under the
//    placement's transform, and the placement is alone in its leaf;
//  - pool slot -> triangle number is a bijection onto the mesh's hittable
//    triangles, and the flat view is the expansion.
//   nw_instance_sanitize
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../a_dive_into_ray_tracing_amd/csrc/rtmi_nw_internal.h"

using namespace rtmi::nw;

#define CHECK(cond)                                                                                        \
  do {                                                                                                     \
    if (!(cond)) {                                                                                         \
      std::fprintf(stderr, "%s:%d: check failed: %s (%s)\n", __FILE__, __LINE__, #cond, rt_last_error()); \
      std::exit(1);                                                                                        \
    }                                                                                                      \
  } while (0)

// icosphere of 20 * 4^subdiv triangles, radius 1.7 about (0.3, -0.2, 0.9)
static void icosphere(int subdiv, std::vector<double> &v, std::vector<int32_t> &f) {
  const double p = (1.0 + std::sqrt(5.0)) / 2.0;
  const double base[12][3] = {{-1, p, 0}, {1, p, 0}, {-1, -p, 0}, {1, -p, 0}, {0, -1, p}, {0, 1, p},
                              {0, -1, -p}, {0, 1, -p}, {p, 0, -1}, {p, 0, 1}, {-p, 0, -1}, {-p, 0, 1}};
  const int32_t faces[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                                {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                                {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  auto push = [&](double x, double y, double z) {
    const double l = std::sqrt(x * x + y * y + z * z);
    v.push_back(x / l);
    v.push_back(y / l);
    v.push_back(z / l);
    return int32_t(v.size() / 3) - 1;
  };
  v.clear();
  f.clear();
  for (auto &b : base) push(b[0], b[1], b[2]);
  for (auto &t : faces) f.insert(f.end(), t, t + 3);
  for (int s = 0; s < subdiv; ++s) {
    std::map<std::pair<int32_t, int32_t>, int32_t> mid;
    auto m = [&](int32_t a, int32_t b) {
      const auto key = std::make_pair(std::min(a, b), std::max(a, b));
      auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      const int32_t id = push(v[3 * a] + v[3 * b], v[3 * a + 1] + v[3 * b + 1], v[3 * a + 2] + v[3 * b + 2]);
      mid[key] = id;
      return id;
    };
    std::vector<int32_t> nf;
    for (size_t k = 0; k < f.size(); k += 3) {
      const int32_t a = f[k], b = f[k + 1], c = f[k + 2], ab = m(a, b), bc = m(b, c), ca = m(c, a);
      const int32_t t[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
      nf.insert(nf.end(), t, t + 12);
    }
    f.swap(nf);
  }
  const double c[3] = {0.3, -0.2, 0.9};
  for (size_t i = 0; i < v.size(); ++i) v[i] = double(float(v[i] * 1.7 + c[i % 3]));
}

struct Placed {
  bool rot, trans;
  double angle, off[3];
};

static void tri_vertices(const Obj &o, double v[3][3]) {
  const float f[9] = {o.g0[0], o.g0[1], o.g0[2], o.g0[3], o.g1[0], o.g1[1], o.g1[2], o.g1[3], o.g2[0]};
  for (int k = 0; k < 9; ++k) v[k / 3][k % 3] = f[k];
}

// Builds `mesh` placed as `where` says, shared; checks the device scene.
static void check_scene(rt_nw_scene *s, int32_t shared, int32_t n_tris, int32_t n_hittable, const std::vector<Placed> &where,
                        int32_t n_other) {
  for (const Placed &p : where) {
    int32_t h = shared;
    if (p.rot) h = rt_nw_rotate_y(s, h, p.angle);
    CHECK(h >= 0);
    if (p.trans) h = rt_nw_translate(s, h, p.off);
    CHECK(h >= 0);
    CHECK(rt_nw_world_add(s, h) == RT_OK);
  }
  rt_nw_flat fl;
  CHECK(rt_nw_scene_flat(s, &fl) == RT_OK);
  CHECK(fl.n_obj == n_other + n_tris * int32_t(where.size()));
  DeviceScene ds;
  CHECK(build_device_scene(s, ds) == RT_OK);
  CHECK(!ds.grid_ok);
  CHECK(ds.mesh.size() == 1 && ds.place_mesh.size() == where.size() && ds.place_slot.size() == where.size());
  const DeviceScene::SharedMesh &M = ds.mesh[0];
  CHECK(M.n_tris == n_tris && M.n_pool == n_hittable && M.node0 == 0 && M.pool0 == 0);
  CHECK(size_t(M.n_pool) == ds.pool.size() && ds.pool_j.size() == ds.pool.size() && size_t(M.n_nodes) == ds.bnodes.size());
  CHECK(ds.obj.size() == size_t(n_other) + where.size() && ds.obj_id.size() == ds.obj.size());
  // pool slot -> triangle number: each hittable triangle once
  std::vector<char> seen(size_t(n_tris), 0);
  for (int32_t q = 0; q < M.n_pool; ++q) {
    const int32_t j = ds.pool_j[size_t(q)];
    CHECK(j >= 0 && j < n_tris && !seen[size_t(j)]);
    seen[size_t(j)] = 1;
    CHECK(ds.pool[size_t(q)].kind == kTriangle && ds.pool[size_t(q)].inst == -1);
  }
  // bottom level: links inside the mesh, boxes over everything below
  std::vector<int32_t> covered(size_t(M.n_pool), 0);
  for (int32_t i = M.node0; i < M.node0 + M.n_nodes; ++i) {
    const Node &nd = ds.bnodes[size_t(i)];
    CHECK(nd.skip > i && nd.skip <= M.node0 + M.n_nodes);
    if (nd.leaf >= 0) {
      const int32_t first = nd.leaf >> 4, cnt = nd.leaf & 15;
      CHECK(cnt >= 1 && cnt <= kNodeLeafMax && first >= M.pool0 && first + cnt <= M.pool0 + M.n_pool);
      for (int32_t q = first; q < first + cnt; ++q) covered[size_t(q - M.pool0)] += 1;
    }
    // the leaves below node i are those of nodes [i, skip)
    for (int32_t k = i; k < nd.skip; ++k) {
      const Node &c = ds.bnodes[size_t(k)];
      if (c.leaf < 0) continue;
      for (int32_t q = c.leaf >> 4; q < (c.leaf >> 4) + (c.leaf & 15); ++q) {
        double v[3][3];
        tri_vertices(ds.pool[size_t(q)], v);
        for (int a = 0; a < 3; ++a)
          for (int w = 0; w < 3; ++w) CHECK(v[w][a] >= nd.bmin[a] && v[w][a] <= nd.bmax[a]);
      }
    }
  }
  for (int32_t c : covered) CHECK(c == 1);
  // top level: each placement's record, alone in a leaf whose box holds the transformed vertices
  for (size_t p = 0; p < where.size(); ++p) {
    const int32_t k = ds.place_slot[p];
    CHECK(k >= 0 && size_t(k) < ds.obj.size() && ds.obj[size_t(k)].kind == kInstance);
    int32_t w[4], np;
    std::memcpy(w, ds.obj[size_t(k)].g0, sizeof w);
    std::memcpy(&np, &ds.obj[size_t(k)].g1[0], 4);
    CHECK(w[0] == M.node0 && w[1] == M.node0 + M.n_nodes && w[2] == M.pool0 && np == M.n_pool);
    CHECK(w[3] == ds.obj_id[size_t(k)] && w[3] >= 0 && w[3] + n_tris <= fl.n_obj);
    const Placed &pl = where[p];
    CHECK((ds.obj[size_t(k)].inst >= 0) == (pl.rot || pl.trans));
    // the expansion: flat objects first(p) + j are the mesh's triangles under this placement's inst
    for (int32_t j = 0; j < n_tris; ++j) {
      const Obj *fo = reinterpret_cast<const Obj *>(fl.obj) + (w[3] + j);
      CHECK(fo->kind == kTriangle && fo->inst == ds.obj[size_t(k)].inst);
    }
    const Node *leaf = nullptr;
    for (const Node &nd : ds.nodes)
      if (nd.leaf >= 0 && (nd.leaf >> 4) <= k && k < (nd.leaf >> 4) + (nd.leaf & 15)) leaf = &nd;
    CHECK(leaf != nullptr && (leaf->leaf & 15) == 1);
    const double th = pl.angle * M_PI / 180.0, c = pl.rot ? std::cos(th) : 1.0, sn = pl.rot ? std::sin(th) : 0.0;
    for (int32_t q = 0; q < M.n_pool; ++q) {
      double v[3][3];
      tri_vertices(ds.pool[size_t(q)], v);
      for (int wv = 0; wv < 3; ++wv) {
        const double x[3] = {c * v[wv][0] + sn * v[wv][2] + (pl.trans ? pl.off[0] : 0.0), v[wv][1] + (pl.trans ? pl.off[1] : 0.0),
                             -sn * v[wv][0] + c * v[wv][2] + (pl.trans ? pl.off[2] : 0.0)};
        for (int a = 0; a < 3; ++a) CHECK(x[a] >= leaf->bmin[a] && x[a] <= leaf->bmax[a]);
      }
    }
  }
  for (const Node &nd : ds.nodes) {
    if (nd.leaf < 0) continue;
    CHECK((nd.leaf >> 4) >= 0 && size_t((nd.leaf >> 4) + (nd.leaf & 15)) <= ds.obj.size());
  }
  int32_t st[6];
  CHECK(rt_nw_scene_instancing_stats(s, st) == RT_OK);
  CHECK(st[0] == 1 && st[1] == int32_t(where.size()) && st[2] == M.n_pool && st[3] == M.n_nodes &&
        st[4] == int32_t(ds.obj.size()) && st[5] == int32_t(ds.nodes.size()));
}

int main() {
  std::vector<double> v;
  std::vector<int32_t> f;
  {  // icosphere(2) five ways (the last placement twice), a collinear triangle in the mesh, four spheres
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.5, 0.5, 0.5));
    CHECK(mat >= 0);
    icosphere(2, v, f);
    CHECK(f.size() == 3 * 320);
    const int mesh = rt_nw_mesh(s, v.data(), int32_t(v.size() / 3), f.data(), 320, nullptr, 0, nullptr, mat);
    const double a[3] = {0, 0, 0}, b[3] = {1, 1, 1}, c[3] = {2, 2, 2};
    const int32_t both[2] = {mesh, rt_nw_triangle(s, a, b, c, mat)};
    CHECK(both[0] >= 0 && both[1] >= 0);
    const int grp = rt_nw_group(s, both, 2);
    const int shared = rt_nw_shared(s, grp);
    CHECK(shared >= 0);
    // what cannot be shared, and where a shared handle cannot go
    const double ctr[3] = {0, 0, 0}, off[3] = {1, 2, 3};
    const int sph = rt_nw_sphere(s, ctr, 1.0, mat);
    CHECK(rt_nw_shared(s, sph) == RT_EUNSUPPORTED);
    CHECK(rt_nw_shared(s, rt_nw_translate(s, mesh, off)) == RT_EUNSUPPORTED);
    CHECK(rt_nw_shared(s, rt_nw_rotate_y(s, mesh, 10)) == RT_EUNSUPPORTED);
    CHECK(rt_nw_shared(s, shared) == RT_EUNSUPPORTED);
    const int32_t mixed[2] = {mesh, sph};
    CHECK(rt_nw_shared(s, rt_nw_group(s, mixed, 2)) == RT_EUNSUPPORTED);
    CHECK(rt_nw_shared(s, rt_nw_group(s, nullptr, 0)) == RT_EINVAL);
    CHECK(rt_nw_shared(s, -1) == RT_EINVAL && rt_nw_shared(s, 1 << 30) == RT_EINVAL && rt_nw_shared(nullptr, 0) == RT_EINVAL);
    CHECK(rt_nw_constant_medium(s, shared, 0.1, 0) == RT_EUNSUPPORTED);
    CHECK(rt_nw_constant_medium(s, rt_nw_translate(s, shared, off), 0.1, 0) == RT_EUNSUPPORTED);
    CHECK(rt_nw_scene_instancing_stats(s, nullptr) == RT_EINVAL);
    for (int k = 0; k < 4; ++k) {
      const double sc[3] = {2.5 - 1.5 * k, 2.6 - k, 0.9 + k};
      CHECK(rt_nw_world_add(s, rt_nw_sphere(s, sc, 0.8, mat)) == RT_OK);
    }
    const std::vector<Placed> where = {{false, false, 0, {0, 0, 0}},        {false, true, 0, {3.1, 0.4, -0.7}},
                                       {true, false, 30, {0, 0, 0}},        {true, true, 75, {-2.9, 0.3, 0.8}},
                                       {true, true, 75, {-2.9, 0.3, 0.8}}};
    check_scene(s, shared, 321, 320, where, 4);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  {  // icosphere(4) three times: a bottom level of thousands of nodes
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.5, 0.5, 0.5));
    icosphere(4, v, f);
    CHECK(f.size() == 3 * 5120);
    const int mesh = rt_nw_mesh(s, v.data(), int32_t(v.size() / 3), f.data(), 5120, nullptr, 0, nullptr, mat);
    const int shared = rt_nw_shared(s, mesh);
    CHECK(mesh >= 0 && shared >= 0);
    const std::vector<Placed> where = {{false, false, 0, {0, 0, 0}}, {true, true, 200, {4, 0.5, 0}}, {true, true, -33, {0, 0.25, 4}}};
    check_scene(s, shared, 5120, 5120, where, 0);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  {  // a shared mesh of collinear triangles only: placed, never hit, no record
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.5, 0.5, 0.5));
    const double a[3] = {0, 0, 0}, b[3] = {1, 1, 1}, c[3] = {2, 2, 2}, ctr[3] = {0, 0, 0};
    const int shared = rt_nw_shared(s, rt_nw_triangle(s, a, b, c, mat));
    CHECK(shared >= 0);
    CHECK(rt_nw_world_add(s, shared) == RT_OK && rt_nw_world_add(s, rt_nw_sphere(s, ctr, 1.0, mat)) == RT_OK);
    DeviceScene ds;
    CHECK(build_device_scene(s, ds) == RT_OK);
    CHECK(ds.obj.size() == 1 && ds.pool.empty() && ds.bnodes.empty() && ds.place_slot.size() == 1 && ds.place_slot[0] == -1);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  std::printf("all checks passed\n");
  return 0;
}
