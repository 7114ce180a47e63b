// nw_motion_sanitize.cpp — stand-alone driver of tests/test_nw_motion.py's
// sanitizer run: rt_nw_move, rt_nw_scene_flat_at and the moving placements of
// build_device_scene (rtmi_nw_scene.cpp) under ASan + UBSan (host code only, no
// device).  The scenes are those of the motion tests (tests/nw_motion_util.py:
// M, S, F, L); for each, at several times and interleaved with the device build:
//  - the flat view at T holds, for every moving placement, motion_offset of the
//    o0 (its Inst) and o1, times (its record) the device scene carries, with the
//    translation flag set; a static placement's row is the device's;
//  - every placement is alone in a leaf whose box contains the mesh's vertices
//    under the placement's transform at 33 times in [0, 1] (the float offset the
//    kernels form, rtmi_nw_types.h motion_offset);
//  - rt_nw_scene_motion_stats counts them; everything is destroyed (leaks are errors).
//   nw_motion_sanitize
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

static void tri_vertices(const Obj &o, double v[3][3]) {
  const float f[9] = {o.g0[0], o.g0[1], o.g0[2], o.g0[3], o.g1[0], o.g1[1], o.g1[2], o.g1[3], o.g2[0]};
  for (int k = 0; k < 9; ++k) v[k / 3][k % 3] = f[k];
}

// the Inst of a placement record at time T, as the kernels form it
static Inst inst_at(const DeviceScene &ds, const Obj &rec, float T) {
  Inst in{1.f, 0.f, {0.f, 0.f, 0.f}, 0, {0, 0}};
  if (rec.inst >= 0) in = ds.inst[size_t(rec.inst)];
  if (rec.aux == 1) {
    const float o0[3] = {in.off[0], in.off[1], in.off[2]}, o1[3] = {rec.g1[1], rec.g1[2], rec.g1[3]};
    motion_offset(o0, o1, rec.g2[1], rec.g2[0], T, in.off);
  }
  return in;
}

// The scene is complete: n_moving + n_static placements of one mesh of n_tris triangles, n_other objects beside.
static void check_scene(rt_nw_scene *s, int32_t n_tris, int32_t n_moving, int32_t n_static, int32_t n_other) {
  const int32_t n_place = n_moving + n_static;
  int32_t ms[2] = {-1, -1};
  CHECK(rt_nw_scene_motion_stats(s, ms) == RT_OK && ms[0] == n_moving && ms[1] == n_static);
  const double times[] = {0.0, 1.0, 0.5, double(1.0f / 3.0f), 0.25, 0.75, double(std::nextafter(1.0f, 0.0f))};
  for (double T : times) {
    rt_nw_flat fl;
    CHECK(rt_nw_scene_flat_at(s, T, &fl) == RT_OK);
    CHECK(fl.n_obj == n_other + n_tris * n_place);
    DeviceScene ds;  // (built between flat views at different times: it must not depend on the view that is there)
    CHECK(build_device_scene(s, ds) == RT_OK);
    CHECK(ds.n_moving == n_moving && ds.mesh.size() == 1 && int32_t(ds.place_slot.size()) == n_place);
    CHECK(ds.obj.size() == size_t(n_other + n_place));
    const Obj *fobj = reinterpret_cast<const Obj *>(fl.obj);
    const Inst *finst = reinterpret_cast<const Inst *>(fl.inst);
    int32_t seen_moving = 0;
    for (int32_t p = 0; p < n_place; ++p) {
      const int32_t k = ds.place_slot[size_t(p)];
      CHECK(k >= 0 && size_t(k) < ds.obj.size() && ds.obj[size_t(k)].kind == kInstance);
      const Obj &rec = ds.obj[size_t(k)];
      CHECK(rec.inst < int32_t(ds.inst.size()) && (rec.aux == 0 || rec.aux == 1));
      int32_t first;
      std::memcpy(&first, &rec.g0[3], 4);
      CHECK(first >= 0 && first + n_tris <= fl.n_obj);
      // the flat view at T: this placement's row is the record's Inst at T
      const Inst want = inst_at(ds, rec, float(T));
      const int32_t fi = fobj[first].inst;
      CHECK((fi >= 0) == (rec.inst >= 0) && fi < fl.n_inst);
      if (fi >= 0) {
        CHECK(std::memcmp(&finst[fi].c, &want.c, 4) == 0 && std::memcmp(&finst[fi].s, &want.s, 4) == 0);
        CHECK(std::memcmp(finst[fi].off, want.off, 12) == 0 && finst[fi].flags == want.flags);
      }
      for (int32_t j = 0; j < n_tris; ++j) CHECK(fobj[first + j].kind == kTriangle && fobj[first + j].inst == fi);
      if (rec.aux == 1) {
        ++seen_moving;
        CHECK(rec.inst >= 0 && (ds.inst[size_t(rec.inst)].flags & 2) && rec.g2[0] != rec.g2[1]);
      } else {
        CHECK(rec.g1[1] == 0.f && rec.g1[2] == 0.f && rec.g1[3] == 0.f && rec.g2[0] == 0.f && rec.g2[1] == 0.f);
      }
      // alone in a leaf whose box holds the mesh at 33 times in [0, 1]
      const Node *leaf = nullptr;
      for (const Node &nd : ds.nodes)
        if (nd.leaf >= 0 && (nd.leaf >> 4) <= k && k < (nd.leaf >> 4) + (nd.leaf & 15)) leaf = &nd;
      CHECK(leaf != nullptr && (leaf->leaf & 15) == 1);
      for (int q = 0; q <= 32; ++q) {
        const Inst in = inst_at(ds, rec, float(q) / 32.0f);
        for (const Obj &tri : ds.pool) {
          double v[3][3];
          tri_vertices(tri, v);
          for (int w = 0; w < 3; ++w) {
            const double x[3] = {double(in.c) * v[w][0] + double(in.s) * v[w][2] + in.off[0], v[w][1] + in.off[1],
                                 -double(in.s) * v[w][0] + double(in.c) * v[w][2] + in.off[2]};
            for (int a = 0; a < 3; ++a) CHECK(x[a] >= leaf->bmin[a] && x[a] <= leaf->bmax[a]);
          }
        }
      }
    }
    CHECK(seen_moving == n_moving);
    int32_t n_attr = 0;
    const float *attr = nullptr;
    const int32_t *of = nullptr;
    CHECK(rt_nw_scene_flat_attr(s, &n_attr, &attr, &of) == RT_OK);  // follows the last flat view
    long sum = 0;
    for (int32_t i = 0; i < fl.n_obj; ++i) sum += of[i];
    CHECK(sum >= -long(fl.n_obj));
  }
}

static int32_t place(rt_nw_scene *s, int32_t h, bool rot, double angle, bool trans, const double *off) {
  if (rot) h = rt_nw_rotate_y(s, h, angle);
  CHECK(h >= 0);
  if (trans) h = rt_nw_translate(s, h, off);
  CHECK(h >= 0);
  return h;
}

int main() {
  std::vector<double> v;
  std::vector<int32_t> f;
  {  // scene M: static, move above a rotation, move under a rotation on the division path; and what cannot move
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.6, 0.5, 0.4));
    icosphere(2, v, f);
    const int mesh = rt_nw_mesh(s, v.data(), int32_t(v.size() / 3), f.data(), 320, nullptr, 0, nullptr, mat);
    const int h = rt_nw_shared(s, mesh);
    CHECK(mat >= 0 && mesh >= 0 && h >= 0);
    const double a_off[3] = {0.4, 0.2, 3.9}, b0[3] = {-2.9, 0.3, 0.8}, b1[3] = {-1.7, 0.9, 0.2}, c0[3] = {3.1, 0.4, -0.7},
                 c1[3] = {3.1, 1.6, -0.7}, ctr[3] = {2.5, 2.6, 0.9}, nan3[3] = {0, NAN, 0}, big[3] = {0, 1e300, 0};
    const int sph = rt_nw_sphere(s, ctr, 0.9, mat);
    CHECK(rt_nw_move(s, sph, b0, b1, 0, 1) == RT_EUNSUPPORTED);
    CHECK(rt_nw_move(s, mesh, b0, b1, 0, 1) == RT_EUNSUPPORTED);
    const int32_t pair[2] = {h, h};
    CHECK(rt_nw_move(s, rt_nw_group(s, pair, 2), b0, b1, 0, 1) == RT_EUNSUPPORTED);
    CHECK(rt_nw_move(s, rt_nw_constant_medium(s, sph, 0.1, 0), b0, b1, 0, 1) == RT_EUNSUPPORTED);
    CHECK(rt_nw_move(s, h, b0, b1, 0.5, 0.5) == RT_EINVAL && rt_nw_move(s, h, b0, b1, NAN, 1) == RT_EINVAL);
    CHECK(rt_nw_move(s, h, nan3, b1, 0, 1) == RT_EINVAL && rt_nw_move(s, h, b0, big, 0, 1) == RT_EINVAL);
    CHECK(rt_nw_move(s, -1, b0, b1, 0, 1) == RT_EINVAL && rt_nw_move(nullptr, h, b0, b1, 0, 1) == RT_EINVAL);
    const int mv = rt_nw_move(s, place(s, h, true, 75, false, nullptr), b0, b1, 0, 1);
    CHECK(mv >= 0);
    CHECK(rt_nw_move(s, mv, b0, b1, 0, 1) == RT_EUNSUPPORTED);
    CHECK(rt_nw_move(s, rt_nw_translate(s, mv, a_off), b0, b1, 0, 1) == RT_EUNSUPPORTED);
    CHECK(rt_nw_shared(s, mv) == RT_EUNSUPPORTED);
    CHECK(rt_nw_constant_medium(s, mv, 0.1, 0) == RT_EUNSUPPORTED);
    CHECK(rt_nw_scene_motion_stats(s, nullptr) == RT_EINVAL);
    CHECK(rt_nw_world_add(s, place(s, h, true, 30, true, a_off)) == RT_OK);
    CHECK(rt_nw_world_add(s, mv) == RT_OK);
    CHECK(rt_nw_world_add(s, rt_nw_rotate_y(s, rt_nw_move(s, h, c0, c1, 0.25, 0.75), 20)) == RT_OK);
    CHECK(rt_nw_world_add(s, sph) == RT_OK);
    check_scene(s, 320, 2, 1, 1);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  {  // scene S: a mesh with normals and uvs under one move, over the ground
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.5, 0.5, 0.5));
    icosphere(2, v, f);
    std::vector<double> nrm(v.size()), uv(v.size() / 3 * 2);
    const double c[3] = {0.3, -0.2, 0.9};
    for (size_t i = 0; i < v.size(); ++i) nrm[i] = (v[i] - c[i % 3]) / 1.7;
    for (size_t i = 0; i < v.size() / 3; ++i) {
      uv[2 * i] = 0.3 * v[3 * i] + 0.1;
      uv[2 * i + 1] = 0.2 * v[3 * i + 1] - 0.4;
    }
    const int mesh = rt_nw_mesh_attr(s, v.data(), int32_t(v.size() / 3), f.data(), 320, nrm.data(), int32_t(nrm.size() / 3), nullptr,
                                     uv.data(), int32_t(uv.size() / 2), nullptr, RT_NW_MESH_SMOOTH | RT_NW_MESH_UV, mat);
    const double s0[3] = {1.5, -0.4, 2.2}, s1[3] = {2.4, 0.1, 1.6}, g[3] = {0, -1002, 0};
    CHECK(mesh >= 0);
    CHECK(rt_nw_world_add(s, rt_nw_move(s, place(s, rt_nw_shared(s, mesh), true, 40, false, nullptr), s0, s1, 0, 1)) == RT_OK);
    CHECK(rt_nw_world_add(s, rt_nw_sphere(s, g, 1000, mat)) == RT_OK);
    check_scene(s, 320, 1, 0, 1);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  {  // scene F: icosphere(3) nine times, the odd copies moving
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.6, 0.5, 0.4));
    icosphere(3, v, f);
    CHECK(f.size() == 3 * 1280);
    const int h = rt_nw_shared(s, rt_nw_mesh(s, v.data(), int32_t(v.size() / 3), f.data(), 1280, nullptr, 0, nullptr, mat));
    CHECK(h >= 0);
    const double zero[3] = {0, 0, 0}, mvv[3] = {0.3, 0.5, -0.4};
    for (int q = 0; q < 9; ++q) {
      const double off[3] = {4.0 * (q / 3), 0.25 * (q % 3), 4.0 * (q % 3)};
      int32_t obj = q == 0 ? h : place(s, h, true, 23.0 * q, true, off);
      if (q % 2) obj = rt_nw_move(s, obj, zero, mvv, 0, 1);
      CHECK(obj >= 0 && rt_nw_world_add(s, obj) == RT_OK);
    }
    check_scene(s, 1280, 4, 5, 0);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  {  // scene L: one moving light, nothing else; then offset0 == offset1
    for (int same = 0; same < 2; ++same) {
      rt_nw_scene *s = nullptr;
      CHECK(rt_nw_scene_create(&s) == RT_OK);
      const int mat = rt_nw_mat_diffuse_light(s, rt_nw_tex_solid(s, 4, 4, 3));
      icosphere(2, v, f);
      const int h = rt_nw_shared(s, rt_nw_mesh(s, v.data(), int32_t(v.size() / 3), f.data(), 320, nullptr, 0, nullptr, mat));
      const double l0[3] = {-1.275, 0, 0}, l1[3] = {1.275, 0, 0};
      CHECK(rt_nw_world_add(s, rt_nw_move(s, h, l0, same ? l0 : l1, 0, 1)) == RT_OK);
      check_scene(s, 320, 1, 0, 0);
      CHECK(rt_nw_scene_destroy(s) == RT_OK);
    }
  }
  {  // without a move node the flat view does not depend on the time, nor do its pointers
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.6, 0.5, 0.4));
    icosphere(1, v, f);
    const int h = rt_nw_shared(s, rt_nw_mesh(s, v.data(), int32_t(v.size() / 3), f.data(), 80, nullptr, 0, nullptr, mat));
    const double off[3] = {1, 2, 3};
    CHECK(rt_nw_world_add(s, place(s, h, true, 12, true, off)) == RT_OK);
    rt_nw_flat a, b;
    CHECK(rt_nw_scene_flat(s, &a) == RT_OK && rt_nw_scene_flat_at(s, 0.7, &b) == RT_OK);
    CHECK(a.obj == b.obj && a.inst == b.inst && a.n_obj == b.n_obj && a.n_inst == 1);
    CHECK(rt_nw_scene_flat_at(s, INFINITY, &b) == RT_EINVAL && rt_nw_scene_flat_at(s, 0.5, nullptr) == RT_EINVAL);
    check_scene(s, 80, 0, 1, 0);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  std::printf("all checks passed\n");
  return 0;
}
