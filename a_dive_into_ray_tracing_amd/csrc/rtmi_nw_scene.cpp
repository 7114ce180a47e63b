// rtmi_nw_scene.cpp — host half of the Next-Week renderer: the scene builder
// (one call per reference constructor, include/rtmi_nw.h), flattening of the
// instance tree into leaf records with composed transforms, the object BVH,
// the reference's scene presets (rt_next_week/cuda/main.cu:163-413) and the
// curand XORWOW restatement they draw from.  No device code.
#include <algorithm>
#include <cmath>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "rtmi_internal.h"
#include "rtmi_nw_internal.h"

using namespace rtmi;
using namespace rtmi::nw;

namespace {

enum SType { kPrim = 0, kGroup = 1, kTranslate = 2, kRotate = 3, kMediumNode = 4, kShared = 5, kMove = 6, kTransform = 7 };

struct SNode {
  int type = kPrim;
  int32_t kind = 0, mat = -1;  // kPrim
  int32_t attr = -1;           // kPrim, a triangle: its attribute record (rt_nw_scene::attr) or -1
  double g[12] = {0};          // kPrim geometry, double (layout of Obj g0..g2); kTransform: the row-major 3x4 map
  std::vector<int32_t> kids;   // kGroup
  int32_t child = -1;          // kTranslate / kRotate / kMediumNode / kShared / kMove / kTransform
  double off[3] = {0, 0, 0};   // kTranslate; kMove: offset0
  double off1[3] = {0, 0, 0};  // kMove: offset1
  double time0 = 0, time1 = 1; // kMove: the times of offset0 and offset1
  double angle = 0;            // kRotate (degrees)
  double density = 0;          // kMediumNode
  int32_t phase_mat = -1;      // kMediumNode: its isotropic material
  int32_t samples = 1;         // kMediumNode: scattering-distance samples (rt_nw_medium_samples)
};

// world = R(theta) * local + t, R about y: (x, z) -> (c x + s z, -s x + c z)
// (rotate_y's local-to-world map, hittable.h:128-131 / 175-179)
struct Xf {
  double theta = 0;  // degrees
  double t[3] = {0, 0, 0};
  bool rot = false, trans = false;
  // under a rt_nw_move node: t is the translation with the node at offset0, t1
  // with it at offset1, each composed as a static translate's would be
  bool moving = false;
  double t1[3] = {0, 0, 0};
  double time0 = 0, time1 = 1;
  // with a rt_nw_transform node in the chain (an affine placement): world =
  // A * local + t, A row-major; theta, rot and trans are not read any more
  bool affine = false;
  double A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
};

struct Bounds {
  double lo[3], hi[3];
};

// curand XORWOW (cuRAND's published device generator): curand_init(seed, 0,
// 0) state set-up and curand(), curand_uniform = x * 2^-32 + 2^-33 as one
// fused multiply-add (nvcc contracts it by default) in (0, 1].
struct Xorwow {
  uint32_t v[5], d;
  explicit Xorwow(uint64_t seed) {
    const uint32_t s0 = uint32_t(seed) ^ 0xaad26b49u;
    const uint32_t s1 = uint32_t(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * s0;
    const uint32_t t1 = 2591861531u * s1;
    d = 6615241u + t1 + t0;
    v[0] = 123456789u + t0;
    v[1] = 362436069u ^ t0;
    v[2] = 521288629u + t1;
    v[3] = 88675123u ^ t1;
    v[4] = 5783321u + t0;
  }
  uint32_t next() {
    const uint32_t t = v[0] ^ (v[0] >> 2);
    v[0] = v[1];
    v[1] = v[2];
    v[2] = v[3];
    v[3] = v[4];
    v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
    d += 362437u;
    return v[4] + d;
  }
  float uniform() {
    const float inv = 2.3283064e-10f;
    return std::fmaf(float(next()), inv, inv * 0.5f);
  }
  // random_float(min, max) rtweekend.h:45-48 (contracted)
  float range(float lo, float hi) { return std::fmaf(uniform(), hi - lo, lo); }
  // random_int(n) rtweekend.h:36-40: (float)n - 0.000001 in double, stored to
  // float (256 - 1e-6 rounds to 256.0f); u = 1.0f would give n: clamped
  int rint(int n) {
    const float val = float(double(float(n)) - 0.000001);
    const int r = int(uniform() * val);
    return r < n ? r : n - 1;
  }
};

}  // namespace

struct rt_nw_scene {
  std::vector<Tex> tex;
  std::vector<float> perlin_vec;
  std::vector<int32_t> perlin_perm;
  std::vector<uint8_t> image_px;
  std::vector<Image> image;
  std::vector<Mat> mat;
  std::vector<SNode> nodes;
  std::vector<TriAttr> attr;  // triangle attribute records (rt_nw_mesh_attr), creation order
  std::vector<int32_t> world;
  float background[3] = {0.f, 0.f, 0.f};
  // flattened view (rt_nw_scene_flat), insertion order
  bool flat_valid = false;
  float flat_time = 0.f;  // the time the moving placements are expanded at (rt_nw_scene_flat_at)
  int32_t n_moves = 0;    // rt_nw_move nodes made: without one the flat view does not depend on the time
  std::vector<Obj> flat_obj;
  std::vector<int32_t> flat_src;  // the SNode a flattened object came from (twin detection)
  std::vector<int32_t> flat_attr; // its attribute record or -1 (rt_nw_scene_flat_attr)
  std::vector<Bounds> flat_bounds;
  std::vector<Inst> flat_inst;
  // affine placements appear baked in the flat view (rt_nw_transform): when one
  // of them carries attribute records, rt_nw_scene_flat_attr shows attr_view
  // (attr, then the baked records) and attr_pub (flat_attr with the baked
  // triangles pointing at theirs); both empty otherwise.  flat_attr itself
  // always names the local record: the device scene is built from it.
  std::vector<TriAttr> flat_attr_view;
  std::vector<int32_t> flat_attr_pub;
  // every occurrence of a shared handle (rt_nw_shared) reached from the world:
  // its kShared node, composed transform, and the flattened objects it
  // expanded to, [first, first + count)
  struct Place {
    int32_t node, first, count;
    Xf x;
  };
  std::vector<Place> flat_place;
};

namespace {

int add_node(rt_nw_scene *s, SNode n) {
  s->nodes.push_back(std::move(n));
  s->flat_valid = false;
  return int(s->nodes.size()) - 1;
}
bool valid_node(const rt_nw_scene *s, int32_t id) { return id >= 0 && id < int32_t(s->nodes.size()); }
bool valid_tex(const rt_nw_scene *s, int32_t id) { return id >= 0 && id < int32_t(s->tex.size()); }
bool valid_mat(const rt_nw_scene *s, int32_t id) { return id >= 0 && id < int32_t(s->mat.size()); }

int add_tex(rt_nw_scene *s, Tex t) {
  s->tex.push_back(t);
  s->flat_valid = false;
  return int(s->tex.size()) - 1;
}
int add_mat(rt_nw_scene *s, Mat m) {
  s->mat.push_back(m);
  s->flat_valid = false;
  return int(s->mat.size()) - 1;
}

// 3x3 helpers of the affine placements (row-major, double)
void mat_vec(const double A[9], const double v[3], double out[3]) {
  for (int i = 0; i < 3; ++i) out[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
void mat_mul(const double A[9], const double B[9], double out[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// rotate_y's local-to-world matrix: (x, z) -> (c x + s z, -s x + c z)
void ry_matrix(double deg, double R[9]) {
  const double th = deg * M_PI / 180.0, c = std::cos(th), sn = std::sin(th);
  const double r[9] = {c, 0, sn, 0, 1, 0, -sn, 0, c};
  for (int i = 0; i < 9; ++i) R[i] = r[i];
}
// The conditioning bound of an affine map (rt_nw_transform, and every
// placement's composite): ||A||_F * ||A^-1||_F <= kAffineCond.  Every matrix
// with singular values in [1/16, 16] passes (at most 16 sqrt 3 * 16 sqrt 3 =
// 768); DESIGN.md §9 "Affine placements" derives the margins from it.
constexpr double kAffineCond = 1024.0;
// inv = A^-1 (the adjugate over the determinant); false: an entry not finite,
// det <= 0 (singular or a mirror) or beyond the bound.  cond, when given,
// receives ||A||_F * ||A^-1||_F.
bool affine_inverse(const double A[9], double inv[9], double *cond = nullptr) {
  double fa = 0;
  for (int i = 0; i < 9; ++i) {
    if (!std::isfinite(float(A[i])) || !std::isfinite(A[i])) return false;
    fa += A[i] * A[i];
  }
  const double adj[9] = {A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                         A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                         A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
  const double det = A[0] * adj[0] + A[1] * adj[3] + A[2] * adj[6];
  if (!(det > 0) || !std::isfinite(det)) return false;
  double fi = 0;
  for (int i = 0; i < 9; ++i) {
    inv[i] = adj[i] / det;
    if (!std::isfinite(float(inv[i]))) return false;
    fi += inv[i] * inv[i];
  }
  const double k = std::sqrt(fa) * std::sqrt(fi);
  if (cond) *cond = k;
  return k <= kAffineCond;
}

Xf compose_translate(const Xf &x, const double off[3]) {
  Xf r = x;
  if (x.affine) {  // b += A off (both ends of a moving placement)
    double d[3];
    mat_vec(x.A, off, d);
    for (int a = 0; a < 3; ++a) {
      r.t[a] = x.t[a] + d[a];
      if (x.moving) r.t1[a] = x.t1[a] + d[a];
    }
    r.trans = true;
    return r;
  }
  const double th = x.theta * M_PI / 180.0, c = std::cos(th), sn = std::sin(th);
  r.t[0] = x.t[0] + (c * off[0] + sn * off[2]);
  r.t[1] = x.t[1] + off[1];
  r.t[2] = x.t[2] + (-sn * off[0] + c * off[2]);
  if (x.moving) {
    r.t1[0] = x.t1[0] + (c * off[0] + sn * off[2]);
    r.t1[1] = x.t1[1] + off[1];
    r.t1[2] = x.t1[2] + (-sn * off[0] + c * off[2]);
  }
  r.trans = true;
  return r;
}
// rt_nw_move under x: two translations, composed side by side from here on
Xf compose_move(const Xf &x, const SNode &n) {
  Xf r = compose_translate(x, n.off);
  const Xf b = compose_translate(x, n.off1);
  for (int a = 0; a < 3; ++a) r.t1[a] = b.t[a];
  r.moving = true;
  r.time0 = n.time0;
  r.time1 = n.time1;
  return r;
}
// o0, o1 of a moving placement: the two composed translations as floats
void motion_ends(const Xf &x, float o0[3], float o1[3]) {
  for (int a = 0; a < 3; ++a) {
    o0[a] = float(x.t[a]);
    o1[a] = float(x.t1[a]);
  }
}
Xf compose_rotate(const Xf &x, double angle) {
  Xf r = x;
  if (x.affine) {  // A = A Ry
    double R[9];
    ry_matrix(angle, R);
    mat_mul(x.A, R, r.A);
    return r;
  }
  r.theta = x.theta + angle;
  r.rot = true;
  return r;
}

// rt_nw_transform (m, row-major 3x4) under x: b += A m_b, then A = A m_A.  The
// first one of a chain takes A from the rotations composed so far.
Xf compose_transform(const Xf &x, const double m[12]) {
  Xf r = x;
  if (!x.affine) {
    ry_matrix(x.rot ? x.theta : 0.0, r.A);
    r.affine = true;
  }
  const double mb[3] = {m[3], m[7], m[11]}, mA[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
  double d[3], P[9];
  mat_vec(r.A, mb, d);
  for (int a = 0; a < 3; ++a) {
    r.t[a] += d[a];
    if (x.moving) r.t1[a] += d[a];
  }
  mat_mul(r.A, mA, P);
  for (int i = 0; i < 9; ++i) r.A[i] = P[i];
  r.trans = true;
  return r;
}

Bounds local_bounds(const SNode &n, int32_t kind) {
  Bounds b;
  const double *g = n.g;
  auto sphere_at = [&](double cx, double cy, double cz, double r, Bounds &acc) {
    r = std::fabs(r);
    const double c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; ++a) {
      acc.lo[a] = std::min(acc.lo[a], c[a] - r);
      acc.hi[a] = std::max(acc.hi[a], c[a] + r);
    }
  };
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = INFINITY;
    b.hi[a] = -INFINITY;
  }
  switch (kind) {
    case kSphere: sphere_at(g[0], g[1], g[2], g[3], b); break;
    case kMovingSphere: {
      // the centre is linear in time: its extremes over the render's times
      // (camera shutters are restricted to [0, 1]) and the sphere's own
      // interval are at the interval ends
      const double t0 = g[7], t1 = g[8];
      for (double tm : {std::min(0.0, t0), std::max(1.0, t1), t0, t1}) {
        const double f = (tm - t0) / (t1 - t0);
        sphere_at(g[0] + f * (g[4] - g[0]), g[1] + f * (g[5] - g[1]), g[2] + f * (g[6] - g[2]), g[3], b);
      }
      break;
    }
    case kRectXY: case kRectXZ: case kRectYZ: {
      const int ax_a = kind == kRectYZ ? 1 : 0;
      const int ax_b = kind == kRectXY ? 1 : 2;
      const int ax_k = kind == kRectXY ? 2 : kind == kRectXZ ? 1 : 0;
      b.lo[ax_a] = std::min(g[0], g[1]); b.hi[ax_a] = std::max(g[0], g[1]);
      b.lo[ax_b] = std::min(g[2], g[3]); b.hi[ax_b] = std::max(g[2], g[3]);
      b.lo[ax_k] = g[4]; b.hi[ax_k] = g[4];
      break;
    }
    case kBox:
      for (int a = 0; a < 3; ++a) {
        b.lo[a] = std::min(g[a], g[4 + a]);
        b.hi[a] = std::max(g[a], g[4 + a]);
      }
      break;
    case kTriangle:  // nine consecutive values: v0, v1, v2
      for (int a = 0; a < 3; ++a) {
        b.lo[a] = std::min(g[a], std::min(g[3 + a], g[6 + a]));
        b.hi[a] = std::max(g[a], std::max(g[3 + a], g[6 + a]));
      }
      break;
  }
  return b;
}

Bounds world_bounds(const Bounds &lb, const Xf &x) {
  if (!x.affine && !x.rot && !x.trans) return lb;
  Bounds b;
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = INFINITY;
    b.hi[a] = -INFINITY;
  }
  if (x.affine) {  // the eight corners through (A, t)
    for (int i = 0; i < 8; ++i) {
      const double p[3] = {(i & 1) ? lb.hi[0] : lb.lo[0], (i & 2) ? lb.hi[1] : lb.lo[1], (i & 4) ? lb.hi[2] : lb.lo[2]};
      double q[3];
      mat_vec(x.A, p, q);
      for (int a = 0; a < 3; ++a) {
        b.lo[a] = std::min(b.lo[a], q[a] + x.t[a]);
        b.hi[a] = std::max(b.hi[a], q[a] + x.t[a]);
      }
    }
    return b;
  }
  const double th = x.theta * M_PI / 180.0, c = std::cos(th), sn = std::sin(th);
  for (int i = 0; i < 8; ++i) {
    const double p[3] = {(i & 1) ? lb.hi[0] : lb.lo[0], (i & 2) ? lb.hi[1] : lb.lo[1], (i & 4) ? lb.hi[2] : lb.lo[2]};
    const double q[3] = {c * p[0] + sn * p[2] + x.t[0], p[1] + x.t[1], -sn * p[0] + c * p[2] + x.t[2]};
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = std::min(b.lo[a], q[a]);
      b.hi[a] = std::max(b.hi[a], q[a]);
    }
  }
  return b;
}

struct Flattener {
  rt_nw_scene *s;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int32_t>, int32_t> inst_ids;
  int err = RT_OK;
  float time = 0.f;  // moving placements are expanded at off(time) (rtmi_nw_types.h motion_offset)

  int32_t inst_of(const Xf &x) {
    if (!x.rot && !x.trans) return -1;
    Inst in{};
    const double th = x.theta * M_PI / 180.0;
    in.c = x.rot ? float(std::cos(th)) : 1.f;
    in.s = x.rot ? float(std::sin(th)) : 0.f;
    for (int a = 0; a < 3; ++a) in.off[a] = x.trans ? float(x.t[a]) : 0.f;
    if (x.moving) {
      float o0[3], o1[3];
      motion_ends(x, o0, o1);
      motion_offset(o0, o1, float(x.time0), float(x.time1), time, in.off);
    }
    in.flags = (x.rot ? 1 : 0) | (x.trans ? 2 : 0);
    uint32_t b[5];
    std::memcpy(&b[0], &in.c, 4);
    std::memcpy(&b[1], &in.s, 4);
    std::memcpy(&b[2], &in.off[0], 12);
    const auto key = std::make_tuple(b[0], b[1], b[2], b[3], b[4], in.flags);
    auto it = inst_ids.find(key);
    if (it != inst_ids.end()) return it->second;
    s->flat_inst.push_back(in);
    const int32_t id = int32_t(s->flat_inst.size()) - 1;
    inst_ids[key] = id;
    return id;
  }

  static void store_geom(Obj &o, const SNode &n) {
    for (int i = 0; i < 4; ++i) {
      o.g0[i] = float(n.g[i]);
      o.g1[i] = float(n.g[4 + i]);
      o.g2[i] = float(n.g[8 + i]);
    }
  }

  // the single primitive under a medium's boundary subtree
  bool boundary_prim(int32_t id, Xf x, int32_t &prim, Xf &xo) {
    const SNode &n = s->nodes[id];
    switch (n.type) {
      case kPrim: prim = id; xo = x; return true;
      case kTranslate: return boundary_prim(n.child, compose_translate(x, n.off), prim, xo);
      case kRotate: return boundary_prim(n.child, compose_rotate(x, n.angle), prim, xo);
      case kGroup:
        if (n.kids.size() == 1) return boundary_prim(n.kids[0], x, prim, xo);
        return false;
      default: return false;
    }
  }

  // A triangle of an affine placement (only triangles stand under a shared
  // handle): the flat view cannot express its row, so the triangle appears
  // baked — vertices float(A v + b(T)) from the double vertices, no Inst, the
  // attribute normals normalize(A^-T n) (rtmi_nw.h rt_nw_transform).
  void emit_baked(int32_t id, const Xf &x) {
    const SNode &n = s->nodes[id];
    double b[3] = {x.t[0], x.t[1], x.t[2]};
    if (x.moving) {
      float o0[3], o1[3], ot[3];
      motion_ends(x, o0, o1);
      motion_offset(o0, o1, float(x.time0), float(x.time1), time, ot);
      for (int a = 0; a < 3; ++a) b[a] = ot[a];
    }
    SNode w = n;
    for (int v = 0; v < 3; ++v) {
      double q[3];
      mat_vec(x.A, &n.g[3 * v], q);
      for (int a = 0; a < 3; ++a) w.g[3 * v + a] = q[a] + b[a];
    }
    Obj o{};
    store_geom(o, w);
    o.kind = n.kind;
    o.mat = n.mat;
    o.inst = -1;
    o.aux = 0;
    s->flat_obj.push_back(o);
    s->flat_src.push_back(id);
    s->flat_attr.push_back(n.attr);
    s->flat_bounds.push_back(local_bounds(w, n.kind));
    if (n.attr < 0) return;
    TriAttr ta = s->attr[size_t(n.attr)];
    double inv[9];
    if ((ta.flags & 1) && affine_inverse(x.A, inv)) {
      for (int v = 0; v < 3; ++v) {  // A^-T n: the inverse read by columns
        double w3[3], l2 = 0;
        for (int j = 0; j < 3; ++j) {
          w3[j] = inv[j] * ta.n[3 * v] + inv[3 + j] * ta.n[3 * v + 1] + inv[6 + j] * ta.n[3 * v + 2];
          l2 += w3[j] * w3[j];
        }
        const double il = l2 > 0 ? 1.0 / std::sqrt(l2) : 0.0;
        for (int j = 0; j < 3; ++j) ta.n[3 * v + j] = float(w3[j] * il);
      }
    }
    baked_attr.push_back(ta);
    baked_of.push_back(int32_t(s->flat_obj.size()) - 1);
  }
  std::vector<TriAttr> baked_attr;  // the baked attribute records and the flattened objects they belong to
  std::vector<int32_t> baked_of;

  void emit(int32_t id, Xf x, int depth) {
    if (err) return;
    if (depth > 64) {
      err = set_error(RT_EINVAL, "rt_nw: object nesting deeper than 64 (a cycle?)");
      return;
    }
    const SNode &n = s->nodes[id];
    switch (n.type) {
      case kPrim: {
        if (x.affine) {
          emit_baked(id, x);
          return;
        }
        Obj o{};
        store_geom(o, n);
        o.kind = n.kind;
        o.mat = n.mat;
        o.inst = inst_of(x);
        o.aux = 0;
        s->flat_obj.push_back(o);
        s->flat_src.push_back(id);
        s->flat_attr.push_back(n.attr);
        s->flat_bounds.push_back(world_bounds(local_bounds(n, n.kind), x));
        return;
      }
      case kGroup:
        for (int32_t k : n.kids) emit(k, x, depth + 1);
        return;
      case kTranslate: emit(n.child, compose_translate(x, n.off), depth + 1); return;
      case kRotate: emit(n.child, compose_rotate(x, n.angle), depth + 1); return;
      case kMove: emit(n.child, compose_move(x, n), depth + 1); return;
      case kTransform: emit(n.child, compose_transform(x, n.g), depth + 1); return;
      case kShared: {  // the flat view is the expansion; the placement is remembered for the device scene
        const int32_t first = int32_t(s->flat_obj.size());
        if (x.affine) {  // the composite map obeys rt_nw_transform's bound, and its offsets are floats
          double inv[9];
          bool ok = affine_inverse(x.A, inv);
          for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(float(x.t[a])) && (!x.moving || std::isfinite(float(x.t1[a])));
          if (!ok) {
            err = set_error(RT_EINVAL,
                            "rt_nw: placement %d (shared handle %d): its composite affine map is not finite, not orientation "
                            "preserving or beyond the conditioning bound %g on |A|_F |A^-1|_F",
                            int(s->flat_place.size()), id, kAffineCond);
            return;
          }
        }
        emit(n.child, x, depth + 1);
        if (!err) s->flat_place.push_back(rt_nw_scene::Place{id, first, int32_t(s->flat_obj.size()) - first, x});
        return;
      }
      case kMediumNode: {
        int32_t prim = -1;
        Xf xb;
        if (!boundary_prim(n.child, x, prim, xb)) {
          err = set_error(RT_EUNSUPPORTED, "constant_medium boundary must be one sphere, moving sphere or box");
          return;
        }
        const SNode &b = s->nodes[prim];
        if (b.kind != kSphere && b.kind != kMovingSphere && b.kind != kBox) {
          err = set_error(RT_EUNSUPPORTED, "constant_medium boundary kind %d unsupported", b.kind);
          return;
        }
        Obj o{};
        store_geom(o, b);
        o.g2[3] = float(-1.0 / n.density);  // neg_inv_density constant_medium.h:13-14
        o.kind = kMedium;
        o.aux = b.kind | (n.samples << 8);
        o.mat = n.phase_mat;
        o.inst = inst_of(xb);
        s->flat_obj.push_back(o);
        s->flat_src.push_back(prim);
        s->flat_attr.push_back(-1);
        s->flat_bounds.push_back(world_bounds(local_bounds(b, b.kind), xb));
        return;
      }
    }
  }
};

// time: the instant moving placements are expanded at; null: whichever view is
// there (time 0 when there is none)
int flatten(rt_nw_scene *s, const float *time = nullptr) {
  if (s->flat_valid && (!time || s->n_moves == 0 || std::memcmp(time, &s->flat_time, sizeof(float)) == 0)) return RT_OK;
  s->flat_valid = false;
  s->flat_time = time ? *time : 0.f;
  s->flat_obj.clear();
  s->flat_src.clear();
  s->flat_attr.clear();
  s->flat_bounds.clear();
  s->flat_inst.clear();
  s->flat_place.clear();
  s->flat_attr_view.clear();
  s->flat_attr_pub.clear();
  Flattener f{s, {}, RT_OK, s->flat_time};
  for (int32_t id : s->world) f.emit(id, Xf{}, 0);
  if (f.err) return f.err;
  if (!f.baked_attr.empty()) {
    if (s->attr.size() + f.baked_attr.size() >= (size_t(1) << 27)) return set_error(RT_EINVAL, "rt_nw: too many attribute records");
    s->flat_attr_view = s->attr;
    s->flat_attr_pub = s->flat_attr;
    for (size_t i = 0; i < f.baked_attr.size(); ++i) {
      s->flat_attr_pub[size_t(f.baked_of[i])] = int32_t(s->flat_attr_view.size());
      s->flat_attr_view.push_back(f.baked_attr[i]);
    }
  }
  // twins: an object that is also a medium's boundary (the same primitive
  // under the same transform, e.g. the final scene's glass sphere and its
  // blue interior, main.cu:386-391) is hidden where that medium hits
  int32_t n_media = 0;
  for (size_t m = 0; m < s->flat_obj.size(); ++m) {
    if (s->flat_obj[m].kind != kMedium) continue;
    ++n_media;
    for (size_t k = 0; k < s->flat_obj.size(); ++k)
      if (s->flat_obj[k].kind != kMedium && s->flat_src[k] == s->flat_src[m] && s->flat_obj[k].inst == s->flat_obj[m].inst &&
          s->flat_obj[k].aux == 0)
        s->flat_obj[k].aux = int32_t(m) + 1;
  }
  if (n_media > kMaxMedia) return set_error(RT_EUNSUPPORTED, "rt_nw: more than %d media", kMaxMedia);
  if (s->flat_obj.size() >= (size_t(1) << 27)) return set_error(RT_EINVAL, "rt_nw: too many objects");
  s->flat_valid = true;
  return RT_OK;
}

// BVH over the flattened objects, built with the surface-area heuristic
// (full sweep over the centroid order on each axis): a child's expected cost
// is its area times the summed test cost of its objects, so a huge object
// (the R=1000 ground sphere) ends up alone near the root instead of inflating
// every box on its path, as a median split leaves it.  Leaves of <=
// kNodeLeafMax objects, DFS order with skip links.  Boxes are the objects'
// double bounds, each grown by its own margin, rounded outward to float
// (the RTIOW BVH's margin argument).
struct ObjBvh {
  const std::vector<Bounds> &b;
  const std::vector<double> &w;  // per-object test cost (relative)
  const std::vector<double> &m;  // per-object box margin
  std::vector<Node> nodes;
  std::vector<int32_t> order;
  const std::vector<char> *solo = nullptr;  // objects that get a leaf of their own (placements); null: none

  static double area(const double lo[3], const double hi[3]) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
  }
  void build(int32_t *ids, int cnt) {
    const int me = int(nodes.size());
    nodes.push_back(Node{});
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double glo[3] = {INFINITY, INFINITY, INFINITY}, ghi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double wsum = 0;
    for (int i = 0; i < cnt; ++i) {
      wsum += w[ids[i]];
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], b[ids[i]].lo[a]);
        hi[a] = std::max(hi[a], b[ids[i]].hi[a]);
        glo[a] = std::min(glo[a], b[ids[i]].lo[a] - m[ids[i]]);
        ghi[a] = std::max(ghi[a], b[ids[i]].hi[a] + m[ids[i]]);
      }
    }
    Node nd{};
    for (int a = 0; a < 3; ++a) {  // every object grown by its own margin
      nd.bmin[a] = std::nextafter(float(glo[a]), -INFINITY);
      nd.bmax[a] = std::nextafter(float(ghi[a]), INFINITY);
    }
    // best SAH split: cost = C_trav * A + A_L * W_L + A_R * W_R (A = area)
    const double pa = std::max(area(lo, hi), 1e-30);
    double best = INFINITY;
    int best_ax = -1, best_i = -1;
    std::vector<double> right_cost(cnt);
    for (int ax = 0; ax < 3 && cnt > 1; ++ax) {
      std::sort(ids, ids + cnt, [&](int32_t x, int32_t y) {
        const double cx = b[x].lo[ax] + b[x].hi[ax], cy = b[y].lo[ax] + b[y].hi[ax];
        return cx < cy || (cx == cy && x < y);
      });
      double rl[3] = {INFINITY, INFINITY, INFINITY}, rh[3] = {-INFINITY, -INFINITY, -INFINITY}, rw = 0;
      for (int i = cnt - 1; i > 0; --i) {  // right part = ids[i..cnt)
        rw += w[ids[i]];
        for (int a = 0; a < 3; ++a) {
          rl[a] = std::min(rl[a], b[ids[i]].lo[a]);
          rh[a] = std::max(rh[a], b[ids[i]].hi[a]);
        }
        right_cost[i] = area(rl, rh) * rw;
      }
      double ll[3] = {INFINITY, INFINITY, INFINITY}, lh[3] = {-INFINITY, -INFINITY, -INFINITY}, lw = 0;
      for (int i = 1; i < cnt; ++i) {  // left part = ids[0..i)
        lw += w[ids[i - 1]];
        for (int a = 0; a < 3; ++a) {
          ll[a] = std::min(ll[a], b[ids[i - 1]].lo[a]);
          lh[a] = std::max(lh[a], b[ids[i - 1]].hi[a]);
        }
        const double c = area(ll, lh) * lw + right_cost[i];
        if (c < best) {
          best = c;
          best_ax = ax;
          best_i = i;
        }
      }
    }
#ifndef RTMI_NW_KTRAV
#define RTMI_NW_KTRAV 2.0
#endif
    const double kTrav = RTMI_NW_KTRAV;  // a node visit against one sphere test
    bool may_share = true;
    if (solo)
      for (int i = 0; i < cnt; ++i) may_share = may_share && !(*solo)[ids[i]];
    const bool leaf = cnt == 1 || (may_share && cnt <= kNodeLeafMax && pa * wsum <= kTrav * pa + best);
    if (leaf) {
      nd.leaf = (int32_t(order.size()) << 4) | cnt;
      for (int i = 0; i < cnt; ++i) order.push_back(ids[i]);
      nd.skip = me + 1;
    } else {
      std::sort(ids, ids + cnt, [&](int32_t x, int32_t y) {
        const double cx = b[x].lo[best_ax] + b[x].hi[best_ax], cy = b[y].lo[best_ax] + b[y].hi[best_ax];
        return cx < cy || (cx == cy && x < y);
      });
      build(ids, best_i);
      build(ids + best_i, cnt - best_i);
      nd.leaf = -1;
      nd.skip = int(nodes.size());
    }
    nodes[me] = nd;
  }
};

// Uniform grid over the non-media objects, the RTIOW grid's
// build (rtmi_accel_build.cpp build_grid) for general objects: an object whose box
// is more than 8x the median's largest extent (the R = 1000 ground, a
// room-sized light) is tested brute force beside the grid; the others are
// listed in every cell their margin-grown box overlaps.  Cell boundaries are
// the float values g0 + c*h the device computes (origin rounded down, size
// rounded up, so the float cells cover the box).  `order` maps leaf-order
// slots to flattened objects; refs hold leaf-order slots.
void build_obj_grid(const std::vector<Bounds> &bounds, const std::vector<double> &margin,
                    const std::vector<int32_t> &order, DeviceScene &out) {
  out.grid_ok = false;
  const int n = int(order.size());
  if (n == 0 || n > 65535) return;
  std::vector<double> ext(n);
  for (int k = 0; k < n; ++k) {
    const Bounds &b = bounds[order[k]];
    double e = 0;
    for (int a = 0; a < 3; ++a) e = std::max(e, b.hi[a] - b.lo[a]);
    ext[k] = e + 2 * margin[order[k]];
  }
  std::vector<double> sorted = ext;
  std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
  const double big_ext = 8.0 * std::max(sorted[n / 2], 1e-9);
  std::vector<int32_t> small;
  out.grid_big.clear();
  for (int k = 0; k < n; ++k) (ext[k] > big_ext ? out.grid_big : small).push_back(k);
  if (small.empty()) return;
  auto grown = [&](int k, int a, bool hi) {
    const Bounds &b = bounds[order[k]];
    return hi ? b.hi[a] + margin[order[k]] : b.lo[a] - margin[order[k]];
  };
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int32_t k : small)
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], grown(k, a, false));
      hi[a] = std::max(hi[a], grown(k, a, true));
    }
  const char *env = std::getenv("RTMI_NW_GRID_CELLS");
  // cells per object: motion-blur scene 0.25 -> 134.1 ms, 0.5 -> 118.1, 1 -> 104.6, 2 -> 113.1,
  // 4 -> 118.7 (BVH 114.0; profiles/r02/nw_grid/)
  const double per_obj = env && std::atof(env) > 0 ? std::atof(env) : 1.0;
  double e[3], vol = 1;
  for (int a = 0; a < 3; ++a) {
    e[a] = std::max(hi[a] - lo[a], 1e-6 * (1 + std::fabs(lo[a])));
    vol *= e[a];
  }
  const double cell = std::cbrt(vol / (per_obj * double(small.size())));
  int64_t total = 1;
  for (int a = 0; a < 3; ++a) {
    out.grid_n[a] = int32_t(std::min<double>(128, std::max<double>(1, std::ceil(e[a] / cell))));
    total *= out.grid_n[a];
  }
  if (total > 16384) return;
  for (int a = 0; a < 3; ++a) {
    float g0 = float(lo[a]);
    if (double(g0) > lo[a]) g0 = std::nextafter(g0, -INFINITY);
    float h = float(e[a] / out.grid_n[a]);
    while (double(g0) + double(h) * out.grid_n[a] < hi[a]) h = std::nextafter(h, INFINITY);
    out.grid_g0[a] = g0;
    out.grid_h[a] = h;
    out.grid_inv_h[a] = 1.0f / h;
    out.grid_g1[a] = std::fmaf(float(out.grid_n[a]), h, g0);
  }
  std::vector<std::vector<uint16_t>> lists(static_cast<size_t>(total));
  for (int32_t k : small) {
    int c0[3], c1[3];
    for (int a = 0; a < 3; ++a) {  // every cell [g0 + c*h, g0 + (c+1)*h] the grown box touches
      const double g0 = out.grid_g0[a], h = out.grid_h[a];
      c0[a] = std::max(0, std::min(out.grid_n[a] - 1, int(std::floor((grown(k, a, false) - g0) / h))));
      c1[a] = std::max(0, std::min(out.grid_n[a] - 1, int(std::floor((grown(k, a, true) - g0) / h))));
    }
    for (int z = c0[2]; z <= c1[2]; ++z)
      for (int y = c0[1]; y <= c1[1]; ++y)
        for (int x = c0[0]; x <= c1[0]; ++x)
          lists[size_t(x + out.grid_n[0] * (y + out.grid_n[1] * z))].push_back(uint16_t(k));
  }
  out.grid_cell_start.assign(size_t(total) + 1, 0);
  out.grid_refs.clear();
  out.grid_max_cell = 0;
  for (int64_t c = 0; c < total; ++c) {
    out.grid_cell_start[size_t(c)] = uint16_t(out.grid_refs.size());
    out.grid_refs.insert(out.grid_refs.end(), lists[size_t(c)].begin(), lists[size_t(c)].end());
    out.grid_max_cell = std::max(out.grid_max_cell, int32_t(lists[size_t(c)].size()));
    if (out.grid_refs.size() > 65535) return;
  }
  out.grid_cell_start[size_t(total)] = uint16_t(out.grid_refs.size());
  out.grid_ok = true;
}

// A triangle whose float vertices are collinear: cross(v1 - v0, v2 - v0),
// evaluated in double from the stored floats, is the zero vector.  It has no
// normal, and the renderer never hits it.
bool collinear_triangle(const Obj &o) {
  if (o.kind != kTriangle) return false;
  const double v0[3] = {o.g0[0], o.g0[1], o.g0[2]}, v1[3] = {o.g0[3], o.g1[0], o.g1[1]}, v2[3] = {o.g1[2], o.g1[3], o.g2[0]};
  const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  return e1[1] * e2[2] - e1[2] * e2[1] == 0.0 && e1[2] * e2[0] - e1[0] * e2[2] == 0.0 && e1[0] * e2[1] - e1[1] * e2[0] == 0.0;
}

}  // namespace

namespace rtmi {
namespace nw {

int build_device_scene(rt_nw_scene *s, DeviceScene &out) {
  if (!s) return set_error(RT_EINVAL, "null scene");
  if (int rc = flatten(s)) return rc;
  const int n_all = int(s->flat_obj.size());
  if (n_all == 0) return set_error(RT_EINVAL, "rt_nw: empty world (rt_nw_world_add)");
  out.mesh.clear();
  out.place_mesh.clear();
  out.place_slot.clear();
  out.pool.clear();
  out.pool_j.clear();
  out.pool_attr.clear();
  out.bnodes.clear();
  // Shared meshes (DESIGN.md §9 "Shared meshes"): the flattened objects of a
  // placement stay out of the top level; the placement itself joins it as
  // object n_all + p, bounded by its mesh's local box under its transform.
  // A mesh's triangles are those of its first placement's expansion (the
  // geometry of every expansion is the same; only `inst` differs).
  const std::vector<rt_nw_scene::Place> &places = s->flat_place;
  const int n_place = int(places.size());
  struct MeshBuild {
    int32_t first;                // its first placement's first flattened object
    std::vector<Bounds> lb;       // per triangle j, local space
    std::vector<int32_t> tris;    // the j that are not collinear
    Bounds box;                   // their union
    double reach = 0;             // the farthest a local ray of one of its affine placements starts (0: none)
  };
  // triangle k of the flat view in its mesh's local space: the flattened record
  // itself, except under an affine placement, whose flat view is baked
  auto local_obj = [&](int32_t k) {
    Obj o = s->flat_obj[size_t(k)];
    if (o.kind == kTriangle) Flattener::store_geom(o, s->nodes[size_t(s->flat_src[size_t(k)])]);
    return o;
  };
  std::vector<MeshBuild> mb;
  std::vector<char> placed;
  std::vector<Bounds> with_places;  // flat_bounds, then one box per placement
  if (n_place > 0) {
    placed.assign(size_t(n_all), 0);
    std::map<int32_t, int32_t> mesh_of_node;
    for (const rt_nw_scene::Place &p : places) {
      for (int32_t k = p.first; k < p.first + p.count; ++k) placed[size_t(k)] = 1;
      auto it = mesh_of_node.find(p.node);
      if (it == mesh_of_node.end()) {
        it = mesh_of_node.emplace(p.node, int32_t(mb.size())).first;
        MeshBuild m;
        m.first = p.first;
        for (int a = 0; a < 3; ++a) {
          m.box.lo[a] = INFINITY;
          m.box.hi[a] = -INFINITY;
        }
        m.lb.resize(size_t(p.count));
        for (int32_t j = 0; j < p.count; ++j) {
          const Obj o = local_obj(p.first + j);
          if (o.kind != kTriangle) return set_error(RT_EINVAL, "rt_nw: shared geometry holds a non-triangle");
          m.lb[size_t(j)] = local_bounds(s->nodes[size_t(s->flat_src[size_t(p.first + j)])], kTriangle);
          if (collinear_triangle(o)) continue;  // never hit: keeps its index j, joins no BVH
          m.tris.push_back(j);
          for (int a = 0; a < 3; ++a) {
            m.box.lo[a] = std::min(m.box.lo[a], m.lb[size_t(j)].lo[a]);
            m.box.hi[a] = std::max(m.box.hi[a], m.lb[size_t(j)].hi[a]);
          }
        }
        mb.push_back(std::move(m));
        out.mesh.push_back(DeviceScene::SharedMesh{0, 0, 0, 0, p.count});
      }
      out.place_mesh.push_back(it->second);
      if (out.mesh[size_t(it->second)].n_tris != p.count) return set_error(RT_EINVAL, "rt_nw: placements of one mesh differ");
    }
    with_places = s->flat_bounds;
    for (int pi = 0; pi < n_place; ++pi) {
      const Bounds &lb = mb[size_t(out.place_mesh[size_t(pi)])].box;
      const Xf &x = places[size_t(pi)].x;
      if (!x.moving) {
        with_places.push_back(world_bounds(lb, x));
        continue;
      }
      // a moving placement: the union of its boxes at render times 0 and 1 (the
      // offset is linear in time and camera shutters lie in [0, 1]: the moving
      // sphere's argument in local_bounds; DESIGN.md §9 "Moving placements")
      Bounds u;
      for (int a = 0; a < 3; ++a) {
        u.lo[a] = INFINITY;
        u.hi[a] = -INFINITY;
      }
      for (double tm : {0.0, 1.0}) {
        const double f = (tm - x.time0) / (x.time1 - x.time0);
        Xf at = x;
        for (int a = 0; a < 3; ++a) at.t[a] = x.t[a] + f * (x.t1[a] - x.t[a]);
        const Bounds b = world_bounds(lb, at);
        for (int a = 0; a < 3; ++a) {
          u.lo[a] = std::min(u.lo[a], b.lo[a]);
          u.hi[a] = std::max(u.hi[a], b.hi[a]);
        }
      }
      with_places.push_back(u);
    }
  }
  const std::vector<Bounds> &bounds = n_place > 0 ? with_places : s->flat_bounds;
  const int n_ext = n_all + n_place;
  // media are evaluated per segment before the BVH walk;
  // the BVH holds the other objects
  std::vector<int32_t> med_index(n_all, -1), ids;
  out.med.clear();
  out.med_id.clear();
  for (int k = 0; k < n_all; ++k) {
    if (s->flat_obj[k].kind == kMedium) {
      med_index[k] = int32_t(out.med.size());
      out.med.push_back(s->flat_obj[k]);
      out.med_id.push_back(k);
    } else if (n_place > 0 && placed[size_t(k)]) {
      // reached through its placement's record
    } else if (collinear_triangle(s->flat_obj[k])) {
      // never hit (rt_nw_triangle): it keeps its insertion index and joins
      // neither the BVH nor the grid
    } else {
      ids.push_back(k);
    }
  }
  for (int pi = 0; pi < n_place; ++pi)  // (a mesh of collinear triangles only is never hit: no record)
    if (!mb[size_t(out.place_mesh[size_t(pi)])].tris.empty()) ids.push_back(n_all + pi);
  double scale = 0;
  for (int32_t k : ids) {
    const Bounds &b = bounds[k];
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(b.lo[a]) || !std::isfinite(b.hi[a]))
        return set_error(RT_EINVAL, "rt_nw: object with non-finite bounds");
      scale = std::max(scale, std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
    }
  }
  // relative test costs: a box is six rectangle tests, a triangle ~47 flop
  // against a sphere's ~30 with its square root, an instance adds a ray
  // transform; a placement is a walk of its own (a guess: a few node visits
  // and triangle tests)
  std::vector<double> cost(n_ext, 1.0);
  for (int k = 0; k < n_all; ++k) {
    const Obj &o = s->flat_obj[k];
    cost[k] = (o.kind == kBox ? 3.0 : o.kind == kMovingSphere ? 1.2 : o.kind == kTriangle ? 1.5 : 1.0) + (o.inst >= 0 ? 0.3 : 0.0);
  }
  for (int k = n_all; k < n_ext; ++k) cost[k] = 8.0;
  // box margins (the RTIOW BVH's argument): 1e-3 of the
  // object's own coordinate scale — ~100x the float error of its hit test —
  // plus 1e-6 of the scene's, for rays from far away.  One scene-wide margin
  // of 1e-3 of the scene scale grew every small box by ~2 units next to the
  // R = 1000 ground (137 node visits per camera ray instead of ~20).
  std::vector<double> margin(n_ext, 0.0);
  for (int32_t k : ids) {
    double own = 0;
    for (int a = 0; a < 3; ++a)
      own = std::max(own, std::max(std::fabs(bounds[k].lo[a]), std::fabs(bounds[k].hi[a])));
    margin[k] = 1e-3 * (1.0 + own) + 1e-6 * scale;
  }
  // Affine placements (DESIGN.md §9 "Affine placements"): the kernels meet the
  // mesh under float(A^-1), and a local ray formed in float, so the surface
  // they see is displaced from A v + b by up to ~2^-22 k (|q| + t |d|) with k =
  // |A|_F |A^-1|_F <= kAffineCond and q the ray origin seen from b.  The own
  // scale takes the box's extent about b, and 4e-6 k of the scene's scale and
  // |b| joins the margin.  The local ray starts up to |A^-1|_F (sqrt 3 scale +
  // |b|) from the mesh's origin: the mesh's bottom-level margins take that reach
  // where the scene's scale stands for the other placements.
  for (int pi = 0; pi < n_place; ++pi) {
    const Xf &x = places[size_t(pi)].x;
    MeshBuild &m = mb[size_t(out.place_mesh[size_t(pi)])];
    if (!x.affine || m.tris.empty()) continue;
    double inv[9], cond = 0, fi = 0, bmax = 0, ext = 0;
    if (!affine_inverse(x.A, inv, &cond)) return set_error(RT_EINVAL, "rt_nw: placement %d: bad affine map", pi);
    for (int i = 0; i < 9; ++i) fi += inv[i] * inv[i];
    for (int a = 0; a < 3; ++a) {
      bmax = std::max(bmax, std::fabs(x.t[a]));
      if (!x.moving) continue;
      for (double tm : {0.0, 1.0})
        bmax = std::max(bmax, std::fabs(x.t[a] + (tm - x.time0) / (x.time1 - x.time0) * (x.t1[a] - x.t[a])));
    }
    for (int i = 0; i < 8; ++i) {
      const double p[3] = {(i & 1) ? m.box.hi[0] : m.box.lo[0], (i & 2) ? m.box.hi[1] : m.box.lo[1], (i & 4) ? m.box.hi[2] : m.box.lo[2]};
      double q[3];
      mat_vec(x.A, p, q);
      for (int a = 0; a < 3; ++a) ext = std::max(ext, std::fabs(q[a]));
    }
    const int k = n_all + pi;
    double own = ext;
    for (int a = 0; a < 3; ++a) own = std::max(own, std::max(std::fabs(bounds[size_t(k)].lo[a]), std::fabs(bounds[size_t(k)].hi[a])));
    margin[size_t(k)] = 1e-3 * (1.0 + own) + 1e-6 * scale + 4e-6 * cond * (std::sqrt(3.0) * scale + bmax);
    m.reach = std::max(m.reach, std::sqrt(fi) * (std::sqrt(3.0) * scale + bmax));
  }
  std::vector<char> solo;
  if (n_place > 0) {
    solo.assign(size_t(n_ext), 0);
    for (int k = n_all; k < n_ext; ++k) solo[size_t(k)] = 1;
  }
  ObjBvh bvh{bounds, cost, margin, {}, {}};
  if (n_place > 0) bvh.solo = &solo;  // the walk enters a placement from a leaf of its own
  const int n = int(ids.size());
  if (n > 0) bvh.build(ids.data(), n);
  out.nodes = std::move(bvh.nodes);
  // bottom level: one BVH per placed mesh over its triangles in local space,
  // margins as above with the mesh's own scale beside the scene's (a local ray
  // starts as far away as the world ray does)
  for (size_t mi = 0; mi < mb.size(); ++mi) {
    const MeshBuild &m = mb[mi];
    DeviceScene::SharedMesh &M = out.mesh[mi];
    M.node0 = int32_t(out.bnodes.size());
    M.pool0 = int32_t(out.pool.size());
    if (m.tris.empty()) continue;
    double lscale = scale;
    for (int a = 0; a < 3; ++a) lscale = std::max(lscale, std::max(std::fabs(m.box.lo[a]), std::fabs(m.box.hi[a])));
    lscale = std::max(lscale, m.reach);  // (0 without an affine placement: today's margins)
    std::vector<double> lcost(m.lb.size(), 1.5), lmargin(m.lb.size(), 0.0);
    for (int32_t j : m.tris) {
      double own = 0;
      for (int a = 0; a < 3; ++a)
        own = std::max(own, std::max(std::fabs(m.lb[size_t(j)].lo[a]), std::fabs(m.lb[size_t(j)].hi[a])));
      lmargin[size_t(j)] = 1e-3 * (1.0 + own) + 1e-6 * lscale;
    }
    ObjBvh lb{m.lb, lcost, lmargin, {}, {}};
    std::vector<int32_t> lids = m.tris;
    lb.build(lids.data(), int(lids.size()));
    if (out.pool.size() + lb.order.size() >= (size_t(1) << 27) || out.bnodes.size() + lb.nodes.size() >= (size_t(1) << 30))
      return set_error(RT_EINVAL, "rt_nw: shared meshes too large");
    M.n_nodes = int32_t(lb.nodes.size());
    M.n_pool = int32_t(lb.order.size());
    for (Node nd : lb.nodes) {  // absolute links: into bnodes and into the pool
      nd.skip += M.node0;
      if (nd.leaf >= 0) nd.leaf = ((M.pool0 + (nd.leaf >> 4)) << 4) | (nd.leaf & 15);
      out.bnodes.push_back(nd);
    }
    for (int32_t j : lb.order) {
      Obj o = local_obj(m.first + j);
      o.inst = -1;
      o.aux = 0;
      out.pool.push_back(o);
      out.pool_j.push_back(j);
    }
  }
  out.obj.resize(n);
  out.obj_id.resize(n);
  out.attr.clear();
  out.obj_attr.clear();
  bool any_attr = false;
  for (int k = 0; k < n && !any_attr; ++k) any_attr = bvh.order[k] < n_all && s->flat_attr[bvh.order[k]] >= 0;
  for (size_t mi = 0; mi < mb.size() && !any_attr; ++mi)
    for (size_t q = 0; q < size_t(out.mesh[mi].n_pool) && !any_attr; ++q)
      any_attr = s->flat_attr[size_t(mb[mi].first + out.pool_j[size_t(out.mesh[mi].pool0) + q])] >= 0;
  if (any_attr) {  // some object carries an attribute record: the locators exist
    out.attr = s->attr;
    out.obj_attr.resize(n);
    for (size_t mi = 0; mi < mb.size(); ++mi)
      for (size_t q = 0; q < size_t(out.mesh[mi].n_pool); ++q)
        out.pool_attr.push_back(s->flat_attr[size_t(mb[mi].first + out.pool_j[size_t(out.mesh[mi].pool0) + q])]);
  }
  out.place_slot.assign(size_t(n_place), -1);
  out.inst = s->flat_inst;
  out.n_moving = 0;
  out.n_affine = 0;
  for (int k = 0; k < n; ++k) {
    if (bvh.order[k] >= n_all) {  // a placement's record (rtmi_nw_types.h kInstance)
      const int pi = bvh.order[k] - n_all;
      const rt_nw_scene::Place &p = places[size_t(pi)];
      const DeviceScene::SharedMesh &M = out.mesh[size_t(out.place_mesh[size_t(pi)])];
      Obj o{};
      const int32_t w[4] = {M.node0, M.node0 + M.n_nodes, M.pool0, p.first};
      std::memcpy(o.g0, w, sizeof w);
      std::memcpy(&o.g1[0], &M.n_pool, 4);
      o.kind = kInstance;
      o.mat = 0;
      o.inst = s->flat_obj[size_t(p.first)].inst;  // every object of the expansion carries the same one
      o.aux = 0;
      if (p.x.affine) {
        // an affine placement (rtmi_nw_types.h AffInst): two Inst rows of its
        // own behind the flat view's hold float(A^-1) and o0; aux bit 1 marks
        // it, and a moving one keeps the motion words where they are
        AffInst ai{};
        double inv[9];
        (void)affine_inverse(p.x.A, inv);  // (checked when the world was flattened)
        float o1[3];
        for (int i = 0; i < 9; ++i) ai.m[i] = float(inv[i]);
        motion_ends(p.x, ai.off, o1);
        ai.flags = 4;
        Inst rows[2];
        std::memcpy(rows, &ai, sizeof ai);
        out.inst.push_back(rows[0]);
        out.inst.push_back(rows[1]);
        o.inst = int32_t(out.inst.size()) - 2;
        o.aux = 2;
        ++out.n_affine;
        if (p.x.moving) {
          for (int a = 0; a < 3; ++a) o.g1[1 + a] = o1[a];
          o.g2[0] = float(p.x.time1);
          o.g2[1] = float(p.x.time0);
          o.aux = 3;
          ++out.n_moving;
        }
      } else if (p.x.moving) {
        // the flat view's Inst is the placement at one instant; the device takes
        // an Inst of its own with o0 and the motion in the record's free words
        // (rtmi_nw_types.h kInstance), and forms off(time) per ray
        Inst in = s->flat_inst[size_t(o.inst)];
        float o1[3];
        motion_ends(p.x, in.off, o1);
        out.inst.push_back(in);
        o.inst = int32_t(out.inst.size()) - 1;
        for (int a = 0; a < 3; ++a) o.g1[1 + a] = o1[a];
        o.g2[0] = float(p.x.time1);
        o.g2[1] = float(p.x.time0);
        o.aux = 1;
        ++out.n_moving;
      }
      out.obj[k] = o;
      out.obj_id[k] = p.first;
      if (any_attr) out.obj_attr[k] = -1;
      out.place_slot[size_t(pi)] = k;
      continue;
    }
    out.obj[k] = s->flat_obj[bvh.order[k]];
    out.obj_id[k] = bvh.order[k];
    if (any_attr) out.obj_attr[k] = s->flat_attr[bvh.order[k]];
    if (out.obj[k].aux > 0) out.obj[k].aux = med_index[out.obj[k].aux - 1] + 1;  // twin -> media-list index + 1
  }
  if (n_place > 0) {  // no uniform grid over placements (out of scope): such a scene renders with the BVH
    out.grid_ok = false;
    out.grid_max_cell = 0;
    out.grid_cell_start.clear();
    out.grid_refs.clear();
    out.grid_big.clear();
  } else {
    build_obj_grid(s->flat_bounds, margin, bvh.order, out);
  }
  out.mat = s->mat;
  out.tex = s->tex;
  out.perlin_vec = s->perlin_vec;
  out.perlin_perm = s->perlin_perm;
  out.image_px = s->image_px;
  out.image = s->image;
  for (int c = 0; c < 3; ++c) out.background[c] = s->background[c];
  out.has_media = !out.med.empty();
  return RT_OK;
}

int scene_instancing_stats(rt_nw_scene *s, int32_t out6[6]) {
  if (!out6) return set_error(RT_EINVAL, "rt_nw_scene_instancing_stats: null");
  DeviceScene ds;
  if (int rc = build_device_scene(s, ds)) return rc;
  out6[0] = int32_t(ds.mesh.size());
  out6[1] = int32_t(ds.place_mesh.size());
  out6[2] = int32_t(ds.pool.size());
  out6[3] = int32_t(ds.bnodes.size());
  out6[4] = int32_t(ds.obj.size());
  out6[5] = int32_t(ds.nodes.size());
  return RT_OK;
}

int scene_grid_stats(rt_nw_scene *s, int32_t *dims3, int32_t *max_cell, int32_t *n_big, int32_t *n_refs) {
  DeviceScene ds;
  if (int rc = build_device_scene(s, ds)) return rc;
  for (int a = 0; a < 3 && dims3; ++a) dims3[a] = ds.grid_ok ? ds.grid_n[a] : 0;
  if (max_cell) *max_cell = ds.grid_ok ? ds.grid_max_cell : 0;
  if (n_big) *n_big = ds.grid_ok ? int32_t(ds.grid_big.size()) : 0;
  if (n_refs) *n_refs = ds.grid_ok ? int32_t(ds.grid_refs.size()) : 0;
  return RT_OK;
}

}  // namespace nw
}  // namespace rtmi

// ---------------------------------------------------------------------------
// C ABI: builder
// ---------------------------------------------------------------------------
RTMI_EXPORT int rt_nw_camera_init(rt_nw_camera *cam, const double lookfrom[3], const double lookat[3],
                                  const double vup[3], double vfov_deg, double aspect_ratio, double aperture,
                                  double focus_dist, double time0, double time1) {
  if (!cam) return set_error(RT_EINVAL, "rt_nw_camera_init: null");
  if (!(time0 >= 0.0 && time1 <= 1.0 && time0 <= time1))
    return set_error(RT_EINVAL, "rt_nw_camera_init: shutter [%g, %g] must lie in [0, 1]", time0, time1);
  if (int rc = rt_camera_init(&cam->cam, lookfrom, lookat, vup, vfov_deg, aspect_ratio, aperture, focus_dist)) return rc;
  cam->time0 = time0;
  cam->time1 = time1;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_scene_create(rt_nw_scene **out) {
  if (!out) return set_error(RT_EINVAL, "null out");
  *out = new (std::nothrow) rt_nw_scene();
  return *out ? RT_OK : set_error(RT_ENOMEM, "rt_nw_scene_create");
}

RTMI_EXPORT int rt_nw_scene_destroy(rt_nw_scene *s) {
  delete s;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_tex_solid(rt_nw_scene *s, double r, double g, double b) {
  if (!s) return set_error(RT_EINVAL, "null scene");
  Tex t{};
  t.kind = kSolid;
  t.rgb[0] = float(r); t.rgb[1] = float(g); t.rgb[2] = float(b);
  return add_tex(s, t);
}

RTMI_EXPORT int rt_nw_tex_checker(rt_nw_scene *s, int32_t even, int32_t odd) {
  if (!s || !valid_tex(s, even) || !valid_tex(s, odd)) return set_error(RT_EINVAL, "rt_nw_tex_checker: bad texture");
  if (s->tex[even].kind == kChecker || s->tex[odd].kind == kChecker)
    return set_error(RT_EUNSUPPORTED, "rt_nw_tex_checker: nested checker textures");
  Tex t{};
  t.kind = kChecker;
  t.a = even;
  t.b = odd;
  return add_tex(s, t);
}

RTMI_EXPORT int rt_nw_tex_noise(rt_nw_scene *s, double scale, const float *ranvec, const int32_t *perm) {
  if (!s || !ranvec || !perm) return set_error(RT_EINVAL, "rt_nw_tex_noise: null");
  for (int i = 0; i < 3 * kPerlinN; ++i)
    if (perm[i] < 0 || perm[i] >= kPerlinN) return set_error(RT_EINVAL, "rt_nw_tex_noise: perm out of range");
  const int id = int(s->perlin_perm.size()) / (3 * kPerlinN);
  for (int i = 0; i < kPerlinN; ++i) {
    s->perlin_vec.push_back(ranvec[3 * i]);
    s->perlin_vec.push_back(ranvec[3 * i + 1]);
    s->perlin_vec.push_back(ranvec[3 * i + 2]);
    s->perlin_vec.push_back(0.f);
  }
  s->perlin_perm.insert(s->perlin_perm.end(), perm, perm + 3 * kPerlinN);
  Tex t{};
  t.kind = kNoise;
  t.a = id;
  t.scale = float(scale);
  return add_tex(s, t);
}

RTMI_EXPORT int rt_nw_tex_image(rt_nw_scene *s, const uint8_t *rgb, int32_t w, int32_t h) {
  if (!s) return set_error(RT_EINVAL, "null scene");
  Image im{};
  if (rgb) {
    if (w <= 0 || h <= 0 || int64_t(w) * h * 3 > (int64_t(1) << 30)) return set_error(RT_EINVAL, "rt_nw_tex_image: bad size");
    if (s->image_px.size() + size_t(w) * h * 3 > (size_t(1) << 31) - 1) return set_error(RT_EINVAL, "rt_nw_tex_image: pool full");
    im.offset = int32_t(s->image_px.size());
    im.w = w;
    im.h = h;
    s->image_px.insert(s->image_px.end(), rgb, rgb + size_t(w) * h * 3);
  }
  s->image.push_back(im);
  Tex t{};
  t.kind = kImage;
  t.a = int32_t(s->image.size()) - 1;
  return add_tex(s, t);
}

RTMI_EXPORT int rt_nw_mat_lambertian(rt_nw_scene *s, int32_t tex) {
  if (!s || !valid_tex(s, tex)) return set_error(RT_EINVAL, "rt_nw_mat_lambertian: bad texture");
  return add_mat(s, Mat{kLambertian, tex, 0.f, 0.f});
}
RTMI_EXPORT int rt_nw_mat_metal(rt_nw_scene *s, int32_t tex, double fuzz) {
  if (!s || !valid_tex(s, tex)) return set_error(RT_EINVAL, "rt_nw_mat_metal: bad texture");
  const float f = float(fuzz);
  return add_mat(s, Mat{kMetal, tex, f < 1.f ? f : 1.f, 0.f});  // material.h:58-62
}
RTMI_EXPORT int rt_nw_mat_dielectric(rt_nw_scene *s, double ir) {
  if (!s || !(ir > 0)) return set_error(RT_EINVAL, "rt_nw_mat_dielectric: bad argument");
  return add_mat(s, Mat{kDielectric, -1, 0.f, float(ir)});
}
RTMI_EXPORT int rt_nw_mat_diffuse_light(rt_nw_scene *s, int32_t tex) {
  if (!s || !valid_tex(s, tex)) return set_error(RT_EINVAL, "rt_nw_mat_diffuse_light: bad texture");
  return add_mat(s, Mat{kDiffuseLight, tex, 0.f, 0.f});
}
RTMI_EXPORT int rt_nw_mat_isotropic(rt_nw_scene *s, int32_t tex) {
  if (!s || !valid_tex(s, tex)) return set_error(RT_EINVAL, "rt_nw_mat_isotropic: bad texture");
  return add_mat(s, Mat{kIsotropic, tex, 0.f, 0.f});
}

RTMI_EXPORT int rt_nw_sphere(rt_nw_scene *s, const double c[3], double r, int32_t mat) {
  if (!s || !c || !valid_mat(s, mat)) return set_error(RT_EINVAL, "rt_nw_sphere: bad argument");
  if (r == 0 || !std::isfinite(r)) return set_error(RT_EINVAL, "rt_nw_sphere: radius must be finite, nonzero");
  SNode n;
  n.kind = kSphere;
  n.mat = mat;
  n.g[0] = c[0]; n.g[1] = c[1]; n.g[2] = c[2]; n.g[3] = r;
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_moving_sphere(rt_nw_scene *s, const double c0[3], const double c1[3], double t0, double t1,
                                    double r, int32_t mat) {
  if (!s || !c0 || !c1 || !valid_mat(s, mat)) return set_error(RT_EINVAL, "rt_nw_moving_sphere: bad argument");
  if (!(t1 != t0) || r == 0) return set_error(RT_EINVAL, "rt_nw_moving_sphere: time0 == time1 or zero radius");
  SNode n;
  n.kind = kMovingSphere;
  n.mat = mat;
  for (int a = 0; a < 3; ++a) {
    n.g[a] = c0[a];
    n.g[4 + a] = c1[a];
  }
  n.g[3] = r;
  n.g[7] = t0;
  n.g[8] = t1;
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_rect(rt_nw_scene *s, int32_t plane, double a0, double a1, double b0, double b1, double k,
                           int32_t mat) {
  if (!s || !valid_mat(s, mat) || plane < RT_NW_XY || plane > RT_NW_YZ) return set_error(RT_EINVAL, "rt_nw_rect: bad argument");
  SNode n;
  n.kind = kRectXY + plane;
  n.mat = mat;
  n.g[0] = a0; n.g[1] = a1; n.g[2] = b0; n.g[3] = b1; n.g[4] = k;
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_box(rt_nw_scene *s, const double p0[3], const double p1[3], int32_t mat) {
  if (!s || !p0 || !p1 || !valid_mat(s, mat)) return set_error(RT_EINVAL, "rt_nw_box: bad argument");
  SNode n;
  n.kind = kBox;
  n.mat = mat;
  for (int a = 0; a < 3; ++a) {
    n.g[a] = p0[a];
    n.g[4 + a] = p1[a];
  }
  return add_node(s, n);
}

// ---------------------------------------------------------------------------
// triangles, meshes and the Wavefront OBJ reader
// ---------------------------------------------------------------------------
namespace {

// One triangle node from three double vertices; the winding is final here.
// Rejected: a coordinate that is not finite as a float, or two vertices equal
// as floats (what the device tests).  Collinear vertices are allowed: such a
// triangle is never hit (build_device_scene leaves it out of the BVH and the
// grid, collinear_triangle).
int add_triangle(rt_nw_scene *s, const double *v0, const double *v1, const double *v2, int32_t mat, const char *who,
                 int32_t attr = -1) {
  const double *v[3] = {v0, v1, v2};
  float f[3][3];
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) {
      f[k][a] = float(v[k][a]);
      if (!std::isfinite(f[k][a])) return set_error(RT_EINVAL, "%s: vertex coordinate not finite", who);
    }
  for (int k = 0; k < 3; ++k) {
    const int j = (k + 1) % 3;
    if (f[k][0] == f[j][0] && f[k][1] == f[j][1] && f[k][2] == f[j][2])
      return set_error(RT_EINVAL, "%s: degenerate triangle (two equal vertices)", who);
  }
  SNode n;
  n.kind = kTriangle;
  n.mat = mat;
  n.attr = attr;
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) n.g[3 * k + a] = v[k][a];
  return add_node(s, n);
}

// Corner attributes of a mesh (rt_nw_mesh_attr, rt_nw_load_obj_attr); flags 0:
// none, add_mesh builds what rt_nw_mesh builds.
struct MeshAttr {
  uint32_t flags = 0;           // RT_NW_MESH_*
  const double *uvs = nullptr;  // RT_NW_MESH_UV: n_uvs pairs
  int32_t n_uvs = 0;
  const int32_t *uvidx = nullptr;  // three per triangle; null: the vertex indices
  bool uv_missing = false;         // a uvidx entry of -1 is a corner without uv (an OBJ face): no uvs for the triangle
};

// The shared builder of rt_nw_mesh and rt_nw_load_obj.  nidx entries may be
// -1 only when allow_missing (an OBJ face without normals keeps its winding).
// line_of (may be null): the file line of each triangle, for error messages.
int add_mesh(rt_nw_scene *s, const double *verts, int32_t n_verts, const int32_t *tri, int32_t n_tris,
             const double *normals, int32_t n_normals, const int32_t *nidx, bool allow_missing, int32_t mat,
             const int32_t *line_of, const char *who, const MeshAttr &at = MeshAttr{}) {
  SNode grp;
  grp.type = kGroup;
  grp.kids.reserve(size_t(n_tris));
  std::string where;
  const bool smooth = (at.flags & RT_NW_MESH_SMOOTH) != 0, want_uv = (at.flags & RT_NW_MESH_UV) != 0;
  // RT_NW_MESH_GEN_NORMALS: per vertex index the sum of cross(v1 - v0, v2 - v0)
  // over the triangles of this call that use it, from the vertices as given
  // (before any exchange), so area-weighted.  (A triangle with an index out of
  // range is skipped here; the loop below refuses it.)
  std::vector<double> gen;
  if (smooth && (at.flags & RT_NW_MESH_GEN_NORMALS)) {
    gen.assign(3 * size_t(n_verts), 0.0);
    for (int32_t t = 0; t < n_tris; ++t) {
      const int32_t *ix = tri + 3 * size_t(t);
      if (ix[0] < 0 || ix[0] >= n_verts || ix[1] < 0 || ix[1] >= n_verts || ix[2] < 0 || ix[2] >= n_verts) continue;
      const double *v0 = verts + 3 * size_t(ix[0]), *v1 = verts + 3 * size_t(ix[1]), *v2 = verts + 3 * size_t(ix[2]);
      const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
      const double fn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) gen[3 * size_t(ix[c]) + a] += fn[a];
    }
  }
  // v / |v| in double, rounded to float; false: zero or not finite
  auto unit_f = [](const double *v, float *out) {
    const double len = std::hypot(v[0], v[1], v[2]);
    if (!(len > 0) || !std::isfinite(len)) return false;
    for (int a = 0; a < 3; ++a) out[a] = float(v[a] / len);
    return true;
  };
  for (int32_t t = 0; t < n_tris; ++t) {
    if (line_of) where = std::string(who) + ": line " + std::to_string(line_of[t]);
    else where = std::string(who) + ": triangle " + std::to_string(t);
    const int32_t *ix = tri + 3 * size_t(t);
    for (int c = 0; c < 3; ++c)
      if (ix[c] < 0 || ix[c] >= n_verts) return set_error(RT_EINVAL, "%s: vertex index %d out of range", where.c_str(), ix[c]);
    const double *v0 = verts + 3 * size_t(ix[0]), *v1 = verts + 3 * size_t(ix[1]), *v2 = verts + 3 * size_t(ix[2]);
    bool swapped = false;
    if (normals) {
      const int32_t *nx = nidx ? nidx + 3 * size_t(t) : ix;
      double ns[3] = {0, 0, 0};
      bool have = true;
      for (int c = 0; c < 3; ++c) {
        if (nx[c] == -1 && allow_missing) { have = false; continue; }
        if (nx[c] < 0 || nx[c] >= n_normals) return set_error(RT_EINVAL, "%s: normal index %d out of range", where.c_str(), nx[c]);
        for (int a = 0; a < 3; ++a) ns[a] += normals[3 * size_t(nx[c]) + a];
      }
      if (have) {  // front = the side of the normals' sum (the OBJ convention)
        const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
        const double fn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        if (fn[0] * ns[0] + fn[1] * ns[1] + fn[2] * ns[2] < 0) {
          std::swap(v1, v2);
          swapped = true;
        }
      }
    }
    int32_t attr = -1;
    if (smooth || want_uv) {
      TriAttr ta{};
      if (smooth) {  // every corner needs a normal: the explicit one, else (GEN_NORMALS) the generated one
        const int32_t *nx = !normals ? nullptr : nidx ? nidx + 3 * size_t(t) : ix;
        bool all = true;
        for (int c = 0; c < 3 && all; ++c) {
          if (nx && nx[c] >= 0) {  // (range-checked above)
            const double *nv = normals + 3 * size_t(nx[c]);
            for (int a = 0; a < 3; ++a)
              if (!std::isfinite(float(nv[a]))) return set_error(RT_EINVAL, "%s: normal %d not finite", where.c_str(), nx[c]);
            if (!unit_f(nv, ta.n + 3 * c)) return set_error(RT_EINVAL, "%s: normal %d has zero length", where.c_str(), nx[c]);
          } else {
            all = !gen.empty() && unit_f(gen.data() + 3 * size_t(ix[c]), ta.n + 3 * c);
          }
        }
        if (all) ta.flags |= 1;
      }
      if (want_uv) {
        const int32_t *ux = at.uvidx ? at.uvidx + 3 * size_t(t) : ix;
        bool all = true;
        for (int c = 0; c < 3; ++c) {
          if (ux[c] == -1 && at.uv_missing) { all = false; continue; }
          if (ux[c] < 0 || ux[c] >= at.n_uvs) return set_error(RT_EINVAL, "%s: uv index %d out of range", where.c_str(), ux[c]);
          for (int a = 0; a < 2; ++a) {
            ta.uv[2 * c + a] = float(at.uvs[2 * size_t(ux[c]) + a]);
            if (!std::isfinite(ta.uv[2 * c + a])) return set_error(RT_EINVAL, "%s: uv %d not finite", where.c_str(), ux[c]);
          }
        }
        if (all) ta.flags |= 2;
      }
      if (swapped) {  // v1 and v2 were exchanged: their normals and uvs go with them
        for (int a = 0; a < 3; ++a) std::swap(ta.n[3 + a], ta.n[6 + a]);
        for (int a = 0; a < 2; ++a) std::swap(ta.uv[2 + a], ta.uv[4 + a]);
      }
      if (!(ta.flags & 1)) std::fill(ta.n, ta.n + 9, 0.f);
      if (!(ta.flags & 2)) std::fill(ta.uv, ta.uv + 6, 0.f);
      if (ta.flags) {
        if (s->attr.size() >= (size_t(1) << 27)) return set_error(RT_EINVAL, "%s: too many attribute records", who);
        s->attr.push_back(ta);
        attr = int32_t(s->attr.size()) - 1;
      }
    }
    const int id = add_triangle(s, v0, v1, v2, mat, where.c_str(), attr);
    if (id < 0) return id;
    grp.kids.push_back(id);
  }
  return add_node(s, grp);
}

}  // namespace

RTMI_EXPORT int rt_nw_triangle(rt_nw_scene *s, const double v0[3], const double v1[3], const double v2[3], int32_t mat) {
  if (!s || !v0 || !v1 || !v2 || !valid_mat(s, mat)) return set_error(RT_EINVAL, "rt_nw_triangle: bad argument");
  return add_triangle(s, v0, v1, v2, mat, "rt_nw_triangle");
}

RTMI_EXPORT int rt_nw_mesh(rt_nw_scene *s, const double *verts, int32_t n_verts, const int32_t *tri_idx, int32_t n_tris,
                           const double *normals, int32_t n_normals, const int32_t *normal_idx, int32_t mat) {
  if (!s || !verts || !tri_idx || n_verts < 1 || n_tris < 1 || !valid_mat(s, mat) || (normals && n_normals < 1) ||
      (!normals && normal_idx))
    return set_error(RT_EINVAL, "rt_nw_mesh: bad argument");
  return add_mesh(s, verts, n_verts, tri_idx, n_tris, normals, n_normals, normal_idx, false, mat, nullptr, "rt_nw_mesh");
}

RTMI_EXPORT int rt_nw_mesh_attr(rt_nw_scene *s, const double *verts, int32_t n_verts, const int32_t *tri_idx, int32_t n_tris,
                                const double *normals, int32_t n_normals, const int32_t *normal_idx, const double *uvs,
                                int32_t n_uvs, const int32_t *uv_idx, uint32_t flags, int32_t mat) {
  if (!s || !verts || !tri_idx || n_verts < 1 || n_tris < 1 || !valid_mat(s, mat) || (normals && n_normals < 1) ||
      (!normals && normal_idx) || (flags & ~uint32_t(RT_NW_MESH_SMOOTH | RT_NW_MESH_UV | RT_NW_MESH_GEN_NORMALS)) ||
      ((flags & RT_NW_MESH_UV) && (!uvs || n_uvs < 1)) || (!uvs && uv_idx))
    return set_error(RT_EINVAL, "rt_nw_mesh_attr: bad argument");
  MeshAttr at;
  at.flags = flags;
  at.uvs = uvs;
  at.n_uvs = n_uvs;
  at.uvidx = uv_idx;
  return add_mesh(s, verts, n_verts, tri_idx, n_tris, normals, n_normals, normal_idx, false, mat, nullptr, "rt_nw_mesh_attr", at);
}

// Wavefront OBJ: v, vn and f (a, a/t, a//n, a/t/n; negative indices count
// back from the latest vertex / normal; polygons fan-triangulated in the
// file's winding) and, for rt_nw_load_obj_attr under RT_NW_MESH_UV only, vt
// and the t of a corner.  Every other statement is ignored.
namespace {
struct ObjFile {
  std::vector<double> verts, normals, uvs;
  std::vector<int32_t> tri, nidx, tidx, line_of;  // nidx / tidx: -1 for a corner without a normal / uv
};
int parse_obj(const char *path, ObjFile &out, bool want_uv = false) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return set_error(RT_EIO, "rt_nw_load_obj: cannot open %s", path);
  std::vector<double> &verts = out.verts, &normals = out.normals, &uvs = out.uvs;
  std::vector<int32_t> &tri = out.tri, &nidx = out.nidx, &tidx = out.tidx, &line_of = out.line_of;
  std::string line;
  int lineno = 0, rc = RT_OK;
  // one number of a v / vn statement: the whole token must parse
  auto number = [](const char *&p, double &out) {
    while (*p == ' ' || *p == '\t') ++p;
    if (!*p) return false;
    char *end = nullptr;
    errno = 0;
    out = std::strtod(p, &end);
    if (end == p || (*end && *end != ' ' && *end != '\t')) return false;
    p = end;
    return true;
  };
  // one integer of a face corner; stops at '/', blank or the end
  auto integer = [](const char *&p, long &out) {
    char *end = nullptr;
    errno = 0;
    out = std::strtol(p, &end, 10);
    if (end == p || errno == ERANGE) return false;
    p = end;
    return true;
  };
  for (bool eof = false; !eof && rc == RT_OK;) {
    line.clear();
    int c;
    while ((c = std::fgetc(f)) != EOF && c != '\n') line.push_back(char(c));
    if (c == EOF) {
      eof = true;
      if (line.empty()) break;
    }
    ++lineno;
    if (line.find('\0') != std::string::npos) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: NUL byte", path, lineno); break; }
    if (const size_t hash = line.find('#'); hash != std::string::npos) line.erase(hash);  // comment
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    const char *p = line.c_str();
    while (*p == ' ' || *p == '\t') ++p;
    const bool is_v = p[0] == 'v' && (p[1] == ' ' || p[1] == '\t');
    const bool is_vn = p[0] == 'v' && p[1] == 'n' && (p[2] == ' ' || p[2] == '\t');
    const bool is_f = p[0] == 'f' && (p[1] == ' ' || p[1] == '\t');
    if (is_v || is_vn) {
      p += is_v ? 1 : 2;
      double x[3];
      for (int a = 0; a < 3 && rc == RT_OK; ++a)
        if (!number(p, x[a])) rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed number", path, lineno);
      if (rc) break;
      if (is_v) {  // an optional w (and vertex colours) may follow: numbers still
        double extra;
        while (*p)
          if (!number(p, extra)) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed number", path, lineno); break; }
        if (rc) break;
      }
      std::vector<double> &dst = is_v ? verts : normals;
      dst.insert(dst.end(), x, x + 3);
    } else if (want_uv && p[0] == 'v' && p[1] == 't' && (p[2] == ' ' || p[2] == '\t' || !p[2])) {
      p += 2;  // vt u [v [w]]: v defaults to 0, w is ignored
      double x[3] = {0, 0, 0};
      int got = 0;
      while (got < 3 && number(p, x[got])) ++got;
      while (*p == ' ' || *p == '\t') ++p;
      if (got < 1 || *p) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed number", path, lineno); break; }
      uvs.insert(uvs.end(), x, x + 2);
    } else if (is_f) {
      p += 1;
      std::vector<int32_t> cv, cn, ct;
      const long nv = long(verts.size() / 3), nn = long(normals.size() / 3), nt = long(uvs.size() / 2);
      for (;;) {
        while (*p == ' ' || *p == '\t') ++p;
        if (!*p) break;
        long iv = 0, in = 0, it = 0;
        bool has_n = false, has_t = false;
        if (!integer(p, iv)) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed face index", path, lineno); break; }
        if (*p == '/') {
          ++p;
          if (*p != '/') {
            if (!integer(p, it)) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed face index", path, lineno); break; }
            has_t = true;
          }
          if (*p == '/') {
            ++p;
            if (!integer(p, in)) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed face index", path, lineno); break; }
            has_n = true;
          }
        }
        if (*p && *p != ' ' && *p != '\t') { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: malformed face index", path, lineno); break; }
        const long av = iv < 0 ? nv + iv : iv - 1, an = !has_n ? -1 : in < 0 ? nn + in : in - 1;
        if (iv == 0 || av < 0 || av >= nv) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: vertex index %ld out of range", path, lineno, iv); break; }
        if (has_n && (in == 0 || an < 0 || an >= nn)) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: normal index %ld out of range", path, lineno, in); break; }
        long at = -1;  // the t of a corner is read under RT_NW_MESH_UV only
        if (want_uv && has_t) {
          at = it < 0 ? nt + it : it - 1;
          if (it == 0 || at < 0 || at >= nt) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: texture index %ld out of range", path, lineno, it); break; }
        }
        cv.push_back(int32_t(av));
        cn.push_back(int32_t(an));
        ct.push_back(int32_t(at));
      }
      if (rc) break;
      if (cv.size() < 3) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: line %d: face with fewer than three corners", path, lineno); break; }
      // a face with a corner lacking t gets no uvs
      const bool face_uv = std::find(ct.begin(), ct.end(), -1) == ct.end();
      for (size_t k = 1; k + 1 < cv.size(); ++k) {  // fan about the first corner
        const size_t c3[3] = {0, k, k + 1};
        for (size_t q : c3) {
          tri.push_back(cv[q]);
          nidx.push_back(cn[q]);
          tidx.push_back(face_uv ? ct[q] : -1);
        }
        line_of.push_back(lineno);
      }
      if (tri.size() / 3 >= (size_t(1) << 27)) { rc = set_error(RT_EINVAL, "rt_nw_load_obj: %s: too many triangles", path); break; }
    }
    // vt, o, g, s, usemtl, mtllib, comments, blank lines, anything else: ignored
  }
  const bool io_error = std::ferror(f) != 0;
  std::fclose(f);
  if (rc) return rc;
  if (io_error) return set_error(RT_EIO, "rt_nw_load_obj: read error in %s", path);
  if (tri.empty()) return set_error(RT_EINVAL, "rt_nw_load_obj: %s: no faces", path);
  return RT_OK;
}
int add_obj_mesh(rt_nw_scene *s, const char *path, const ObjFile &o, int32_t mat, int32_t *n_tris, uint32_t flags = 0) {
  const int32_t nt = int32_t(o.tri.size() / 3);
  const std::string who = std::string("rt_nw_load_obj: ") + path;
  const bool nrm = !o.normals.empty();
  MeshAttr at;
  at.flags = flags;
  if (flags & RT_NW_MESH_UV) {
    at.uvs = o.uvs.data();
    at.n_uvs = int32_t(o.uvs.size() / 2);
    at.uvidx = o.tidx.data();
    at.uv_missing = true;
  }
  const int id = add_mesh(s, o.verts.data(), int32_t(o.verts.size() / 3), o.tri.data(), nt, nrm ? o.normals.data() : nullptr,
                          int32_t(o.normals.size() / 3), nrm ? o.nidx.data() : nullptr, true, mat, o.line_of.data(), who.c_str(), at);
  if (id >= 0 && n_tris) *n_tris = nt;
  return id;
}
bool mesh_flags_ok(uint32_t flags) {
  return !(flags & ~uint32_t(RT_NW_MESH_SMOOTH | RT_NW_MESH_UV | RT_NW_MESH_GEN_NORMALS));
}
}  // namespace

RTMI_EXPORT int rt_nw_load_obj_attr(rt_nw_scene *s, const char *path, int32_t mat, uint32_t flags, int32_t *n_tris) {
  if (!s || !path || !valid_mat(s, mat) || !mesh_flags_ok(flags)) return set_error(RT_EINVAL, "rt_nw_load_obj_attr: bad argument");
  ObjFile o;
  if (int rc = parse_obj(path, o, (flags & RT_NW_MESH_UV) != 0)) return rc;
  return add_obj_mesh(s, path, o, mat, n_tris, flags);
}

RTMI_EXPORT int rt_nw_load_obj(rt_nw_scene *s, const char *path, int32_t mat, int32_t *n_tris) {
  if (!s || !path || !valid_mat(s, mat)) return set_error(RT_EINVAL, "rt_nw_load_obj: bad argument");
  ObjFile o;
  if (int rc = parse_obj(path, o)) return rc;
  return add_obj_mesh(s, path, o, mat, n_tris);
}

// The scene of `rtmi_nw_render --obj`: the file's mesh scaled (uniformly) and
// centred into the box [-1, 1] x [0, 2] x [-1, 1] — its largest extent 2 units,
// standing on y = 0 — on a checker ground (a sphere of radius 1000 below it),
// one 3 x 3 xz_rect light of emission 6 at y = 5 and the background (0.05,
// 0.07, 0.12).  Camera: from (3.2, 2.4, 4.8) at the box centre (0, 1, 0),
// vfov 30, no aperture.
// rt_nw_scene_obj_stage_attr: the same stage with the mesh loaded under `flags`
// (rt_nw_load_obj_attr) and, when rgb is given, that image as the texture of
// the mesh's lambertian or metal material.
namespace {
int obj_stage(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags, const uint8_t *rgb, int32_t w, int32_t h,
              double aspect, rt_nw_camera *cam, int32_t *n_tris, int32_t copies = 1, const double *move = nullptr,
              bool tumble = false) {
  if (!s || !path || !cam || !(aspect > 0) || !mesh_flags_ok(flags)) return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: bad argument");
  if (move && !(std::isfinite(float(move[0])) && std::isfinite(float(move[1])) && std::isfinite(float(move[2]))))
    return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: move vector not finite");
  if (copies < 1 || copies > 256) return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: copies must be in 1..256");
  if (mat_kind != RT_NW_LAMBERTIAN && mat_kind != RT_NW_METAL && mat_kind != RT_NW_DIELECTRIC)
    return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: material must be lambertian, metal or dielectric");
  if (rgb && mat_kind == RT_NW_DIELECTRIC) return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: a dielectric takes no texture image");
  if (rgb && (w <= 0 || h <= 0)) return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: bad image size");
  ObjFile o;
  if (int rc = parse_obj(path, o, (flags & RT_NW_MESH_UV) != 0)) return rc;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int32_t ix : o.tri)  // the vertices the faces use
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], o.verts[3 * size_t(ix) + a]);
      hi[a] = std::max(hi[a], o.verts[3 * size_t(ix) + a]);
    }
  const double ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
  if (!(ext > 0) || !std::isfinite(ext)) return set_error(RT_EINVAL, "rt_nw_scene_obj_stage: %s: mesh without extent", path);
  const double k = 2.0 / ext, c[3] = {0.5 * (lo[0] + hi[0]), lo[1], 0.5 * (lo[2] + hi[2])};
  for (size_t i = 0; i < o.verts.size(); ++i) o.verts[i] = (o.verts[i] - c[i % 3]) * k;
  int rc = RT_OK;
  auto chk = [&](int v) {
    if (v < 0 && rc == RT_OK) rc = v;
    return v;
  };
  const int mat = mat_kind == RT_NW_LAMBERTIAN
                      ? chk(rt_nw_mat_lambertian(s, chk(rgb ? rt_nw_tex_image(s, rgb, w, h) : rt_nw_tex_solid(s, 0.7, 0.35, 0.2))))
                  : mat_kind == RT_NW_METAL
                      ? chk(rt_nw_mat_metal(s, chk(rgb ? rt_nw_tex_image(s, rgb, w, h) : rt_nw_tex_solid(s, 0.8, 0.8, 0.85)), 0.05))
                      : chk(rt_nw_mat_dielectric(s, 1.5));
  if (rc) return rc;
  const int mesh = chk(add_obj_mesh(s, path, o, mat, n_tris, flags));
  const double gc[3] = {0, -1000, 0};
  const int ground = chk(rt_nw_sphere(s, gc, 1000, chk(rt_nw_mat_lambertian(s, chk(rt_nw_tex_checker(
                                                      s, chk(rt_nw_tex_solid(s, 0.2, 0.3, 0.1)), chk(rt_nw_tex_solid(s, 0.9, 0.9, 0.9))))))));
  const int light = chk(rt_nw_rect(s, RT_NW_XZ, -1.5, 1.5, -1.5, 1.5, 5.0, chk(rt_nw_mat_diffuse_light(s, chk(rt_nw_tex_solid(s, 6, 6, 6))))));
  if (rc) return rc;
  chk(rt_nw_world_add(s, ground));
  const double still[3] = {0, 0, 0};
  // --obj-tumble: copy q as an affine placement (rt_nw_transform) at its field
  // position — uniform scale 0.75 + 0.25 sin(2.9 q), turned 37 q degrees about
  // normalize(sin 1.3 q, 1, cos 0.7 q), lifted until the lowest corner of its
  // transformed stage box [-1, 1] x [0, 2] x [-1, 1] stands on y = 0
  auto tumbled = [&](int shared, int q, const double off[3]) {
    const double sc = 0.75 + 0.25 * std::sin(2.9 * q), th = 37.0 * q * M_PI / 180.0;
    double ax[3] = {std::sin(1.3 * q), 1.0, std::cos(0.7 * q)};
    const double al = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    for (double &v : ax) v /= al;
    const double c = std::cos(th), sn = std::sin(th), k1 = 1.0 - c;
    const double R[9] = {c + k1 * ax[0] * ax[0],          k1 * ax[0] * ax[1] - sn * ax[2], k1 * ax[0] * ax[2] + sn * ax[1],
                         k1 * ax[1] * ax[0] + sn * ax[2], c + k1 * ax[1] * ax[1],          k1 * ax[1] * ax[2] - sn * ax[0],
                         k1 * ax[2] * ax[0] - sn * ax[1], k1 * ax[2] * ax[1] + sn * ax[0], c + k1 * ax[2] * ax[2]};
    double low = INFINITY;
    for (int i = 0; i < 8; ++i) {
      const double p[3] = {(i & 1) ? 1.0 : -1.0, (i & 2) ? 2.0 : 0.0, (i & 4) ? 1.0 : -1.0};
      low = std::min(low, sc * (R[3] * p[0] + R[4] * p[1] + R[5] * p[2]));
    }
    const double m[12] = {sc * R[0], sc * R[1], sc * R[2], off[0], sc * R[3], sc * R[4], sc * R[5], off[1] - low,
                          sc * R[6], sc * R[7], sc * R[8], off[2]};
    return rt_nw_transform(s, shared, m);
  };
  if (copies == 1 && tumble) {
    const int placed = chk(tumbled(chk(rt_nw_shared(s, mesh)), 0, still));
    chk(rt_nw_world_add(s, move ? chk(rt_nw_move(s, placed, still, move, 0.0, 1.0)) : placed));
  } else if (copies == 1 && move) {  // one moving placement of the model as a shared mesh
    chk(rt_nw_world_add(s, chk(rt_nw_move(s, chk(rt_nw_shared(s, mesh)), still, move, 0.0, 1.0))));
  } else if (copies == 1) {
    chk(rt_nw_world_add(s, mesh));
  } else {
    // copies x copies placements of the one shared mesh, 3 units apart and
    // centred on the origin; copy (i, k) is turned by 37 (i * copies + k)
    // degrees, and nudged by up to 0.4 units along x and z (a fixed formula)
    const int shared = chk(rt_nw_shared(s, mesh));
    if (rc) return rc;
    for (int i = 0; i < copies; ++i)
      for (int k = 0; k < copies; ++k) {
        const int q = i * copies + k;
        const double off[3] = {3.0 * (i - 0.5 * (copies - 1)) + 0.4 * std::sin(1.7 * q), 0.0,
                               3.0 * (k - 0.5 * (copies - 1)) + 0.4 * std::cos(2.3 * q)};
        const int placed = tumble ? chk(tumbled(shared, q, off)) : chk(rt_nw_translate(s, chk(rt_nw_rotate_y(s, shared, 37.0 * q)), off));
        chk(rt_nw_world_add(s, move ? chk(rt_nw_move(s, placed, still, move, 0.0, 1.0)) : placed));
        if (rc) return rc;
      }
  }
  chk(rt_nw_world_add(s, light));
  chk(rt_nw_set_background(s, 0.05, 0.07, 0.12));
  if (rc) return rc;
  // the camera backs away along its line of sight with the field's extent
  const double back = copies == 1 ? 1.0 : 0.5 + 0.75 * copies;
  const double from[3] = {3.2 * back, copies == 1 ? 2.4 : 1.0 + 1.4 * back, 4.8 * back}, at[3] = {0, 1, 0}, vup[3] = {0, 1, 0};
  const double dist = std::sqrt(3.2 * 3.2 + 1.4 * 1.4 + 4.8 * 4.8) * back;
  return rt_nw_camera_init(cam, from, at, vup, 30.0, aspect, 0.0, dist, 0.0, 1.0);
}
}  // namespace

RTMI_EXPORT int rt_nw_scene_obj_stage(rt_nw_scene *s, const char *path, int32_t mat_kind, double aspect, rt_nw_camera *cam,
                                      int32_t *n_tris) {
  return obj_stage(s, path, mat_kind, 0, nullptr, 0, 0, aspect, cam, n_tris);
}

RTMI_EXPORT int rt_nw_scene_obj_stage_attr(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags,
                                           const uint8_t *rgb, int32_t w, int32_t h, double aspect, rt_nw_camera *cam,
                                           int32_t *n_tris) {
  return obj_stage(s, path, mat_kind, flags, rgb, w, h, aspect, cam, n_tris);
}

RTMI_EXPORT int rt_nw_scene_obj_stage_copies(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags,
                                             const uint8_t *rgb, int32_t w, int32_t h, int32_t copies, double aspect,
                                             rt_nw_camera *cam, int32_t *n_tris) {
  return obj_stage(s, path, mat_kind, flags, rgb, w, h, aspect, cam, n_tris, copies);
}

RTMI_EXPORT int rt_nw_scene_obj_stage_moving(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags,
                                             const uint8_t *rgb, int32_t w, int32_t h, int32_t copies, const double move[3],
                                             double aspect, rt_nw_camera *cam, int32_t *n_tris) {
  if (!move) return set_error(RT_EINVAL, "rt_nw_scene_obj_stage_moving: null move vector");
  return obj_stage(s, path, mat_kind, flags, rgb, w, h, aspect, cam, n_tris, copies, move);
}

RTMI_EXPORT int rt_nw_scene_obj_stage_tumbled(rt_nw_scene *s, const char *path, int32_t mat_kind, uint32_t flags,
                                              const uint8_t *rgb, int32_t w, int32_t h, int32_t copies, const double *move,
                                              double aspect, rt_nw_camera *cam, int32_t *n_tris) {
  return obj_stage(s, path, mat_kind, flags, rgb, w, h, aspect, cam, n_tris, copies, move, true);
}

RTMI_EXPORT int rt_nw_constant_medium(rt_nw_scene *s, int32_t boundary, double density, int32_t tex) {
  if (!s || !valid_node(s, boundary) || !valid_tex(s, tex) || !(density > 0))
    return set_error(RT_EINVAL, "rt_nw_constant_medium: bad argument");
  {  // a triangle (under any translate / rotate_y chain) bounds no volume
    int32_t b = boundary;
    while (valid_node(s, b) && (s->nodes[b].type == kTranslate || s->nodes[b].type == kRotate || s->nodes[b].type == kMove ||
                                s->nodes[b].type == kTransform))
      b = s->nodes[b].child;
    if (valid_node(s, b) && ((s->nodes[b].type == kPrim && s->nodes[b].kind == kTriangle) || s->nodes[b].type == kShared))
      return set_error(RT_EUNSUPPORTED, "rt_nw_constant_medium: a triangle cannot be a medium's boundary");
  }
  const int m = rt_nw_mat_isotropic(s, tex);  // phase_function = new isotropic(a) constant_medium.h:12-17
  if (m < 0) return m;
  SNode n;
  n.type = kMediumNode;
  n.child = boundary;
  n.density = density;
  n.phase_mat = m;
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_medium_samples(rt_nw_scene *s, int32_t medium, int32_t samples) {
  if (!s || !valid_node(s, medium) || s->nodes[medium].type != kMediumNode || samples < 1 || samples > 8)
    return set_error(RT_EINVAL, "rt_nw_medium_samples: bad medium or samples not in 1..8");
  s->nodes[medium].samples = samples;
  s->flat_valid = false;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_group(rt_nw_scene *s, const int32_t *objects, int32_t count) {
  if (!s || (count > 0 && !objects) || count < 0) return set_error(RT_EINVAL, "rt_nw_group: bad argument");
  SNode n;
  n.type = kGroup;
  for (int i = 0; i < count; ++i) {
    if (!valid_node(s, objects[i])) return set_error(RT_EINVAL, "rt_nw_group: bad object %d", objects[i]);
    n.kids.push_back(objects[i]);
  }
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_translate(rt_nw_scene *s, int32_t object, const double offset[3]) {
  if (!s || !offset || !valid_node(s, object)) return set_error(RT_EINVAL, "rt_nw_translate: bad argument");
  SNode n;
  n.type = kTranslate;
  n.child = object;
  for (int a = 0; a < 3; ++a) n.off[a] = offset[a];
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_rotate_y(rt_nw_scene *s, int32_t object, double angle_deg) {
  if (!s || !valid_node(s, object) || !std::isfinite(angle_deg)) return set_error(RT_EINVAL, "rt_nw_rotate_y: bad argument");
  SNode n;
  n.type = kRotate;
  n.child = object;
  n.angle = angle_deg;
  return add_node(s, n);
}

namespace {
// the subtree of a shared handle: triangles and groups of them; counts the triangles
int shared_subtree(const rt_nw_scene *s, int32_t id, int depth, int64_t &n_tris) {
  if (depth > 64) return set_error(RT_EINVAL, "rt_nw_shared: object nesting deeper than 64 (a cycle?)");
  const SNode &n = s->nodes[size_t(id)];
  if (n.type == kPrim && n.kind == kTriangle) {
    ++n_tris;
    return RT_OK;
  }
  if (n.type == kGroup) {
    for (int32_t k : n.kids)
      if (int rc = shared_subtree(s, k, depth + 1, n_tris)) return rc;
    return RT_OK;
  }
  return set_error(RT_EUNSUPPORTED, "rt_nw_shared: only triangles and groups of them can be shared geometry");
}
}  // namespace

RTMI_EXPORT int rt_nw_shared(rt_nw_scene *s, int32_t object) {
  if (!s || !valid_node(s, object)) return set_error(RT_EINVAL, "rt_nw_shared: bad argument");
  int64_t n_tris = 0;
  if (int rc = shared_subtree(s, object, 0, n_tris)) return rc;
  if (n_tris == 0) return set_error(RT_EINVAL, "rt_nw_shared: no triangle under object %d", object);
  SNode n;
  n.type = kShared;
  n.child = object;
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_move(rt_nw_scene *s, int32_t object, const double offset0[3], const double offset1[3], double time0,
                           double time1) {
  if (!s || !offset0 || !offset1 || !valid_node(s, object)) return set_error(RT_EINVAL, "rt_nw_move: bad argument");
  if (!std::isfinite(float(time0)) || !std::isfinite(float(time1)) || float(time0) == float(time1))
    return set_error(RT_EINVAL, "rt_nw_move: times must be finite and differ (as floats: the kernels divide by their difference)");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(float(offset0[a])) || !std::isfinite(float(offset1[a])))
      return set_error(RT_EINVAL, "rt_nw_move: offset not finite");
  // under it: one shared handle, optionally under translate / rotate_y / transform nodes
  int32_t b = object;
  for (int depth = 0; s->nodes[size_t(b)].type == kTranslate || s->nodes[size_t(b)].type == kRotate ||
                      s->nodes[size_t(b)].type == kTransform;
       ++depth) {
    if (depth > 64) return set_error(RT_EINVAL, "rt_nw_move: object nesting deeper than 64 (a cycle?)");
    b = s->nodes[size_t(b)].child;
  }
  if (s->nodes[size_t(b)].type == kMove) return set_error(RT_EUNSUPPORTED, "rt_nw_move: a move under a move");
  if (s->nodes[size_t(b)].type != kShared)
    return set_error(RT_EUNSUPPORTED, "rt_nw_move: only a placement of a shared mesh (rt_nw_shared) can move");
  SNode n;
  n.type = kMove;
  n.child = object;
  for (int a = 0; a < 3; ++a) {
    n.off[a] = offset0[a];
    n.off1[a] = offset1[a];
  }
  n.time0 = time0;
  n.time1 = time1;
  ++s->n_moves;
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_transform(rt_nw_scene *s, int32_t object, const double m[12]) {
  if (!s || !m || !valid_node(s, object)) return set_error(RT_EINVAL, "rt_nw_transform: bad argument");
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(m[i]) || !std::isfinite(float(m[i]))) return set_error(RT_EINVAL, "rt_nw_transform: entry %d not finite as a float", i);
  const double A[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
  double inv[9];
  if (!affine_inverse(A, inv))
    return set_error(RT_EINVAL,
                     "rt_nw_transform: the 3x3 part must have a positive determinant (no mirror) and |A|_F |A^-1|_F <= %g",
                     kAffineCond);
  // under it: one shared handle, optionally under translate / rotate_y /
  // transform nodes and at most one move (rt_nw_move sees to that)
  int32_t b = object;
  for (int depth = 0; s->nodes[size_t(b)].type == kTranslate || s->nodes[size_t(b)].type == kRotate ||
                      s->nodes[size_t(b)].type == kTransform || s->nodes[size_t(b)].type == kMove;
       ++depth) {
    if (depth > 64) return set_error(RT_EINVAL, "rt_nw_transform: object nesting deeper than 64 (a cycle?)");
    b = s->nodes[size_t(b)].child;
  }
  if (s->nodes[size_t(b)].type != kShared)
    return set_error(RT_EUNSUPPORTED, "rt_nw_transform: only a placement of a shared mesh (rt_nw_shared) takes an affine map");
  SNode n;
  n.type = kTransform;
  n.child = object;
  for (int i = 0; i < 12; ++i) n.g[i] = m[i];
  return add_node(s, n);
}

RTMI_EXPORT int rt_nw_scene_affine_stats(rt_nw_scene *s, int32_t out[2]) {
  if (!s || !out) return set_error(RT_EINVAL, "rt_nw_scene_affine_stats: null");
  if (int rc = flatten(s)) return rc;
  out[0] = out[1] = 0;
  for (const rt_nw_scene::Place &p : s->flat_place) ++out[p.x.affine ? 0 : 1];
  return RT_OK;
}

RTMI_EXPORT int rt_nw_scene_motion_stats(rt_nw_scene *s, int32_t out[2]) {
  if (!s || !out) return set_error(RT_EINVAL, "rt_nw_scene_motion_stats: null");
  if (int rc = flatten(s)) return rc;
  out[0] = out[1] = 0;
  for (const rt_nw_scene::Place &p : s->flat_place) ++out[p.x.moving ? 0 : 1];
  return RT_OK;
}

RTMI_EXPORT int rt_nw_scene_instancing_stats(rt_nw_scene *s, int32_t out[6]) {
  return rtmi::nw::scene_instancing_stats(s, out);
}

RTMI_EXPORT int rt_nw_world_add(rt_nw_scene *s, int32_t object) {
  if (!s || !valid_node(s, object)) return set_error(RT_EINVAL, "rt_nw_world_add: bad object");
  s->world.push_back(object);
  s->flat_valid = false;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_set_background(rt_nw_scene *s, double r, double g, double b) {
  if (!s) return set_error(RT_EINVAL, "null scene");
  s->background[0] = float(r);
  s->background[1] = float(g);
  s->background[2] = float(b);
  return RT_OK;
}

RTMI_EXPORT int rt_nw_scene_grid_stats(rt_nw_scene *s, int32_t *dims3, int32_t *max_cell, int32_t *n_big,
                                       int32_t *n_refs) {
  return rtmi::nw::scene_grid_stats(s, dims3, max_cell, n_big, n_refs);
}

RTMI_EXPORT int rt_nw_scene_flat(rt_nw_scene *s, rt_nw_flat *out) { return rt_nw_scene_flat_at(s, 0.0, out); }

RTMI_EXPORT int rt_nw_scene_flat_at(rt_nw_scene *s, double time, rt_nw_flat *out) {
  if (!s || !out) return set_error(RT_EINVAL, "null");
  const float tf = float(time);
  if (!std::isfinite(tf)) return set_error(RT_EINVAL, "rt_nw_scene_flat_at: time not finite");
  if (int rc = flatten(s, &tf)) return rc;
  out->n_obj = int32_t(s->flat_obj.size());
  out->n_inst = int32_t(s->flat_inst.size());
  out->n_mat = int32_t(s->mat.size());
  out->n_tex = int32_t(s->tex.size());
  out->n_perlin = int32_t(s->perlin_perm.size() / (3 * kPerlinN));
  out->n_image = int32_t(s->image.size());
  out->obj = reinterpret_cast<const float *>(s->flat_obj.data());
  out->inst = reinterpret_cast<const float *>(s->flat_inst.data());
  out->mat = reinterpret_cast<const float *>(s->mat.data());
  out->tex = reinterpret_cast<const float *>(s->tex.data());
  out->perlin_vec = s->perlin_vec.data();
  out->perlin_perm = s->perlin_perm.data();
  out->image_desc = reinterpret_cast<const int32_t *>(s->image.data());
  out->image_px = s->image_px.data();
  out->image_bytes = int64_t(s->image_px.size());
  for (int c = 0; c < 3; ++c) out->background[c] = s->background[c];
  return RT_OK;
}

RTMI_EXPORT int rt_nw_scene_flat_attr(rt_nw_scene *s, int32_t *n_attr, const float **attr, const int32_t **attr_of_obj) {
  if (!s || !n_attr || !attr || !attr_of_obj) return set_error(RT_EINVAL, "null");
  if (int rc = flatten(s)) return rc;
  const bool baked = !s->flat_attr_pub.empty();  // an affine placement with attribute records
  const std::vector<TriAttr> &rec = baked ? s->flat_attr_view : s->attr;
  *n_attr = int32_t(rec.size());
  *attr = reinterpret_cast<const float *>(rec.data());
  *attr_of_obj = baked ? s->flat_attr_pub.data() : s->flat_attr.data();
  return RT_OK;
}

// ---------------------------------------------------------------------------
// scene hash and checkpoint files of the progressive accumulator (rtmi_nw.h)
// ---------------------------------------------------------------------------
namespace {
constexpr uint64_t kFnvBasis = 14695981039346656037ull, kFnvPrime = 1099511628211ull;
struct Fnv {
  uint64_t h = kFnvBasis;
  void bytes(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * kFnvPrime;
  }
  void i64(int64_t v) { bytes(&v, sizeof v); }
  template <class T> void table(const std::vector<T> &v) {  // count, then the records' bytes
    i64(int64_t(v.size()));
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
};
constexpr char kCkptMagic[8] = {'R', 'T', 'M', 'I', 'N', 'W', 'A', '1'};
}  // namespace

// The serialisation is written out beside the declaration (rtmi_nw.h).  Every
// record type below is made of 4-byte fields without padding, and the builder
// zero-fills the words it does not use.
RTMI_EXPORT int rt_nw_scene_hash(rt_nw_scene *s, uint64_t *out) {
  if (!s || !out) return set_error(RT_EINVAL, "rt_nw_scene_hash: null argument");
  // the flat view at time 0; a caller's view at another time is put back
  const bool had = s->flat_valid;
  const float t_had = s->flat_time, t0 = 0.f;
  if (int rc = flatten(s, &t0)) return rc;
  Fnv f;
  f.bytes("RTMINWS1", 8);
  f.table(s->flat_obj);
  f.table(s->flat_inst);
  f.table(s->mat);
  f.table(s->tex);
  f.table(s->perlin_vec);
  f.table(s->perlin_perm);
  f.table(s->image);
  f.table(s->image_px);
  f.bytes(s->background, sizeof s->background);
  f.table(s->attr);
  f.table(s->flat_attr);
  f.i64(int64_t(s->flat_place.size()));
  for (const rt_nw_scene::Place &p : s->flat_place) {
    const int32_t w[3] = {p.first, p.count, (p.x.moving ? 1 : 0) | (p.x.affine ? 2 : 0)};
    f.bytes(w, sizeof w);
    if (p.x.moving) {  // what the kernels form off(T) from (build_device_scene)
      float o[6];
      motion_ends(p.x, o, o + 3);
      const float t[2] = {float(p.x.time0), float(p.x.time1)};
      f.bytes(o, sizeof o);
      f.bytes(t, sizeof t);
    }
    if (p.x.affine) {  // the placement's AffInst rows: M = float(A^-1), off = float(b)
      double inv[9];
      (void)affine_inverse(p.x.A, inv);  // (checked when the world was flattened)
      float m[12];
      for (int i = 0; i < 9; ++i) m[i] = float(inv[i]);
      for (int a = 0; a < 3; ++a) m[9 + a] = float(p.x.t[a]);
      f.bytes(m, sizeof m);
    }
  }
  *out = f.h;
  if (had && s->n_moves > 0 && std::memcmp(&t_had, &t0, sizeof(float)) != 0) return flatten(s, &t_had);
  return RT_OK;
}

namespace rtmi {
namespace nw {

uint64_t camera_hash(const rt_nw_camera *cam) {
  static_assert(sizeof(rt_nw_camera) % sizeof(double) == 0, "rt_nw_camera is doubles only: no padding to hash");
  Fnv f;
  f.bytes(cam, sizeof *cam);
  return f.h;
}

int ckpt_write(const char *path, const CkptHeader &h_in, const int64_t *raw) {
  if (!path || !raw || h_in.W < 1 || h_in.nrows < 0) return set_error(RT_EINVAL, "rt_nw_accum_save: bad argument");
  CkptHeader h = h_in;
  std::memcpy(h.magic, kCkptMagic, 8);
  h.zero = 0;
  const size_t n = size_t(h.W) * size_t(h.nrows) * 3;
  const std::string tmp = std::string(path) + ".tmp";
  FILE *fp = std::fopen(tmp.c_str(), "wb");
  if (!fp) return set_error(RT_EIO, "rt_nw_accum_save: cannot open %s", tmp.c_str());
  bool ok = std::fwrite(&h, sizeof h, 1, fp) == 1 && (n == 0 || std::fwrite(raw, sizeof(int64_t), n, fp) == n);
  if (std::fclose(fp) != 0) ok = false;
  if (!ok || std::rename(tmp.c_str(), path) != 0) {
    std::remove(tmp.c_str());
    return set_error(RT_EIO, "rt_nw_accum_save: write to %s failed", path);
  }
  return RT_OK;
}

int ckpt_read(const char *path, CkptHeader &h, std::vector<int64_t> *raw) {
  if (!path) return set_error(RT_EINVAL, "null path");
  FILE *fp = std::fopen(path, "rb");
  if (!fp) return set_error(RT_EIO, "cannot open %s", path);
  CkptHeader r{};
  if (std::fread(&r, sizeof r, 1, fp) != 1 || std::memcmp(r.magic, kCkptMagic, 8) != 0) {
    std::fclose(fp);
    return set_error(RT_EIO, "%s is not a Next-Week checkpoint", path);
  }
  h = r;
  if (!raw) {
    std::fclose(fp);
    return RT_OK;
  }
  // the body's size comes from the header: bounded before anything is allocated
  const bool sane = r.W >= 1 && r.nrows >= 0 && int64_t(r.W) * r.nrows < (int64_t(1) << 40);
  bool ok = sane && std::fseek(fp, 0, SEEK_END) == 0;
  const long end = ok ? std::ftell(fp) : -1;
  const uint64_t n = sane ? uint64_t(r.W) * uint64_t(r.nrows) * 3 : 0;
  ok = ok && end >= 0 && uint64_t(end) == sizeof r + n * sizeof(int64_t) && std::fseek(fp, long(sizeof r), SEEK_SET) == 0;
  if (ok) {
    raw->resize(size_t(n));
    ok = n == 0 || std::fread(raw->data(), sizeof(int64_t), size_t(n), fp) == size_t(n);
  }
  std::fclose(fp);
  if (!ok) return set_error(RT_EIO, "%s is truncated, or holds more than its header states", path);
  return RT_OK;
}

namespace {
constexpr char kAdaptMagic[8] = {'R', 'T', 'M', 'I', 'N', 'W', 'D', '1'};
}

int adapt_ckpt_write(const char *path, const CkptHeader &h_in, const int64_t *sum, const uint64_t *m2, const int32_t *n) {
  if (!path || !sum || !m2 || !n || h_in.W < 1 || h_in.nrows < 1) return set_error(RT_EINVAL, "rt_nw_adapt_save: bad argument");
  CkptHeader h = h_in;
  std::memcpy(h.magic, kAdaptMagic, 8);
  h.zero = 0;
  const size_t npix = size_t(h.W) * size_t(h.nrows);
  const std::string tmp = std::string(path) + ".tmp";
  FILE *fp = std::fopen(tmp.c_str(), "wb");
  if (!fp) return set_error(RT_EIO, "rt_nw_adapt_save: cannot open %s", tmp.c_str());
  bool ok = std::fwrite(&h, sizeof h, 1, fp) == 1 && std::fwrite(sum, sizeof(int64_t), npix * 3, fp) == npix * 3 &&
            std::fwrite(m2, sizeof(uint64_t), npix, fp) == npix && std::fwrite(n, sizeof(int32_t), npix, fp) == npix;
  if (std::fclose(fp) != 0) ok = false;
  if (!ok || std::rename(tmp.c_str(), path) != 0) {
    std::remove(tmp.c_str());
    return set_error(RT_EIO, "rt_nw_adapt_save: write to %s failed", path);
  }
  return RT_OK;
}

int adapt_ckpt_read(const char *path, CkptHeader &h, std::vector<int64_t> *sum, std::vector<uint64_t> *m2, std::vector<int32_t> *n) {
  if (!path) return set_error(RT_EINVAL, "null path");
  FILE *fp = std::fopen(path, "rb");
  if (!fp) return set_error(RT_EIO, "cannot open %s", path);
  CkptHeader r{};
  if (std::fread(&r, sizeof r, 1, fp) != 1 || std::memcmp(r.magic, kAdaptMagic, 8) != 0) {
    std::fclose(fp);
    return set_error(RT_EIO, "%s is not a Next-Week adaptive checkpoint", path);
  }
  h = r;
  if (!sum || !m2 || !n) {
    std::fclose(fp);
    return RT_OK;
  }
  // the body's size comes from the header: bounded before anything is allocated
  const bool sane = r.W >= 1 && r.nrows >= 1 && int64_t(r.W) * r.nrows < (int64_t(1) << 40);
  bool ok = sane && std::fseek(fp, 0, SEEK_END) == 0;
  const long end = ok ? std::ftell(fp) : -1;
  const uint64_t npix = sane ? uint64_t(r.W) * uint64_t(r.nrows) : 0;
  ok = ok && end >= 0 && uint64_t(end) == sizeof r + npix * (3 * sizeof(int64_t) + sizeof(uint64_t) + sizeof(int32_t)) &&
       std::fseek(fp, long(sizeof r), SEEK_SET) == 0;
  if (ok) {
    sum->resize(size_t(npix) * 3);
    m2->resize(size_t(npix));
    n->resize(size_t(npix));
    ok = std::fread(sum->data(), sizeof(int64_t), size_t(npix) * 3, fp) == size_t(npix) * 3 &&
         std::fread(m2->data(), sizeof(uint64_t), size_t(npix), fp) == size_t(npix) &&
         std::fread(n->data(), sizeof(int32_t), size_t(npix), fp) == size_t(npix);
  }
  std::fclose(fp);
  if (!ok) return set_error(RT_EIO, "%s is truncated, or holds more than its header states", path);
  return RT_OK;
}

}  // namespace nw
}  // namespace rtmi

RTMI_EXPORT int rt_nw_adapt_info(const char *path, int32_t out8[8], uint64_t out3[3]) {
  if (!path || !out8 || !out3) return set_error(RT_EINVAL, "rt_nw_adapt_info: null argument");
  CkptHeader h{};
  std::vector<int64_t> sum;
  std::vector<uint64_t> m2;
  std::vector<int32_t> n;
  if (int rc = adapt_ckpt_read(path, h, &sum, &m2, &n)) return rc;  // (the body too: a truncated file is refused)
  const int32_t v[8] = {h.W, h.H, h.row0, h.row_step, h.nrows, h.spp_done, h.max_depth, h.zero};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  out3[0] = h.seed;
  out3[1] = h.scene_hash;
  out3[2] = h.camera_hash;
  return RT_OK;
}

// The stopping rule of adaptive sampling, per pixel in float64 (this file is compiled without contraction), in the
// order the header states.  A pixel with fewer than two samples has no variance estimate: its err is +inf.  A
// threshold of exactly 0 keeps every pixel below max_spp active.
RTMI_EXPORT int rt_nw_adapt_criterion(const int64_t *sum, const uint64_t *m2, const int32_t *n, int32_t W, int32_t nrows,
                                      int32_t min_spp, int32_t max_spp, double threshold, double floor, int32_t dilate,
                                      uint8_t *active, double *err, int64_t *n_active) {
  if (!sum || !m2 || !n || !active) return set_error(RT_EINVAL, "rt_nw_adapt_criterion: null argument");
  if (W < 1 || nrows < 1 || int64_t(W) * nrows >= (int64_t(1) << 40)) return set_error(RT_EINVAL, "rt_nw_adapt_criterion: bad size");
  if (min_spp < 0 || max_spp < 2 || min_spp > max_spp || max_spp > RT_NW_ADAPT_MAX_SPP)
    return set_error(RT_EINVAL, "rt_nw_adapt_criterion: need 0 <= min_spp <= max_spp, 2 <= max_spp <= 2^20");
  if (!(threshold >= 0.0) || !(floor > 0.0) || !std::isfinite(floor) || dilate < 0)
    return set_error(RT_EINVAL, "rt_nw_adapt_criterion: need threshold >= 0, floor > 0 and dilate >= 0");
  const size_t npix = size_t(W) * size_t(nrows);
  const int32_t least = std::max(min_spp, 2);
  dilate = std::min(dilate, std::max(W, nrows));  // (a wider window covers the strip already)
  std::vector<uint8_t> raw(npix);
  for (size_t p = 0; p < npix; ++p) {
    const int32_t k = n[p];
    if (k < 0) return set_error(RT_EINVAL, "rt_nw_adapt_criterion: negative sample count");
    double e = std::numeric_limits<double>::infinity();
    if (k >= 2) {
      const double nn = double(k);
      const double mean = double(sum[3 * p] + sum[3 * p + 1] + sum[3 * p + 2]) * 0x1p-32 / nn;
      const double ex2 = double(m2[p]) * 0x1p-28 / nn;
      const double var = std::max(0.0, ex2 - mean * mean) * nn / (nn - 1.0);
      e = std::sqrt(var / nn) / std::max(mean, floor);
    }
    if (err) err[p] = e;
    // (a threshold of 0 cannot be met, not even by equal samples, whose err is 0)
    raw[p] = k < max_spp && (k < least || e > threshold || threshold == 0.0) ? 1 : 0;
  }
  // dilation by `dilate` pixels (a square window), never onto a pixel at max_spp: along rows, then along columns
  std::vector<uint8_t> rows(raw);
  if (dilate > 0) {
    for (int32_t y = 0; y < nrows; ++y)
      for (int32_t x = 0; x < W; ++x) {
        uint8_t v = 0;
        for (int32_t i = std::max(0, x - dilate); i <= std::min(W - 1, x + dilate) && !v; ++i) v = raw[size_t(y) * W + i];
        rows[size_t(y) * W + x] = v;
      }
  }
  int64_t count = 0;
  for (int32_t y = 0; y < nrows; ++y)
    for (int32_t x = 0; x < W; ++x) {
      uint8_t v = 0;
      for (int32_t j = std::max(0, y - dilate); j <= std::min(nrows - 1, y + dilate) && !v; ++j) v = rows[size_t(j) * W + x];
      v = v && n[size_t(y) * W + x] < max_spp ? 1 : 0;
      active[size_t(y) * W + x] = v;
      count += v;
    }
  if (n_active) *n_active = count;
  return RT_OK;
}

// The variance of each pixel's mean channel sum (the denoiser's guide), from the criterion's moments in its float64
// order: var = max(0, ex2 - mean^2) / (n - 1), which is the criterion's var / n.  Fewer than two samples: +inf.
RTMI_EXPORT int rt_nw_adapt_variance(const int64_t *sum, const uint64_t *m2, const int32_t *n, int32_t W, int32_t nrows, float *var) {
  if (!sum || !m2 || !n || !var) return set_error(RT_EINVAL, "rt_nw_adapt_variance: null argument");
  if (W < 1 || nrows < 1 || int64_t(W) * nrows >= (int64_t(1) << 40)) return set_error(RT_EINVAL, "rt_nw_adapt_variance: bad size");
  const size_t npix = size_t(W) * size_t(nrows);
  for (size_t p = 0; p < npix; ++p)
    if (n[p] < 0) return set_error(RT_EINVAL, "rt_nw_adapt_variance: negative sample count");
  for (size_t p = 0; p < npix; ++p) {
    const int32_t k = n[p];
    double v = std::numeric_limits<double>::infinity();
    if (k >= 2) {
      const double nn = double(k);
      const double mean = double(sum[3 * p] + sum[3 * p + 1] + sum[3 * p + 2]) * 0x1p-32 / nn;
      const double ex2 = double(m2[p]) * 0x1p-28 / nn;
      v = std::max(0.0, ex2 - mean * mean) / (nn - 1.0);
    }
    var[p] = float(v);
  }
  return RT_OK;
}

// The denoiser's parameters (rt_nw_denoise; the filter itself is rtmi_nw_denoise.hip): host only
RTMI_EXPORT int rt_nw_denoise_params_default(rt_nw_denoise_params *p) {
  if (!p) return set_error(RT_EINVAL, "rt_nw_denoise_params_default: null argument");
  *p = rt_nw_denoise_params{5, 4.0f, 128.0f, 1.0f, RT_NW_DENOISE_DEMODULATE};
  return RT_OK;
}

RTMI_EXPORT int rt_nw_denoise_params_check(const rt_nw_denoise_params *p) {
  if (!p) return set_error(RT_EINVAL, "rt_nw_denoise_params_check: null argument");
  if (p->iterations < 1 || p->iterations > 8) return set_error(RT_EINVAL, "rt_nw_denoise: iterations %d outside 1..8", p->iterations);
  for (float s : {p->sigma_l, p->sigma_n, p->sigma_z})
    if (!std::isfinite(s) || !(s > 0.0f)) return set_error(RT_EINVAL, "rt_nw_denoise: every sigma must be finite and > 0");
  if (p->flags & ~uint32_t(RT_NW_DENOISE_DEMODULATE | RT_NW_DENOISE_NO_EDGES))
    return set_error(RT_EINVAL, "rt_nw_denoise: unknown flag bits 0x%x", p->flags);
  return RT_OK;
}

RTMI_EXPORT int rt_nw_accum_info(const char *path, int32_t out8[8], uint64_t out3[3]) {
  if (!path || !out8 || !out3) return set_error(RT_EINVAL, "rt_nw_accum_info: null argument");
  CkptHeader h{};
  if (int rc = ckpt_read(path, h, nullptr)) return rc;
  const int32_t v[8] = {h.W, h.H, h.row0, h.row_step, h.nrows, h.spp_done, h.max_depth, h.zero};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  out3[0] = h.seed;
  out3[1] = h.scene_hash;
  out3[2] = h.camera_hash;
  return RT_OK;
}

RTMI_EXPORT int rt_nw_xorwow_uniforms(uint64_t seed, int32_t n, float *out) {
  if (n < 0 || (n > 0 && !out)) return set_error(RT_EINVAL, "rt_nw_xorwow_uniforms: bad argument");
  Xorwow g(seed);
  for (int i = 0; i < n; ++i) out[i] = g.uniform();
  return RT_OK;
}

// ---------------------------------------------------------------------------
// The reference's scenes (rt_next_week/cuda/main.cu:163-413, create_world
// main.cu:415-490), drawing from curand_init(1984, 0, 0) (main.cu:103-107).
// ---------------------------------------------------------------------------
namespace {

struct Preset {
  rt_nw_scene *s;
  Xorwow g;
  bool rtl;
  int rc = RT_OK;

  int chk(int v) {
    if (v < 0 && rc == RT_OK) rc = v;
    return v;
  }
  // vec3(f(), f(), f()) with the configured argument evaluation order
  template <class F> void vec3_draw(F f, float out[3]) {
    if (rtl) { out[2] = f(); out[1] = f(); out[0] = f(); }
    else { out[0] = f(); out[1] = f(); out[2] = f(); }
  }
  int solid(double r, double g_, double b) { return chk(rt_nw_tex_solid(s, r, g_, b)); }
  int lam(double r, double g_, double b) { return chk(rt_nw_mat_lambertian(s, solid(r, g_, b))); }
  int lam_t(int tex) { return chk(rt_nw_mat_lambertian(s, tex)); }
  int sphere(double x, double y, double z, double r, int m) {
    const double c[3] = {x, y, z};
    return chk(rt_nw_sphere(s, c, r, m));
  }
  void add(int obj) { chk(rt_nw_world_add(s, obj)); }
  int checker() { return chk(rt_nw_tex_checker(s, solid(0.2, 0.3, 0.1), solid(0.9, 0.9, 0.9))); }
  // perlin::perlin perlin.h:8-21: ranvec = random_vec3(-1, 1), then
  // perm_x, perm_y, perm_z by perlin_generate_perm / permute (perlin.h:92-112)
  int noise(double scale) {
    float ranvec[3 * kPerlinN];
    int32_t perm[3 * kPerlinN];
    for (int i = 0; i < kPerlinN; ++i) vec3_draw([&] { return g.range(-1.f, 1.f); }, ranvec + 3 * i);
    for (int a = 0; a < 3; ++a) {
      int32_t *p = perm + a * kPerlinN;
      for (int i = 0; i < kPerlinN; ++i) p[i] = i;
      for (int i = kPerlinN - 1; i > 0; --i) std::swap(p[i], p[g.rint(kPerlinN)]);
    }
    return chk(rt_nw_tex_noise(s, scale, ranvec, perm));
  }
  int box(double x0, double y0, double z0, double x1, double y1, double z1, int m) {
    const double p0[3] = {x0, y0, z0}, p1[3] = {x1, y1, z1};
    return chk(rt_nw_box(s, p0, p1, m));
  }
  int xf(int obj, double angle, double tx, double ty, double tz) {
    const double off[3] = {tx, ty, tz};
    return chk(rt_nw_translate(s, chk(rt_nw_rotate_y(s, obj, angle)), off));
  }

  // random_scene main.cu:163-213
  void random_scene() {
    add(sphere(0, -1000.0, -1, 1000, lam_t(checker())));
    for (int a = -11; a < 11; a++)
      for (int b = -11; b < 11; b++) {
        const float choose_mat = g.uniform();
        float ctr[3];
        if (rtl) { ctr[2] = float(b) + g.uniform(); ctr[0] = float(a) + g.uniform(); }
        else { ctr[0] = float(a) + g.uniform(); ctr[2] = float(b) + g.uniform(); }
        ctr[1] = 0.2f;
        const double c0[3] = {ctr[0], ctr[1], ctr[2]};
        if (choose_mat < 0.8f) {
          const double c1[3] = {ctr[0], ctr[1] + g.uniform() * 0.5f, ctr[2]};
          float alb[3];
          vec3_draw([&] { const float x = g.uniform(); return x * g.uniform(); }, alb);
          add(chk(rt_nw_moving_sphere(s, c0, c1, 0.0, 1.0, 0.2, lam(alb[0], alb[1], alb[2]))));
        } else if (choose_mat < 0.95f) {
          float alb[3], fuzz;
          if (rtl) {
            fuzz = 0.5f * g.uniform();
            vec3_draw([&] { return 0.5f * (1.0f + g.uniform()); }, alb);
          } else {
            vec3_draw([&] { return 0.5f * (1.0f + g.uniform()); }, alb);
            fuzz = 0.5f * g.uniform();
          }
          add(chk(rt_nw_sphere(s, c0, 0.2, chk(rt_nw_mat_metal(s, solid(alb[0], alb[1], alb[2]), fuzz)))));
        } else {
          add(chk(rt_nw_sphere(s, c0, 0.2, chk(rt_nw_mat_dielectric(s, 1.5)))));
        }
      }
    add(sphere(0, 1, 0, 1.0, chk(rt_nw_mat_dielectric(s, 1.5))));
    add(sphere(-4, 1, 0, 1.0, lam(0.4, 0.2, 0.1)));
    add(sphere(4, 1, 0, 1.0, chk(rt_nw_mat_metal(s, solid(0.7, 0.6, 0.5), 0.0))));
  }
  // two_spheres main.cu:215-226
  void two_spheres() {
    const int m = lam_t(checker());
    add(sphere(0, -10, 0, 10, m));
    add(sphere(0, 10, 0, 10, m));
  }
  // two_perlin_spheres main.cu:228-238
  void two_perlin_spheres() {
    const int m = lam_t(noise(4));
    add(sphere(0, -1000, 0, 1000, m));
    add(sphere(0, 2, 0, 2, m));
  }
  // earth main.cu:240-248
  void earth(const uint8_t *img, int w, int h) {
    add(sphere(0, 0, 0, 2, lam_t(chk(rt_nw_tex_image(s, img, w, h)))));
  }
  // simple_light main.cu:250-266
  void simple_light() {
    const int m = lam_t(noise(4));
    add(sphere(0, -1000, 0, 1000, m));
    add(sphere(0, 2, 0, 2, m));
    add(chk(rt_nw_rect(s, RT_NW_XY, 3, 5, 1, 2, -2, chk(rt_nw_mat_diffuse_light(s, solid(4, 4, 4))))));
    add(sphere(0, 6, 0, 1.5, chk(rt_nw_mat_diffuse_light(s, solid(6, 4, 4)))));
  }
  // cornell_box main.cu:268-299, cornell_smoke main.cu:301-329
  void cornell(bool smoke) {
    const int red = lam(.65, .05, .05), white = lam(.73, .73, .73), green = lam(.12, .45, .15);
    const int light = chk(rt_nw_mat_diffuse_light(s, solid(15, 15, 15)));
    add(chk(rt_nw_rect(s, RT_NW_YZ, 0, 555, 0, 555, 555, green)));
    add(chk(rt_nw_rect(s, RT_NW_YZ, 0, 555, 0, 555, 0, red)));
    add(chk(rt_nw_rect(s, RT_NW_XZ, 213, 343, 227, 332, 554, light)));
    add(chk(rt_nw_rect(s, RT_NW_XZ, 0, 555, 0, 555, 0, white)));
    add(chk(rt_nw_rect(s, RT_NW_XZ, 0, 555, 0, 555, 555, white)));
    add(chk(rt_nw_rect(s, RT_NW_XY, 0, 555, 0, 555, 555, white)));
    int box1 = xf(box(0, 0, 0, 165, 330, 165, white), 15, 265, 0, 295);
    int box2 = xf(box(0, 0, 0, 165, 165, 165, white), -18, 130, 0, 65);
    if (smoke) {
      box1 = chk(rt_nw_constant_medium(s, box1, 0.01, solid(0, 0, 0)));
      box2 = chk(rt_nw_constant_medium(s, box2, 0.01, solid(1, 1, 1)));
    }
    add(box1);
    add(box2);
  }
  // rt_next_week_final_scene main.cu:331-413
  void final_scene(const uint8_t *img, int w, int h) {
    const int ground = lam(0.48, 0.83, 0.53);
    for (int i = 0; i < 20; i++)
      for (int j = 0; j < 20; j++) {
        const float wd = 100.0f;
        const float x0 = -1000.0f + float(i) * wd, z0 = -1000.0f + float(j) * wd, y0 = 0.0f;
        const float x1 = x0 + wd, y1 = g.range(1.f, 101.f), z1 = z0 + wd;
        add(box(x0, y0, z0, x1, y1, z1, ground));
      }
    add(chk(rt_nw_rect(s, RT_NW_XZ, 123, 423, 147, 412, 554, chk(rt_nw_mat_diffuse_light(s, solid(7, 7, 7))))));
    {
      const double c1[3] = {400, 400, 200}, c2[3] = {430, 400, 200};
      add(chk(rt_nw_moving_sphere(s, c1, c2, 0, 1, 50, lam(0.7, 0.3, 0.1))));
    }
    add(sphere(260, 150, 45, 50, chk(rt_nw_mat_dielectric(s, 1.5))));
    add(sphere(0, 150, 145, 50, chk(rt_nw_mat_metal(s, solid(0.8, 0.8, 0.9), 1.0))));
    const int sd2 = sphere(360, 150, 145, 70, chk(rt_nw_mat_dielectric(s, 1.5)));
    add(sd2);
    add(chk(rt_nw_constant_medium(s, sd2, 0.2, solid(0.2, 0.4, 0.9))));
    const int fog = sphere(0, 0, 0, 5000, chk(rt_nw_mat_dielectric(s, 1.5)));
    const int fog_medium = chk(rt_nw_constant_medium(s, fog, 0.0001, solid(1, 1, 1)));
    // The fog's box (r = 5000) sorts first on every axis, so the reference's
    // bvh_node puts it alone in a span-1 leaf (left = right, bvh.h:147-151)
    // that its traversal evaluates twice per ray (bvh.h:90-97): two
    // scattering-distance draws, the last hit wins.
    chk(rt_nw_medium_samples(s, fog_medium, 2));
    add(fog_medium);
    add(sphere(400, 200, 400, 100, lam_t(chk(rt_nw_tex_image(s, img, w, h)))));
    add(sphere(220, 280, 300, 80, lam_t(noise(0.1))));
    const int white = lam(.73, .73, .73);
    std::vector<int32_t> cluster(1000);
    for (int j = 0; j < 1000; j++) {
      float c[3];
      vec3_draw([&] { return g.range(0.f, 165.f); }, c);
      cluster[j] = sphere(c[0], c[1], c[2], 10, white);
    }
    add(xf(chk(rt_nw_group(s, cluster.data(), 1000)), 15, -100, 270, 395));
  }
};

}  // namespace

RTMI_EXPORT int rt_nw_scene_preset(rt_nw_scene *s, int32_t which, const uint8_t *image, int32_t w, int32_t h,
                                   double aspect, uint32_t flags, rt_nw_camera *cam) {
  if (!s || !cam || !(aspect > 0)) return set_error(RT_EINVAL, "rt_nw_scene_preset: bad argument");
  if (which < 1 || which > 8) return set_error(RT_EINVAL, "rt_nw_scene_preset: scene %d not in 1..8", which);
  if (image && (w <= 0 || h <= 0)) return set_error(RT_EINVAL, "rt_nw_scene_preset: bad image size");
  Preset p{s, Xorwow(1984), (flags & RT_NW_ARGS_RTL) != 0};
  // create_world defaults main.cu:421-427, then the per-scene switch
  double lookfrom[3] = {13, 2, 3}, lookat[3] = {0, 0, 0};
  double aperture = 0.0, vfov = 40.0;
  const double sky[3] = {0.70, 0.80, 1.00};
  const double *bg = sky;
  const double black[3] = {0, 0, 0};
  switch (which) {
    case 1: p.random_scene(); vfov = 20.0; aperture = 0.05; break;
    case 2: p.two_spheres(); vfov = 20.0; break;
    case 3: p.two_perlin_spheres(); vfov = 20.0; break;
    case 4: p.earth(image, w, h); break;
    case 5:
      bg = black;
      p.simple_light();
      lookfrom[0] = 26; lookfrom[1] = 3; lookfrom[2] = 6;
      lookat[0] = 0; lookat[1] = 2; lookat[2] = 0;
      vfov = 20.0;
      break;
    case 6: case 7:
      bg = black;
      p.cornell(which == 7);
      lookfrom[0] = 278; lookfrom[1] = 278; lookfrom[2] = -800;
      lookat[0] = 278; lookat[1] = 278; lookat[2] = 0;
      break;
    case 8:
      bg = black;
      p.final_scene(image, w, h);
      lookfrom[0] = 478; lookfrom[1] = 278; lookfrom[2] = -600;
      lookat[0] = 278; lookat[1] = 278; lookat[2] = 0;
      break;
  }
  if (p.rc) return p.rc;
  rt_nw_set_background(s, bg[0], bg[1], bg[2]);
  const double vup[3] = {0, 1, 0};
  const double dx = lookfrom[0] - lookat[0], dy = lookfrom[1] - lookat[1], dz = lookfrom[2] - lookat[2];
  const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);  // main.cu:486
  return rt_nw_camera_init(cam, lookfrom, lookat, vup, vfov, aspect, aperture, dist, 0.0, 1.0);
}
