// nw_mesh_ref.cpp — the checker of the Next-Week renderer's triangles
// (tests/test_nw_mesh.py, tests/test_nw_mesh_gpu.py): a plain C++ restatement
// of the triangle test and hit record, written from the specification comment
// in csrc/rtmi_nw_path.h ("triangle (kTriangle)") and from DESIGN.md §9 — it
// includes no header of the library — plus a brute-force closest hit over a
// flattened scene (rt_nw_flat) of spheres and triangles with optional
// instances, under the (t, insertion index) winner rule.
//
// Built by csrc/Makefile with g++ -O2 -ffp-contract=off: every float
// operation below is one IEEE operation, fmaf only where written.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct V3 {
  float x, y, z;
};
float get(V3 a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }
V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// the library's dot3: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))
float dot3(V3 a, V3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
// ray::at as the library evaluates it: fma(t, d, o) per component
V3 at3(V3 o, V3 d, float t) { return V3{std::fmaf(t, d.x, o.x), std::fmaf(t, d.y, o.y), std::fmaf(t, d.z, o.z)}; }

struct Shear {
  int kx, ky, kz;
  float Sx, Sy, Sz;
};
Shear shear_of(V3 d) {
  Shear s;
  s.kz = 0;
  if (std::fabs(d.y) > std::fabs(get(d, s.kz))) s.kz = 1;
  if (std::fabs(d.z) > std::fabs(get(d, s.kz))) s.kz = 2;
  s.kx = (s.kz + 1) % 3;
  s.ky = (s.kx + 1) % 3;
  if (get(d, s.kz) < 0.0f) {
    const int tmp = s.kx;
    s.kx = s.ky;
    s.ky = tmp;
  }
  s.Sx = get(d, s.kx) / get(d, s.kz);
  s.Sy = get(d, s.ky) / get(d, s.kz);
  s.Sz = 1.0f / get(d, s.kz);
  return s;
}

struct Edges {
  float U, V, W, det, T;
  bool inside, fallback;
};
Edges edges_of(V3 o, const Shear &s, V3 v0, V3 v1, V3 v2) {
  const V3 A = sub(v0, o), B = sub(v1, o), C = sub(v2, o);
  const float Ax = get(A, s.kx) - s.Sx * get(A, s.kz), Ay = get(A, s.ky) - s.Sy * get(A, s.kz);
  const float Bx = get(B, s.kx) - s.Sx * get(B, s.kz), By = get(B, s.ky) - s.Sy * get(B, s.kz);
  const float Cx = get(C, s.kx) - s.Sx * get(C, s.kz), Cy = get(C, s.ky) - s.Sy * get(C, s.kz);
  Edges e;
  e.U = Cx * By - Cy * Bx;
  e.V = Ax * Cy - Ay * Cx;
  e.W = Bx * Ay - By * Ax;
  e.fallback = e.U == 0.0f || e.V == 0.0f || e.W == 0.0f;
  if (e.fallback) {
    e.U = float(double(Cx) * double(By) - double(Cy) * double(Bx));
    e.V = float(double(Ax) * double(Cy) - double(Ay) * double(Cx));
    e.W = float(double(Bx) * double(Ay) - double(By) * double(Ax));
  }
  const bool any_neg = e.U < 0.0f || e.V < 0.0f || e.W < 0.0f;
  const bool any_pos = e.U > 0.0f || e.V > 0.0f || e.W > 0.0f;
  e.det = (e.U + e.V) + e.W;
  e.inside = !(any_neg && any_pos) && e.det != 0.0f;
  const float Az = s.Sz * get(A, s.kz), Bz = s.Sz * get(B, s.kz), Cz = s.Sz * get(C, s.kz);
  e.T = ((e.U * Az) + (e.V * Bz)) + (e.W * Cz);
  return e;
}

// "never hit": collinear vertices, by the cross product in double
bool collinear(V3 v0, V3 v1, V3 v2) {
  const double e1[3] = {double(v1.x) - double(v0.x), double(v1.y) - double(v0.y), double(v1.z) - double(v0.z)};
  const double e2[3] = {double(v2.x) - double(v0.x), double(v2.y) - double(v0.y), double(v2.z) - double(v0.z)};
  return e1[1] * e2[2] - e1[2] * e2[1] == 0.0 && e1[2] * e2[0] - e1[0] * e2[2] == 0.0 && e1[0] * e2[1] - e1[1] * e2[0] == 0.0;
}

bool tri_hit(V3 o, V3 d, V3 v0, V3 v1, V3 v2, float &t, bool &fallback) {
  fallback = false;
  if (collinear(v0, v1, v2)) return false;
  const Edges e = edges_of(o, shear_of(d), v0, v1, v2);
  fallback = e.fallback;
  if (!e.inside) return false;
  const float tt = e.T / e.det;
  if (!(tt >= 0.001f)) return false;
  t = tt;
  return true;
}

void tri_rec(V3 o, V3 d, V3 v0, V3 v1, V3 v2, float t, V3 &p, V3 &n, float &u, float &v) {
  p = at3(o, d, t);
  const V3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  const V3 c = V3{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
  const float inv_len = 1.0f / std::sqrt(dot3(c, c));
  n = V3{c.x * inv_len, c.y * inv_len, c.z * inv_len};
  const Edges e = edges_of(o, shear_of(d), v0, v1, v2);
  u = e.V / e.det;
  v = e.W / e.det;
}

// sphere::hit as the library evaluates it: disc > 0, roots
// strictly inside (0.001, inf)
bool sphere_hit(V3 o, V3 d, V3 c, float r, float &t) {
  const V3 oc = sub(o, c);
  const float a = dot3(d, d), b = dot3(oc, d), cc = dot3(oc, oc) - r * r;
  const float disc = std::fmaf(b, b, -(a * cc));
  if (!(disc > 0.0f)) return false;
  const float sq = std::sqrt(disc);
  float tt = (-b - sq) / a;
  if (tt < INFINITY && tt > 0.001f) { t = tt; return true; }
  tt = (-b + sq) / a;
  if (tt < INFINITY && tt > 0.001f) { t = tt; return true; }
  return false;
}

// flattened records (include/rtmi_nw.h rt_nw_flat): 16 floats per object,
// 8 per instance
struct Obj {
  float g0[4], g1[4], g2[4];
  int32_t kind, mat, inst, aux;
};
struct Inst {
  float c, s, off[3];
  int32_t flags, pad[2];
};
enum { kSphere = 0, kTriangle = 7 };

void tri_verts(const Obj &ob, V3 &v0, V3 &v1, V3 &v2) {
  v0 = V3{ob.g0[0], ob.g0[1], ob.g0[2]};
  v1 = V3{ob.g0[3], ob.g1[0], ob.g1[1]};
  v2 = V3{ob.g1[2], ob.g1[3], ob.g2[0]};
}
// world ray -> the instance's local ray: translate, then rotate_y
void to_local(const Inst &in, V3 &o, V3 &d) {
  if (in.flags & 2) o = V3{o.x - in.off[0], o.y - in.off[1], o.z - in.off[2]};
  if (in.flags & 1) {
    o = V3{std::fmaf(in.c, o.x, -(in.s * o.z)), o.y, std::fmaf(in.s, o.x, in.c * o.z)};
    d = V3{std::fmaf(in.c, d.x, -(in.s * d.z)), d.y, std::fmaf(in.s, d.x, in.c * d.z)};
  }
}
V3 rot_to_world(const Inst &in, V3 v) {
  return V3{std::fmaf(in.c, v.x, in.s * v.z), v.y, std::fmaf(-in.s, v.x, in.c * v.z)};
}

bool obj_hit(const Obj &ob, const Inst *inst, V3 o, V3 d, float &t, bool &fallback) {
  fallback = false;
  if (ob.inst >= 0) to_local(inst[ob.inst], o, d);
  if (ob.kind == kSphere) return sphere_hit(o, d, V3{ob.g0[0], ob.g0[1], ob.g0[2]}, ob.g0[3], t);
  V3 v0, v1, v2;
  tri_verts(ob, v0, v1, v2);
  return tri_hit(o, d, v0, v1, v2, t, fallback);
}

bool supported(const float *obj, int32_t n_obj, int32_t n_inst) {
  const Obj *ob = reinterpret_cast<const Obj *>(obj);
  for (int32_t k = 0; k < n_obj; ++k)
    if ((ob[k].kind != kSphere && ob[k].kind != kTriangle) || ob[k].inst >= n_inst) return false;
  return true;
}

}  // namespace

extern "C" {

// (a) one triangle: v = v0 v1 v2 as nine floats.  Returns 1 and *t on a hit;
// *fallback = 1 when the edge functions took the double evaluation.
int nwm_tri_hit(const float *o, const float *d, const float *v, float *t, int32_t *fallback) {
  bool fb = false;
  float tt = 0.0f;
  const bool h = tri_hit(V3{o[0], o[1], o[2]}, V3{d[0], d[1], d[2]}, V3{v[0], v[1], v[2]}, V3{v[3], v[4], v[5]},
                         V3{v[6], v[7], v[8]}, tt, fb);
  if (h && t) *t = tt;
  if (fallback) *fallback = fb ? 1 : 0;
  return h ? 1 : 0;
}

// n rays (o.xyz d.xyz, 6 floats each) against one list of n_tri triangles
// (nine floats each): the closest hit's triangle (lowest index among equal
// t; -1: none) and t, and the number of (ray, triangle) tests that took the
// double fallback.
int nwm_tri_closest(const float *tris, int32_t n_tri, const float *rays, int32_t n, int32_t *out_id, float *out_t,
                    int64_t *fallbacks) {
  int64_t nfb = 0;
  for (int32_t i = 0; i < n; ++i) {
    const float *r = rays + 6 * size_t(i);
    const V3 o = V3{r[0], r[1], r[2]}, d = V3{r[3], r[4], r[5]};
    float best = INFINITY;
    int32_t id = -1;
    for (int32_t k = 0; k < n_tri; ++k) {
      const float *v = tris + 9 * size_t(k);
      float t;
      bool fb;
      const bool h = tri_hit(o, d, V3{v[0], v[1], v[2]}, V3{v[3], v[4], v[5]}, V3{v[6], v[7], v[8]}, t, fb);
      nfb += fb ? 1 : 0;
      if (h && (id < 0 || t < best)) {
        best = t;
        id = k;
      }
    }
    out_id[i] = id;
    out_t[i] = best;
  }
  if (fallbacks) *fallbacks = nfb;
  return 0;
}

// (c) brute-force closest hit over a flattened scene of spheres and triangles:
// rays are 8 floats each (o.xyz, d.xyz, time, unused — as rt_nw_debug_hits).
// The winner is the smallest (t, insertion index).  -1: a kind this checker
// does not know.
int nwm_closest(const float *obj, int32_t n_obj, const float *inst, int32_t n_inst, const float *rays, int32_t n,
                int32_t *out_id, float *out_t) {
  if (!supported(obj, n_obj, n_inst)) return -1;
  const Obj *ob = reinterpret_cast<const Obj *>(obj);
  const Inst *in = reinterpret_cast<const Inst *>(inst);
  auto work = [&](int32_t lo, int32_t hi) {
    for (int32_t i = lo; i < hi; ++i) {
      const float *r = rays + 8 * size_t(i);
      const V3 o = V3{r[0], r[1], r[2]}, d = V3{r[3], r[4], r[5]};
      float best = INFINITY;
      int32_t id = -1;
      for (int32_t k = 0; k < n_obj; ++k) {
        float t;
        bool fb;
        // insertion order: an equal t keeps the earlier object
        if (obj_hit(ob[k], in, o, d, t, fb) && (id < 0 || t < best)) {
          best = t;
          id = k;
        }
      }
      out_id[i] = id;
      out_t[i] = best;
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
  if (int64_t(n) * n_obj < (int64_t(1) << 22)) nt = 1;
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < nt; ++w) {
    const int32_t lo = int32_t(int64_t(n) * w / nt), hi = int32_t(int64_t(n) * (w + 1) / nt);
    if (w + 1 == nt) work(lo, hi);
    else pool.emplace_back(work, lo, hi);
  }
  for (std::thread &th : pool) th.join();
  return 0;
}

// (b) the hit record of object k for the world ray (o, d) at t: the point and
// the normal in world space (instance applied), and a triangle's u, v (a
// sphere's are left 0: no test here reads them).
int nwm_record(const float *obj, int32_t n_obj, const float *inst, int32_t n_inst, int32_t k, const float *o6, float t,
               float *p3, float *n3, float *uv2) {
  if (!supported(obj, n_obj, n_inst) || k < 0 || k >= n_obj) return -1;
  const Obj &ob = reinterpret_cast<const Obj *>(obj)[k];
  const Inst *in = ob.inst >= 0 ? reinterpret_cast<const Inst *>(inst) + ob.inst : nullptr;
  V3 o = V3{o6[0], o6[1], o6[2]}, d = V3{o6[3], o6[4], o6[5]};
  if (in) to_local(*in, o, d);
  V3 p, n;
  float u = 0.0f, v = 0.0f;
  if (ob.kind == kSphere) {
    p = at3(o, d, t);
    const float inv_r = 1.0f / ob.g0[3];
    n = V3{inv_r * (p.x - ob.g0[0]), inv_r * (p.y - ob.g0[1]), inv_r * (p.z - ob.g0[2])};
  } else {
    V3 v0, v1, v2;
    tri_verts(ob, v0, v1, v2);
    tri_rec(o, d, v0, v1, v2, t, p, n, u, v);
  }
  if (in && (in->flags & 1)) {
    p = rot_to_world(*in, p);
    n = rot_to_world(*in, n);
  }
  if (in && (in->flags & 2)) p = V3{p.x + in->off[0], p.y + in->off[1], p.z + in->off[2]};
  p3[0] = p.x; p3[1] = p.y; p3[2] = p.z;
  n3[0] = n.x; n3[1] = n.y; n3[2] = n.z;
  uv2[0] = u; uv2[1] = v;
  return 0;
}

}  // extern "C"
