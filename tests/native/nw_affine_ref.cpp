// nw_affine_ref.cpp — the checker of the Next-Week renderer's affine
// placements (tests/test_nw_affine.py, tests/test_nw_affine_gpu.py): a plain
// C++ restatement of the closest hit and the hit record of a triangle under
// an affine placement of a shared mesh, written from the specification
// comment beside to_local_affine in csrc/rtmi_nw_path.h, on top of the
// attribute checker (nw_smooth_ref.cpp, included: the triangle test, the
// local record with its side rule).  It knows nothing of boxes or walks: the
// closest hit is brute force over every triangle of every placement.
//
// The meshes come as a flattened scene of their own (rt_nw_flat of the meshes
// added unplaced: local triangles, materials, attribute records); a placement
// is 24 words:
//   float m[9]      float(A^-1), row-major
//   float o0[3]     float(b); of a moving placement: at offset0
//   float o1[3]     a moving placement's translation at offset1
//   float time0, time1
//   int32 moving, first (the insertion index of its triangle 0), tri0 (its
//         mesh's first object in the local scene), n_tri, pad[3]
//
// Built by csrc/Makefile with g++ -O2 -ffp-contract=off: every float
// operation below is one IEEE operation, fmaf only where written.
#include "nw_smooth_ref.cpp"

namespace {

struct PlaceRef {
  float m[9], o0[3], o1[3], time0, time1;
  int32_t moving, first, tri0, n_tri, pad[3];
};
static_assert(sizeof(PlaceRef) == 96, "PlaceRef layout");

// off(T) of a moving placement: a subtract, a multiply and an add, each rounded
void off_at(const PlaceRef &p, float T, float off[3]) {
  for (int a = 0; a < 3; ++a) off[a] = p.o0[a];
  if (!p.moving) return;
  const float f = (p.time0 == 0.0f && p.time1 == 1.0f) ? T : (T - p.time0) / (p.time1 - p.time0);
  for (int a = 0; a < 3; ++a) {
    const float d = p.o1[a] - p.o0[a];
    const float fd = f * d;
    off[a] = p.o0[a] + fd;
  }
}

V3 rows(const float *m, V3 q) {
  return V3{std::fmaf(m[0], q.x, std::fmaf(m[1], q.y, m[2] * q.z)), std::fmaf(m[3], q.x, std::fmaf(m[4], q.y, m[5] * q.z)),
            std::fmaf(m[6], q.x, std::fmaf(m[7], q.y, m[8] * q.z))};
}
V3 columns(const float *m, V3 n) {
  return V3{std::fmaf(m[0], n.x, std::fmaf(m[3], n.y, m[6] * n.z)), std::fmaf(m[1], n.x, std::fmaf(m[4], n.y, m[7] * n.z)),
            std::fmaf(m[2], n.x, std::fmaf(m[5], n.y, m[8] * n.z))};
}

// the ray into the placement's frame: q = o - off, M q, M d; nothing normalised
void to_local_affine(const PlaceRef &p, float T, V3 &o, V3 &d) {
  float off[3];
  off_at(p, T, off);
  const V3 q = V3{o.x - off[0], o.y - off[1], o.z - off[2]};
  o = rows(p.m, q);
  d = rows(p.m, d);
}

bool places_ok(const Obj *ob, int32_t n_obj, const PlaceRef *pl, int32_t n_place) {
  for (int32_t p = 0; p < n_place; ++p) {
    if (pl[p].tri0 < 0 || pl[p].n_tri < 0 || pl[p].tri0 + pl[p].n_tri > n_obj) return false;
    for (int32_t j = 0; j < pl[p].n_tri; ++j)
      if (ob[pl[p].tri0 + j].kind != kTriangle || ob[pl[p].tri0 + j].inst >= 0) return false;
  }
  return true;
}

}  // namespace

extern "C" {

// n rays (8 floats each: o.xyz, d.xyz, time, unused): the closest hit over the
// placements' triangles, the smallest (t, first(p) + j).  out_id = first(p) + j
// or -1; out_place, out_j: the winner's placement and triangle.
int nwa_closest(const float *obj, int32_t n_obj, const float *places, int32_t n_place, const float *rays, int32_t n,
                int32_t *out_id, float *out_t, int32_t *out_place, int32_t *out_j) {
  const Obj *ob = reinterpret_cast<const Obj *>(obj);
  const PlaceRef *pl = reinterpret_cast<const PlaceRef *>(places);
  if (!places_ok(ob, n_obj, pl, n_place)) return -2;
  auto work = [&](int32_t lo, int32_t hi) {
    for (int32_t i = lo; i < hi; ++i) {
      const float *r = rays + 8 * size_t(i);
      float best = INFINITY;
      int32_t id = -1, bp = -1, bj = -1;
      for (int32_t p = 0; p < n_place; ++p) {
        V3 o = V3{r[0], r[1], r[2]}, d = V3{r[3], r[4], r[5]};
        to_local_affine(pl[p], r[6], o, d);
        for (int32_t j = 0; j < pl[p].n_tri; ++j) {
          V3 v0, v1, v2;
          tri_verts(ob[pl[p].tri0 + j], v0, v1, v2);
          float t;
          bool fb;
          if (!tri_hit(o, d, v0, v1, v2, t, fb)) continue;
          const int32_t k = pl[p].first + j;
          if (id < 0 || t < best || (t == best && k < id)) {
            best = t;
            id = k;
            bp = p;
            bj = j;
          }
        }
      }
      out_id[i] = id;
      out_t[i] = best;
      out_place[i] = bp;
      out_j[i] = bj;
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < nt; ++w) {
    const int32_t lo = int32_t(int64_t(n) * w / nt), hi = int32_t(int64_t(n) * (w + 1) / nt);
    if (w + 1 == nt) work(lo, hi);
    else pool.emplace_back(work, lo, hi);
  }
  for (std::thread &th : pool) th.join();
  return 0;
}

// The record of ray i at t[i] on triangle j[i] of placement place[i] (rays with
// place[i] < 0 are left alone): pnuv = {p.xyz, n.xyz, u, v}, the material, the
// side code of nw_smooth_ref.cpp's tri_rec_attr.
int nwa_records(const float *obj, int32_t n_obj, const float *mat, int32_t n_mat, const float *tex, int32_t n_tex,
                const float *attr, int32_t n_attr, const int32_t *attr_of_obj, const float *places, int32_t n_place,
                const float *rays, int32_t n, const int32_t *place, const int32_t *tri, const float *t, float *out_pnuv,
                int32_t *out_mat, int32_t *out_side) {
  const SceneRef s = scene_of(obj, n_obj, nullptr, 0, mat, n_mat, tex, n_tex, attr, n_attr, attr_of_obj);
  if (int rc = check_scene(s)) return rc;
  const PlaceRef *pl = reinterpret_cast<const PlaceRef *>(places);
  if (!places_ok(s.obj, n_obj, pl, n_place)) return -2;
  for (int32_t i = 0; i < n; ++i) {
    if (place[i] < 0) continue;
    if (place[i] >= n_place || tri[i] < 0 || tri[i] >= pl[place[i]].n_tri) return -2;
    const PlaceRef &p = pl[place[i]];
    const float *r = rays + 8 * size_t(i);
    const V3 ow = V3{r[0], r[1], r[2]}, dw = V3{r[3], r[4], r[5]};
    V3 o = ow, d = dw;
    to_local_affine(p, r[6], o, d);
    const int32_t k = p.tri0 + tri[i];
    const Obj &ob = s.obj[k];
    V3 v0, v1, v2;
    tri_verts(ob, v0, v1, v2);
    const int32_t a = s.attr_of_obj ? s.attr_of_obj[k] : -1;
    V3 pl_local, nl;
    float u, v;
    int32_t sd;
    tri_rec_attr(o, d, v0, v1, v2, t[i], a >= 0 ? s.attr + a : nullptr, needs_uv(s.mat, s.tex, ob.mat), pl_local, nl, u, v, sd);
    const V3 pw = at3(ow, dw, t[i]);  // from the world ray
    const V3 w = columns(p.m, nl);    // the inverse transpose
    const float il = 1.0f / std::sqrt(dot3(w, w));
    float *q = out_pnuv + 8 * size_t(i);
    q[0] = pw.x; q[1] = pw.y; q[2] = pw.z;
    q[3] = w.x * il; q[4] = w.y * il; q[5] = w.z * il;
    q[6] = u; q[7] = v;
    out_mat[i] = ob.mat;
    out_side[i] = sd;
  }
  return 0;
}

}  // extern "C"
