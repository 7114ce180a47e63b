// nw_smooth_ref.cpp — the checker of the Next-Week renderer's triangle
// attributes (tests/test_nw_smooth.py, tests/test_nw_smooth_gpu.py): a plain
// C++ restatement of the hit record of a triangle with an attribute record —
// interpolated normals under the side rule, interpolated texture coordinates —
// written from the specification comment in csrc/rtmi_nw_path.h ("Triangle
// attributes") on top of the triangle checker (nw_mesh_ref.cpp, included: its
// edge functions, records and brute-force closest hit), over a flattened scene
// (rt_nw_flat) plus the attribute arrays of rt_nw_scene_flat_attr.
//
// Built by csrc/Makefile with g++ -O2 -ffp-contract=off: every float
// operation below is one IEEE operation, fmaf only where written.
#include "nw_mesh_ref.cpp"

namespace {

struct Attr {  // rt_nw_scene_flat_attr: 16 floats
  float n[9], uv[6];
  int32_t flags;
};
struct Mat4 {
  int32_t kind, tex;
  float fuzz, ir;
};
struct Tex8 {
  int32_t kind, a, b, pad;
  float rgb[3], scale;
};
enum { kDielectricMat = 2, kCheckerTex = 1, kImageTex = 3 };

// does the material's texture read u, v?  (an image, or a checker of one)
bool needs_uv(const Mat4 *mat, const Tex8 *tex, int32_t m) {
  if (mat[m].kind == kDielectricMat) return false;
  const Tex8 &t = tex[mat[m].tex];
  if (t.kind == kImageTex) return true;
  if (t.kind == kCheckerTex) return tex[t.a].kind == kImageTex || tex[t.b].kind == kImageTex;
  return false;
}

// side: 0 no interpolated normal involved, 1 the record took ns, 2 the side
// rule fell back to ng, 3 ns had no length (!(l2 > 0)): ng
void tri_rec_attr(V3 o, V3 d, V3 v0, V3 v1, V3 v2, float t, const Attr *at, bool need_uv, V3 &p, V3 &n, float &u, float &v,
                  int32_t &side) {
  float bu, bv;
  tri_rec(o, d, v0, v1, v2, t, p, n, bu, bv);  // p, the geometric normal, the barycentric u, v
  side = 0;
  u = 0.0f;
  v = 0.0f;
  if (!at) {
    if (need_uv) { u = bu; v = bv; }
    return;
  }
  const Edges e = edges_of(o, shear_of(d), v0, v1, v2);
  const float b0 = e.U / e.det, b1 = e.V / e.det, b2 = e.W / e.det;
  if (at->flags & 1) {
    const float *n0 = at->n, *n1 = at->n + 3, *n2 = at->n + 6;
    V3 ns = V3{std::fmaf(b2, n2[0], std::fmaf(b1, n1[0], b0 * n0[0])), std::fmaf(b2, n2[1], std::fmaf(b1, n1[1], b0 * n0[1])),
               std::fmaf(b2, n2[2], std::fmaf(b1, n1[2], b0 * n0[2]))};
    const float l2 = dot3(ns, ns);
    if (!(l2 > 0.0f)) {
      side = 3;
    } else {
      const float inv_l = 1.0f / std::sqrt(l2);
      ns = V3{ns.x * inv_l, ns.y * inv_l, ns.z * inv_l};
      const float a = dot3(d, n), b = dot3(d, ns);
      if ((a > 0.0f && b > 0.0f) || (a < 0.0f && b < 0.0f)) {
        n = ns;
        side = 1;
      } else {
        side = 2;
      }
    }
  }
  if (need_uv) {
    if (at->flags & 2) {
      u = std::fmaf(b2, at->uv[4], std::fmaf(b1, at->uv[2], b0 * at->uv[0]));
      v = std::fmaf(b2, at->uv[5], std::fmaf(b1, at->uv[3], b0 * at->uv[1]));
    } else {
      u = b1;
      v = b2;
    }
  }
}

struct SceneRef {
  const Obj *obj;
  int32_t n_obj;
  const Inst *inst;
  int32_t n_inst;
  const Mat4 *mat;
  int32_t n_mat;
  const Tex8 *tex;
  int32_t n_tex;
  const Attr *attr;
  int32_t n_attr;
  const int32_t *attr_of_obj;
};

// 0, or a negative code: -1 a kind the checker does not know, -2 an index out
// of range, -3 a sphere whose texture reads u, v (not restated here)
int check_scene(const SceneRef &s) {
  if (!supported(reinterpret_cast<const float *>(s.obj), s.n_obj, s.n_inst)) return -1;
  for (int32_t k = 0; k < s.n_obj; ++k) {
    const int32_t m = s.obj[k].mat;
    if (m < 0 || m >= s.n_mat) return -2;
    if (s.mat[m].kind != kDielectricMat) {
      const int32_t t = s.mat[m].tex;
      if (t < 0 || t >= s.n_tex) return -2;
      if (s.tex[t].kind == kCheckerTex && (s.tex[t].a < 0 || s.tex[t].a >= s.n_tex || s.tex[t].b < 0 || s.tex[t].b >= s.n_tex)) return -2;
    }
    const int32_t a = s.attr_of_obj ? s.attr_of_obj[k] : -1;
    if (a < -1 || a >= s.n_attr || (a >= 0 && s.obj[k].kind != kTriangle)) return -2;
    if (s.obj[k].kind == kSphere && needs_uv(s.mat, s.tex, m)) return -3;
  }
  return 0;
}

// the record of object k for the world ray (o, d) at t, world space
void record_of(const SceneRef &s, int32_t k, V3 o, V3 d, float t, float *pnuv, int32_t *mat, int32_t *side) {
  const Obj &ob = s.obj[k];
  const Inst *in = ob.inst >= 0 ? s.inst + ob.inst : nullptr;
  if (in) to_local(*in, o, d);
  V3 p, n;
  float u = 0.0f, v = 0.0f;
  int32_t sd = 0;
  if (ob.kind == kSphere) {
    p = at3(o, d, t);
    const float inv_r = 1.0f / ob.g0[3];
    n = V3{inv_r * (p.x - ob.g0[0]), inv_r * (p.y - ob.g0[1]), inv_r * (p.z - ob.g0[2])};
  } else {
    V3 v0, v1, v2;
    tri_verts(ob, v0, v1, v2);
    const int32_t a = s.attr_of_obj ? s.attr_of_obj[k] : -1;
    tri_rec_attr(o, d, v0, v1, v2, t, a >= 0 ? s.attr + a : nullptr, needs_uv(s.mat, s.tex, ob.mat), p, n, u, v, sd);
  }
  if (in && (in->flags & 1)) {
    p = rot_to_world(*in, p);
    n = rot_to_world(*in, n);
  }
  if (in && (in->flags & 2)) p = V3{p.x + in->off[0], p.y + in->off[1], p.z + in->off[2]};
  pnuv[0] = p.x; pnuv[1] = p.y; pnuv[2] = p.z;
  pnuv[3] = n.x; pnuv[4] = n.y; pnuv[5] = n.z;
  pnuv[6] = u; pnuv[7] = v;
  *mat = ob.mat;
  if (side) *side = sd;
}

SceneRef scene_of(const float *obj, int32_t n_obj, const float *inst, int32_t n_inst, const float *mat, int32_t n_mat,
                  const float *tex, int32_t n_tex, const float *attr, int32_t n_attr, const int32_t *attr_of_obj) {
  return SceneRef{reinterpret_cast<const Obj *>(obj),  n_obj, reinterpret_cast<const Inst *>(inst), n_inst,
                  reinterpret_cast<const Mat4 *>(mat), n_mat, reinterpret_cast<const Tex8 *>(tex),  n_tex,
                  reinterpret_cast<const Attr *>(attr), n_attr, attr_of_obj};
}

}  // namespace

extern "C" {

// One record: object k (insertion index) for the world ray o6 = (o.xyz, d.xyz)
// at t -> pnuv = {p.xyz, n.xyz, u, v}, the material, the side code.
int nws_record(const float *obj, int32_t n_obj, const float *inst, int32_t n_inst, const float *mat, int32_t n_mat,
               const float *tex, int32_t n_tex, const float *attr, int32_t n_attr, const int32_t *attr_of_obj, int32_t k,
               const float *o6, float t, float *pnuv, int32_t *out_mat, int32_t *out_side) {
  const SceneRef s = scene_of(obj, n_obj, inst, n_inst, mat, n_mat, tex, n_tex, attr, n_attr, attr_of_obj);
  if (int rc = check_scene(s)) return rc;
  if (k < 0 || k >= n_obj) return -2;
  record_of(s, k, V3{o6[0], o6[1], o6[2]}, V3{o6[3], o6[4], o6[5]}, t, pnuv, out_mat, out_side);
  return 0;
}

// n rays (8 floats each, as rt_nw_debug_records): the brute-force closest hit
// of nwm_closest — the smallest (t, insertion index) — and its record; a miss
// writes index -1 and zeros.
int nws_records(const float *obj, int32_t n_obj, const float *inst, int32_t n_inst, const float *mat, int32_t n_mat,
                const float *tex, int32_t n_tex, const float *attr, int32_t n_attr, const int32_t *attr_of_obj,
                const float *rays, int32_t n, int32_t *out_id, float *out_t, float *out_pnuv, int32_t *out_mat,
                int32_t *out_side) {
  const SceneRef s = scene_of(obj, n_obj, inst, n_inst, mat, n_mat, tex, n_tex, attr, n_attr, attr_of_obj);
  if (int rc = check_scene(s)) return rc;
  if (nwm_closest(obj, n_obj, inst, n_inst, rays, n, out_id, out_t) != 0) return -1;
  for (int32_t i = 0; i < n; ++i) {
    float *q = out_pnuv + 8 * size_t(i);
    if (out_id[i] < 0) {
      out_t[i] = 0.0f;
      out_mat[i] = 0;
      out_side[i] = 0;
      for (int c = 0; c < 8; ++c) q[c] = 0.0f;
      continue;
    }
    const float *r = rays + 8 * size_t(i);
    record_of(s, out_id[i], V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, out_t[i], q, out_mat + i, out_side + i);
  }
  return 0;
}

}  // extern "C"
