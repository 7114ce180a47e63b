/* oracle/rt_nw_oracle.inc — TEST INFRASTRUCTURE ONLY (included at the end of
 * rt_oracle.c; uses its xoroshiro stream and fast-mode helpers).
 *
 * CPU restatement of the Next-Week path (SURVEY §8(f) rank 4): the
 * reference's rt_next_week/cuda/ hittables (sphere.h, moving_sphere.h,
 * aarect.h, box.h, hittable.h translate/rotate_y, constant_medium.h),
 * textures (texture.h, perlin.h), materials (material.h) and emission-aware
 * integration (get_color, main.cu:47-101), in float with the explicit fmaf
 * policy of DESIGN.md §9.  It reads the FLATTENED scene (rt_nw_scene_flat,
 * insertion order) and finds closest hits by brute force over every object —
 * no BVH — so the GPU's BVH, leaf order and traversal are checked against
 * the plain list.  Triangles (kind 7) and their attribute records are written
 * from the two specification comments of csrc/rtmi_nw_path.h alone: a third
 * restatement beside the kernels and tests/native/nw_*_ref.cpp.  An object
 * kind this file does not know is refused by every entry point.  Parity
 * with the CUDA reference itself is statistical only (tests/test_nw_gpu.py):
 * the reference cannot run here.
 */

/* or_nw_scene and the entry points' prototypes: rt_oracle.h */

enum { NW_SPHERE = 0, NW_MOVING = 1, NW_XY = 2, NW_XZ = 3, NW_YZ = 4, NW_BOX = 5, NW_MEDIUM = 6, NW_TRIANGLE = 7,
       NW_KINDS = 8 };
enum { NWM_LAMB = 0, NWM_METAL = 1, NWM_DIEL = 2, NWM_LIGHT = 3, NWM_ISO = 4 };
enum { NWT_SOLID = 0, NWT_CHECKER = 1, NWT_NOISE = 2, NWT_IMAGE = 3 };

static inline int32_t nw_ibits(float f) { int32_t i; memcpy(&i, &f, 4); return i; }
static inline float nw_fbits(int32_t i) { float f; memcpy(&f, &i, 4); return f; }

typedef fast_V NV;
static inline NV nv(float x, float y, float z) { return fast_mk(x, y, z); }
static inline float ndot(NV a, NV b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static inline NV nat(NV o, NV d, float t) { return nv(fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z)); }

/* ---- transcendentals: sin by rint quadrant + 3-part pi/2, Cephes polys ---- */
static float nw_sin(float x) {
  const float kf = rintf(x * 0.636619747f);
  float r = fmaf(-kf, 1.57079637f, x);
  r = fmaf(-kf, -4.37113883e-8f, r);
  r = fmaf(-kf, -1.77635684e-15f, r);
  const int k = (int)kf & 3;
  const float r2 = r * r;
  float p = fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
  p = fmaf(r2, p, -1.6666654611e-1f);
  const float sn = fmaf(r * r2, p, r);
  float q = fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
  q = fmaf(r2, q, 4.166664568298827e-2f);
  const float cs = fmaf(r2 * r2, q, fmaf(-0.5f, r2, 1.0f));
  return k == 0 ? sn : k == 1 ? cs : k == 2 ? -sn : -cs;
}
/* log: x = m 2^e, m in [sqrt(1/2), sqrt(2)), Cephes logf polynomial */
static float nw_log(float x) {
  const int32_t bits = nw_ibits(x);
  int e = ((bits >> 23) & 255) - 126;
  float m = nw_fbits((bits & 0x7fffff) | 0x3f000000);
  if (m < 0.707106781f) {
    e -= 1;
    m = m + m;
  }
  m = m - 1.0f;
  const float z = m * m;
  float y = fmaf(7.0376836292e-2f, m, -1.1514610310e-1f);
  y = fmaf(y, m, 1.1676998740e-1f);
  y = fmaf(y, m, -1.2420140846e-1f);
  y = fmaf(y, m, 1.4249322787e-1f);
  y = fmaf(y, m, -1.6668057665e-1f);
  y = fmaf(y, m, 2.0000714765e-1f);
  y = fmaf(y, m, -2.4999993993e-1f);
  y = fmaf(y, m, 3.3333331174e-1f);
  y = (y * m) * z;
  const float fe = (float)e;
  y = fmaf(fe, -2.12194440e-4f, y);
  y = fmaf(-0.5f, z, y);
  return fmaf(fe, 0.693359375f, m + y);
}
static float nw_atan(float x) {
  const int neg = x < 0.0f;
  float a = neg ? -x : x, y0 = 0.0f;
  if (a > 2.414213562373095f) {
    y0 = 1.57079637f;
    a = -1.0f / a;
  } else if (a > 0.4142135623730950f) {
    y0 = 0.785398185f;
    a = (a - 1.0f) / (a + 1.0f);
  }
  const float z = a * a;
  float p = fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
  p = fmaf(p, z, 1.99777106478e-1f);
  p = fmaf(p, z, -3.33329491539e-1f);
  const float r = fmaf(p * z, a, a) + y0;
  return neg ? -r : r;
}
static float nw_atan2(float y, float x) {
  if (x == 0.0f) return y > 0.0f ? 1.57079637f : y < 0.0f ? -1.57079637f : 0.0f;
  const float a = nw_atan(y / x);
  if (x > 0.0f) return a;
  return y >= 0.0f ? a + 3.14159274f : a - 3.14159274f;
}
static float nw_acos(float x) {
  x = fminf(fmaxf(x, -1.0f), 1.0f);
  return nw_atan2(sqrtf((1.0f - x) * (1.0f + x)), x);
}

/* ---- object accessors ---------------------------------------------------- */
typedef struct nw_obj {
  float g0[4], g1[4], g2[4];
  int32_t kind, mat, inst, aux;
} nw_obj;
static nw_obj nw_load(const or_nw_scene *s, int32_t k) {
  nw_obj o;
  memcpy(&o, s->obj + 16 * (size_t)k, sizeof o);
  return o;
}
typedef struct nw_inst {
  float c, s, off[3];
  int32_t flags;
} nw_inst;
static nw_inst nw_inst_load(const or_nw_scene *s, int32_t i) {
  const float *p = s->inst + 8 * (size_t)i;
  nw_inst r;
  r.c = p[0]; r.s = p[1]; r.off[0] = p[2]; r.off[1] = p[3]; r.off[2] = p[4];
  r.flags = nw_ibits(p[5]);
  return r;
}
/* translate::hit hittable.h:66-69 then rotate_y::hit hittable.h:147-156 */
static void nw_local(const nw_inst *in, NV *o, NV *d) {
  if (in->flags & 2) *o = nv(o->x - in->off[0], o->y - in->off[1], o->z - in->off[2]);
  if (in->flags & 1) {
    const NV a = *o, b = *d;
    *o = nv(fmaf(in->c, a.x, -(in->s * a.z)), a.y, fmaf(in->s, a.x, in->c * a.z));
    *d = nv(fmaf(in->c, b.x, -(in->s * b.z)), b.y, fmaf(in->s, b.x, in->c * b.z));
  }
}
static NV nw_rot_world(const nw_inst *in, NV v) {
  return nv(fmaf(in->c, v.x, in->s * v.z), v.y, fmaf(-in->s, v.x, in->c * v.z));
}

/* ---- hittables (local frame) --------------------------------------------- */
/* sphere.h:42-77 */
static int nw_hit_sphere(NV o, NV d, NV c, float r, float tmin, float tmax, float *t) {
  const NV oc = nv(o.x - c.x, o.y - c.y, o.z - c.z);
  const float a = ndot(d, d), b = ndot(oc, d), cc = ndot(oc, oc) - r * r;
  const float disc = fmaf(b, b, -(a * cc));
  if (disc > 0.0f) {
    const float sq = sqrtf(disc);
    float tt = (-b - sq) / a;
    if (tt < tmax && tt > tmin) { *t = tt; return 1; }
    tt = (-b + sq) / a;
    if (tt < tmax && tt > tmin) { *t = tt; return 1; }
  }
  return 0;
}
/* moving_sphere.h:44-46 */
static NV nw_center(const nw_obj *ob, float time) {
  const float f = (time - ob->g1[3]) / (ob->g2[0] - ob->g1[3]);
  return nv(fmaf(f, ob->g1[0] - ob->g0[0], ob->g0[0]), fmaf(f, ob->g1[1] - ob->g0[1], ob->g0[1]),
            fmaf(f, ob->g1[2] - ob->g0[2], ob->g0[2]));
}
/* moving_sphere.h:48-77 */
static int nw_hit_moving(NV o, NV d, NV c, float r, float tmin, float tmax, float *t) {
  const NV oc = nv(o.x - c.x, o.y - c.y, o.z - c.z);
  const float a = ndot(d, d), hb = ndot(oc, d), cc = ndot(oc, oc) - r * r;
  const float disc = fmaf(hb, hb, -(a * cc));
  if (disc < 0.0f) return 0;
  const float sq = sqrtf(disc);
  float root = (-hb - sq) / a;
  if (root < tmin || tmax < root) {
    root = (-hb + sq) / a;
    if (root < tmin || tmax < root) return 0;
  }
  *t = root;
  return 1;
}
static float nw_comp(NV v, int ax) { return ax == 0 ? v.x : ax == 1 ? v.y : v.z; }
/* aarect.h xy_rect/xz_rect/yz_rect ::hit; plane axis ka, in-plane axes aa, ba */
static int nw_hit_rect(int ka, int aa, int ba, NV o, NV d, float a0, float a1, float b0, float b1, float k,
                       float tmin, float tmax, float *t) {
  const float tt = (k - nw_comp(o, ka)) / nw_comp(d, ka);
  if (tt < tmin || tt > tmax) return 0;
  const float x = fmaf(tt, nw_comp(d, aa), nw_comp(o, aa));
  const float y = fmaf(tt, nw_comp(d, ba), nw_comp(o, ba));
  if (x < a0 || x > a1 || y < b0 || y > b1) return 0;
  *t = tt;
  return 1;
}
/* box.h: hittable_list over the six sides in constructor order (box.h:37-48) */
static int nw_hit_box(NV o, NV d, const float p0[4], const float p1[4], float tmin, float tmax, float *t) {
  int face = -1;
  float closest = tmax, tt;
  if (nw_hit_rect(2, 0, 1, o, d, p0[0], p1[0], p0[1], p1[1], p1[2], tmin, closest, &tt)) { closest = tt; face = 0; }
  if (nw_hit_rect(2, 0, 1, o, d, p0[0], p1[0], p0[1], p1[1], p0[2], tmin, closest, &tt)) { closest = tt; face = 1; }
  if (nw_hit_rect(1, 0, 2, o, d, p0[0], p1[0], p0[2], p1[2], p1[1], tmin, closest, &tt)) { closest = tt; face = 2; }
  if (nw_hit_rect(1, 0, 2, o, d, p0[0], p1[0], p0[2], p1[2], p0[1], tmin, closest, &tt)) { closest = tt; face = 3; }
  if (nw_hit_rect(0, 1, 2, o, d, p0[1], p1[1], p0[2], p1[2], p1[0], tmin, closest, &tt)) { closest = tt; face = 4; }
  if (nw_hit_rect(0, 1, 2, o, d, p0[1], p1[1], p0[2], p1[2], p0[0], tmin, closest, &tt)) { closest = tt; face = 5; }
  *t = closest;
  return face;
}
/* The rectangles and boxes of nw_hit_object (objects; media boundaries keep
 * the division forms): the plane parameter as (k - o_k) * inv_k with inv =
 * 1/d per axis of the (local) ray — the device's hit_rect_inv / hit_box_inv. */
static int nw_hit_rect_inv(int ka, int aa, int ba, NV o, NV d, NV inv, float a0, float a1, float b0, float b1, float k,
                           float tmin, float tmax, float *t) {
  const float tt = (k - nw_comp(o, ka)) * nw_comp(inv, ka);
  if (tt < tmin || tt > tmax) return 0;
  const float x = fmaf(tt, nw_comp(d, aa), nw_comp(o, aa));
  const float y = fmaf(tt, nw_comp(d, ba), nw_comp(o, ba));
  if (x < a0 || x > a1 || y < b0 || y > b1) return 0;
  *t = tt;
  return 1;
}
static int nw_hit_box_inv(NV o, NV d, NV inv, const float p0[4], const float p1[4], float tmin, float tmax, float *t) {
  int face = -1;
  float closest = tmax, tt;
  if (nw_hit_rect_inv(2, 0, 1, o, d, inv, p0[0], p1[0], p0[1], p1[1], p1[2], tmin, closest, &tt)) { closest = tt; face = 0; }
  if (nw_hit_rect_inv(2, 0, 1, o, d, inv, p0[0], p1[0], p0[1], p1[1], p0[2], tmin, closest, &tt)) { closest = tt; face = 1; }
  if (nw_hit_rect_inv(1, 0, 2, o, d, inv, p0[0], p1[0], p0[2], p1[2], p1[1], tmin, closest, &tt)) { closest = tt; face = 2; }
  if (nw_hit_rect_inv(1, 0, 2, o, d, inv, p0[0], p1[0], p0[2], p1[2], p0[1], tmin, closest, &tt)) { closest = tt; face = 3; }
  if (nw_hit_rect_inv(0, 1, 2, o, d, inv, p0[1], p1[1], p0[2], p1[2], p1[0], tmin, closest, &tt)) { closest = tt; face = 4; }
  if (nw_hit_rect_inv(0, 1, 2, o, d, inv, p0[1], p1[1], p0[2], p1[2], p0[0], tmin, closest, &tt)) { closest = tt; face = 5; }
  *t = closest;
  return face;
}
/* ---- triangle: "triangle (kTriangle) ... THE SPECIFICATION" ----------------
 * Every product, sum and difference below is one float operation (the build
 * keeps -ffp-contract=off); the three divisions of the ray constants and
 * t = T / det are IEEE divisions. */
static void nw_tri_verts(const nw_obj *ob, float v0[3], float v1[3], float v2[3]) {
  v0[0] = ob->g0[0]; v0[1] = ob->g0[1]; v0[2] = ob->g0[2];
  v1[0] = ob->g0[3]; v1[1] = ob->g1[0]; v1[2] = ob->g1[1];
  v2[0] = ob->g1[2]; v2[1] = ob->g1[3]; v2[2] = ob->g2[0];
}
/* "never hit": the double cross product of the float vertices is the zero vector */
static int nw_tri_collinear(const float v0[3], const float v1[3], const float v2[3]) {
  double p[3], q[3];
  for (int a = 0; a < 3; a++) {
    p[a] = (double)v1[a] - (double)v0[a];
    q[a] = (double)v2[a] - (double)v0[a];
  }
  const double cx = p[1] * q[2] - p[2] * q[1];
  const double cy = p[2] * q[0] - p[0] * q[2];
  const double cz = p[0] * q[1] - p[1] * q[0];
  return cx == 0.0 && cy == 0.0 && cz == 0.0;
}
typedef struct nw_tri_fn {
  float U, V, W, det, T;
  int miss; /* the sign rule or det == 0 */
} nw_tri_fn;
static nw_tri_fn nw_tri_edges(NV o, NV d, const float v0[3], const float v1[3], const float v2[3]) {
  const float dv[3] = {d.x, d.y, d.z}, ov[3] = {o.x, o.y, o.z};
  /* ray constants */
  int kz = 0;
  if (fabsf(dv[1]) > fabsf(dv[kz])) kz = 1;
  if (fabsf(dv[2]) > fabsf(dv[kz])) kz = 2;
  int kx = (kz + 1) % 3, ky = (kx + 1) % 3;
  if (dv[kz] < 0.0f) {
    const int sw = kx;
    kx = ky;
    ky = sw;
  }
  const float Sx = dv[kx] / dv[kz], Sy = dv[ky] / dv[kz], Sz = 1.0f / dv[kz];
  /* test */
  float A[3], B[3], C[3];
  for (int a = 0; a < 3; a++) {
    A[a] = v0[a] - ov[a];
    B[a] = v1[a] - ov[a];
    C[a] = v2[a] - ov[a];
  }
  const float Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz];
  const float Bx = B[kx] - Sx * B[kz], By = B[ky] - Sy * B[kz];
  const float Cx = C[kx] - Sx * C[kz], Cy = C[ky] - Sy * C[kz];
  nw_tri_fn f;
  f.U = Cx * By - Cy * Bx;
  f.V = Ax * Cy - Ay * Cx;
  f.W = Bx * Ay - By * Ax;
  if (f.U == 0.0f || f.V == 0.0f || f.W == 0.0f) {
    f.U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
    f.V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
    f.W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
  }
  const int any_neg = f.U < 0.0f || f.V < 0.0f || f.W < 0.0f;
  const int any_pos = f.U > 0.0f || f.V > 0.0f || f.W > 0.0f;
  f.det = (f.U + f.V) + f.W;
  f.miss = (any_neg && any_pos) || f.det == 0.0f;
  const float Az = Sz * A[kz], Bz = Sz * B[kz], Cz = Sz * C[kz];
  f.T = ((f.U * Az) + (f.V * Bz)) + (f.W * Cz);
  return f;
}
static int nw_hit_triangle(const nw_obj *ob, NV o, NV d, float *t) {
  float v0[3], v1[3], v2[3];
  nw_tri_verts(ob, v0, v1, v2);
  if (nw_tri_collinear(v0, v1, v2)) return 0;
  const nw_tri_fn f = nw_tri_edges(o, d, v0, v1, v2);
  if (f.miss) return 0;
  const float tt = f.T / f.det;
  if (!(tt >= 0.001f)) return 0;
  *t = tt;
  return 1;
}

static int nw_hit_boundary(const nw_obj *ob, NV o, NV d, float time, float tmin, float tmax, float *t) {
  const int bk = ob->aux & 255;
  if (bk == NW_SPHERE) return nw_hit_sphere(o, d, nv(ob->g0[0], ob->g0[1], ob->g0[2]), ob->g0[3], tmin, tmax, t);
  if (bk == NW_MOVING) return nw_hit_moving(o, d, nw_center(ob, time), ob->g0[3], tmin, tmax, t);
  return nw_hit_box(o, d, ob->g0, ob->g1, tmin, tmax, t) >= 0;
}
/* per-(segment, medium, sample) uniform in (0, 1] */
static float nw_medium_u(uint64_t seg_key, int32_t id, int smp) {
  const uint64_t h = mix64(seg_key ^ ((uint64_t)((uint32_t)id + 1u) * 0x9E3779B97F4A7C15ULL) ^
                           ((uint64_t)(uint32_t)smp * 0xD1B54A32D192ED03ULL));
  return (float)((uint32_t)(h >> 40) + 1u) * 0x1p-24f;
}
/* constant_medium.h:41-78, `samples` scattering-distance draws (last hit wins) */
static int nw_hit_medium(const nw_obj *ob, int32_t id, NV o, NV d, NV dw, float time, uint64_t seg_key, float *t) {
  float r1, r2;
  if (!nw_hit_boundary(ob, o, d, time, -INFINITY, INFINITY, &r1)) return 0;
  if (!nw_hit_boundary(ob, o, d, time, (float)((double)r1 + 0.00001), INFINITY, &r2)) return 0;
  if (r1 < 0.0f) r1 = 0.0f;
  const float len = sqrtf(ndot(dw, dw));
  const float inside = (r2 - r1) * len;
  int hit = 0;
  for (int smp = 0; smp < (ob->aux >> 8); smp++) {
    const float hd = ob->g2[3] * nw_log(nw_medium_u(seg_key, id, smp));
    if (!(hd > inside)) {
      *t = r1 + hd / len;
      hit = 1;
    }
  }
  return hit;
}
/* a non-medium object (world ray; t_min 0.001, no upper bound) */
static int nw_hit_object(const or_nw_scene *s, const nw_obj *ob, NV ow, NV dw, float time, float *t, int *face) {
  NV o = ow, d = dw;
  if (ob->inst >= 0) {
    const nw_inst in = nw_inst_load(s, ob->inst);
    nw_local(&in, &o, &d);
  }
  const float tmin = 0.001f;
  switch (ob->kind) {
    case NW_SPHERE: return nw_hit_sphere(o, d, nv(ob->g0[0], ob->g0[1], ob->g0[2]), ob->g0[3], tmin, INFINITY, t);
    case NW_MOVING: return nw_hit_moving(o, d, nw_center(ob, time), ob->g0[3], tmin, INFINITY, t);
    case NW_XY: case NW_XZ: case NW_YZ: {
      const NV inv = nv(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
      const int k = ob->kind;
      if (k == NW_XY) return nw_hit_rect_inv(2, 0, 1, o, d, inv, ob->g0[0], ob->g0[1], ob->g0[2], ob->g0[3], ob->g1[0], tmin, INFINITY, t);
      if (k == NW_XZ) return nw_hit_rect_inv(1, 0, 2, o, d, inv, ob->g0[0], ob->g0[1], ob->g0[2], ob->g0[3], ob->g1[0], tmin, INFINITY, t);
      return nw_hit_rect_inv(0, 1, 2, o, d, inv, ob->g0[0], ob->g0[1], ob->g0[2], ob->g0[3], ob->g1[0], tmin, INFINITY, t);
    }
    case NW_BOX: *face = nw_hit_box_inv(o, d, nv(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), ob->g0, ob->g1, tmin, INFINITY, t); return *face >= 0;
    case NW_TRIANGLE: return nw_hit_triangle(ob, o, d, t);
    default: return 0; /* not reached: nw_scene_known refuses the scene */
  }
}
/* 0 when every object's kind is one this file restates (the entry points
 * refuse the scene otherwise: an unknown kind is never rendered as another) */
static int nw_scene_known(const or_nw_scene *s) {
  if (!s || s->n_obj < 0) return -1;
  for (int32_t k = 0; k < s->n_obj; k++) {
    const int32_t kind = nw_load(s, k).kind;
    if (kind < 0 || kind >= NW_KINDS) return -1;
  }
  if (s->n_attr > 0) {
    if (!s->attr || !s->attr_of_obj) return -1;
    for (int32_t k = 0; k < s->n_obj; k++)
      if (s->attr_of_obj[k] < -1 || s->attr_of_obj[k] >= s->n_attr) return -1;
  }
  return 0;
}
/* closest hit of a segment (DESIGN.md §9): media first (each hit marks
 * itself), then every other object by brute force over the list, skipping
 * an object whose twin medium hit; the smallest (t, index) wins. */
static int32_t nw_hit_world(const or_nw_scene *s, const int32_t *med_list, int32_t nmed, NV o, NV d, float time,
                            uint64_t seg_key, float *best_t, int *best_face) {
  int32_t best = -1;
  *best_t = INFINITY;
  *best_face = -1;
  unsigned char med_hit[64] = {0};
  for (int32_t m = 0; m < nmed; m++) {
    const int32_t k = med_list[m];
    const nw_obj ob = nw_load(s, k);
    NV lo = o, ld = d;
    if (ob.inst >= 0) {
      const nw_inst in = nw_inst_load(s, ob.inst);
      nw_local(&in, &lo, &ld);
    }
    float t;
    if (nw_hit_medium(&ob, k, lo, ld, d, time, seg_key, &t) && !(t < 0.001f)) {
      med_hit[m] = 1;
      if (t < *best_t || (t == *best_t && k < best)) {
        *best_t = t;
        best = k;
      }
    }
  }
  for (int32_t k = 0; k < s->n_obj; k++) {
    const nw_obj ob = nw_load(s, k);
    if (ob.kind == NW_MEDIUM) continue;
    if (ob.aux > 0) { /* twin: the medium at insertion index aux-1 */
      int32_t m = 0;
      while (m < nmed && med_list[m] != ob.aux - 1) m++;
      if (m < nmed && med_hit[m]) continue;
    }
    float t;
    int face = -1;
    if (nw_hit_object(s, &ob, o, d, time, &t, &face) && (t < *best_t || (t == *best_t && k < best))) {
      *best_t = t;
      best = k;
      *best_face = face;
    }
  }
  return best;
}

/* ---- textures ------------------------------------------------------------ */
typedef struct nw_tex {
  int32_t kind, a, b;
  float rgb[3], scale;
} nw_tex;
static nw_tex nw_tex_load(const or_nw_scene *s, int32_t i) {
  const float *p = s->tex + 8 * (size_t)i;
  nw_tex t;
  t.kind = nw_ibits(p[0]); t.a = nw_ibits(p[1]); t.b = nw_ibits(p[2]);
  t.rgb[0] = p[4]; t.rgb[1] = p[5]; t.rgb[2] = p[6]; t.scale = p[7];
  return t;
}
/* perlin.h:30-63, 114-127 */
static float nw_noise(const or_nw_scene *s, int32_t pid, NV p) {
  const float *rv = s->perlin_vec + (size_t)pid * 256 * 4;
  const int32_t *px = s->perlin_perm + (size_t)pid * 768, *py = px + 256, *pz = py + 256;
  const float fx = floorf(p.x), fy = floorf(p.y), fz = floorf(p.z);
  float u = p.x - fx, v = p.y - fy, w = p.z - fz;
  u = (u * u) * fmaf(-2.0f, u, 3.0f);
  v = (v * v) * fmaf(-2.0f, v, 3.0f);
  w = (w * w) * fmaf(-2.0f, w, 3.0f);
  const int i = (int)fx, j = (int)fy, k = (int)fz;
  float accum = 0.0f;
  for (int di = 0; di < 2; di++)
    for (int dj = 0; dj < 2; dj++)
      for (int dk = 0; dk < 2; dk++) {
        const float *c = rv + 4 * (px[(i + di) & 255] ^ py[(j + dj) & 255] ^ pz[(k + dk) & 255]);
        const float wi = di ? u : 1.0f - u, wj = dj ? v : 1.0f - v, wk = dk ? w : 1.0f - w;
        const float dd = ndot(nv(c[0], c[1], c[2]), nv(u - (float)di, v - (float)dj, w - (float)dk));
        accum = fmaf((wi * wj) * wk, dd, accum);
      }
  return accum;
}
/* perlin.h:65-78 */
static float nw_turb(const or_nw_scene *s, int32_t pid, NV p) {
  float accum = 0.0f, weight = 1.0f;
  for (int i = 0; i < 7; i++) {
    accum = fmaf(weight, nw_noise(s, pid, p), accum);
    weight *= 0.5f;
    p = nv(p.x * 2.0f, p.y * 2.0f, p.z * 2.0f);
  }
  return fabsf(accum);
}
static NV nw_tex_leaf(const or_nw_scene *s, const nw_tex *tx, float u, float v, NV p) {
  if (tx->kind == NWT_SOLID) return nv(tx->rgb[0], tx->rgb[1], tx->rgb[2]);
  if (tx->kind == NWT_NOISE) { /* texture.h:71-80 */
    const NV sp = nv(tx->scale * p.x, tx->scale * p.y, tx->scale * p.z);
    const float f = 0.5f * (1.0f + nw_sin(fmaf(10.0f, nw_turb(s, tx->a, sp), tx->scale * p.z)));
    return nv(f, f, f);
  }
  /* texture.h:94-120 */
  const int32_t *im = s->image_desc + 4 * (size_t)tx->a;
  const int32_t off = im[0], w = im[1], h = im[2];
  if (w == 0) return nv(0.0f, 1.0f, 1.0f);
  u = fminf(fmaxf(u, 0.0f), 1.0f);
  v = 1.0f - fminf(fmaxf(v, 0.0f), 1.0f);
  int i = (int)(u * (float)w), j = (int)(v * (float)h);
  if (i >= w) i = w - 1;
  if (j >= h) j = h - 1;
  i = (i + w / 2 + w / 3) % w;
  const uint8_t *px = s->image_px + off + (size_t)(j * w + i) * 3;
  const float sc = 1.0f / 255.0f;
  return nv(sc * (float)px[0], sc * (float)px[1], sc * (float)px[2]);
}
/* checker_texture::value texture.h:48-55 */
static NV nw_tex_value(const or_nw_scene *s, int32_t tid, float u, float v, NV p) {
  nw_tex tx = nw_tex_load(s, tid);
  if (tx.kind == NWT_CHECKER) {
    const float sines = (nw_sin(10.0f * p.x) * nw_sin(10.0f * p.y)) * nw_sin(10.0f * p.z);
    tx = nw_tex_load(s, sines < 0.0f ? tx.b : tx.a);
  }
  return nw_tex_leaf(s, &tx, u, v, p);
}
static int nw_tex_needs_uv(const or_nw_scene *s, int32_t tid) {
  const nw_tex t = nw_tex_load(s, tid);
  if (t.kind == NWT_IMAGE) return 1;
  if (t.kind == NWT_CHECKER) return nw_tex_load(s, t.a).kind == NWT_IMAGE || nw_tex_load(s, t.b).kind == NWT_IMAGE;
  return 0;
}
/* sphere.h:30-40 */
static void nw_sphere_uv(NV p, float *u, float *v) {
  const float theta = nw_acos(-p.y);
  const float phi = nw_atan2(-p.z, p.x) + 3.14159274f;
  *u = phi / (2.0f * 3.14159274f);
  *v = theta / 3.14159274f;
}

/* ---- hit record and materials --------------------------------------------- */
typedef struct nw_rec {
  NV p, n;
  float u, v;
  int32_t mat;
} nw_rec;
/* kk: the object's insertion index (finds a triangle's attribute record) */
static nw_rec nw_make_rec(const or_nw_scene *s, int32_t kk, const nw_obj *ob, NV ow, NV dw, float time, float t, int face) {
  nw_rec r;
  r.mat = ob->mat;
  r.u = 0.0f;
  r.v = 0.0f;
  nw_inst in = {1.0f, 0.0f, {0.0f, 0.0f, 0.0f}, 0};
  if (ob->inst >= 0) in = nw_inst_load(s, ob->inst);
  NV o = ow, d = dw;
  if (ob->inst >= 0) nw_local(&in, &o, &d);
  if (ob->kind == NW_MEDIUM) { /* constant_medium.h:73-77 */
    float r1 = 0.0f;
    (void)nw_hit_boundary(ob, o, d, time, -INFINITY, INFINITY, &r1);
    if (r1 < 0.0f) r1 = 0.0f;
    r.p = nat(ow, dw, r1);
    r.n = nv(1.0f, 0.0f, 0.0f);
    return r;
  }
  NV p = nat(o, d, t), n;
  const float *m = s->mat + 4 * (size_t)ob->mat;
  const int mkind = nw_ibits(m[0]);
  const int need_uv = mkind != NWM_DIEL && nw_tex_needs_uv(s, nw_ibits(m[1]));
  if (ob->kind == NW_SPHERE || ob->kind == NW_MOVING) {
    const NV c = ob->kind == NW_SPHERE ? nv(ob->g0[0], ob->g0[1], ob->g0[2]) : nw_center(ob, time);
    const float inv_r = 1.0f / ob->g0[3];
    n = nv(inv_r * (p.x - c.x), inv_r * (p.y - c.y), inv_r * (p.z - c.z));
    if (need_uv) nw_sphere_uv(n, &r.u, &r.v);
  } else if (ob->kind == NW_TRIANGLE) {
    /* "record (make_rec)" of the triangle specification, then "Triangle
     * attributes ... THE SPECIFICATION" for a triangle with a record */
    float v0[3], v1[3], v2[3];
    nw_tri_verts(ob, v0, v1, v2);
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const NV c = nv(e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]);
    const float inv_len = 1.0f / sqrtf(ndot(c, c));
    const NV ng = nv(c.x * inv_len, c.y * inv_len, c.z * inv_len);
    n = ng;
    const int32_t ai = s->n_attr > 0 ? s->attr_of_obj[kk] : -1;
    if (ai >= 0) {
      const float *ar = s->attr + 16 * (size_t)ai;
      const float *n0 = ar, *n1 = ar + 3, *n2 = ar + 6, *t0 = ar + 9, *t1 = ar + 11, *t2 = ar + 13;
      const int32_t flags = nw_ibits(ar[15]);
      const nw_tri_fn f = nw_tri_edges(o, d, v0, v1, v2);
      const float b0 = f.U / f.det, b1 = f.V / f.det, b2 = f.W / f.det;
      if (flags & 1) {
        NV ns = nv(fmaf(b2, n2[0], fmaf(b1, n1[0], b0 * n0[0])), fmaf(b2, n2[1], fmaf(b1, n1[1], b0 * n0[1])),
                   fmaf(b2, n2[2], fmaf(b1, n1[2], b0 * n0[2])));
        const float l2 = ndot(ns, ns);
        if (l2 > 0.0f) {
          const float inv_l = 1.0f / sqrtf(l2);
          ns = nv(ns.x * inv_l, ns.y * inv_l, ns.z * inv_l);
          const float a = ndot(d, ng), b = ndot(d, ns);
          if ((a > 0.0f && b > 0.0f) || (a < 0.0f && b < 0.0f)) n = ns;
        }
      }
      if (need_uv) {
        if (flags & 2) {
          r.u = fmaf(b2, t2[0], fmaf(b1, t1[0], b0 * t0[0]));
          r.v = fmaf(b2, t2[1], fmaf(b1, t1[1], b0 * t0[1]));
        } else {
          r.u = b1;
          r.v = b2;
        }
      }
    } else if (need_uv) {
      const nw_tri_fn f = nw_tri_edges(o, d, v0, v1, v2);
      r.u = f.V / f.det;
      r.v = f.W / f.det;
    }
  } else {
    int kind = ob->kind;
    float a0, a1, b0, b1, x, y;
    if (kind == NW_BOX) {
      kind = face < 2 ? NW_XY : face < 4 ? NW_XZ : NW_YZ;
      if (kind == NW_XY) { a0 = ob->g0[0]; a1 = ob->g1[0]; b0 = ob->g0[1]; b1 = ob->g1[1]; }
      else if (kind == NW_XZ) { a0 = ob->g0[0]; a1 = ob->g1[0]; b0 = ob->g0[2]; b1 = ob->g1[2]; }
      else { a0 = ob->g0[1]; a1 = ob->g1[1]; b0 = ob->g0[2]; b1 = ob->g1[2]; }
    } else {
      a0 = ob->g0[0]; a1 = ob->g0[1]; b0 = ob->g0[2]; b1 = ob->g0[3];
    }
    if (kind == NW_XY) { x = fmaf(t, d.x, o.x); y = fmaf(t, d.y, o.y); n = nv(0.0f, 0.0f, 1.0f); }
    else if (kind == NW_XZ) { x = fmaf(t, d.x, o.x); y = fmaf(t, d.z, o.z); n = nv(0.0f, 1.0f, 0.0f); }
    else { x = fmaf(t, d.y, o.y); y = fmaf(t, d.z, o.z); n = nv(1.0f, 0.0f, 0.0f); }
    if (need_uv) { /* as the spheres: u = v = 0 where no texture reads them */
      r.u = (x - a0) / (a1 - a0);
      r.v = (y - b0) / (b1 - b0);
    }
  }
  if (in.flags & 1) {
    p = nw_rot_world(&in, p);
    n = nw_rot_world(&in, n);
  }
  if (in.flags & 2) p = nv(p.x + in.off[0], p.y + in.off[1], p.z + in.off[2]);
  r.p = p;
  r.n = n;
  return r;
}
/* material.h:97-101 */
static float nw_schlick(float cosine, float ri) {
  float r0 = (1.0f - ri) / (1.0f + ri);
  r0 = r0 * r0;
  return fmaf(1.0f - r0, pow5f(1.0f - cosine), r0);
}
static int nw_scatter(const or_nw_scene *s, const nw_rec *rec, NV din, xo *g, NV *atten, NV *dir) {
  const float *m = s->mat + 4 * (size_t)rec->mat;
  const int kind = nw_ibits(m[0]), tex = nw_ibits(m[1]);
  const float fuzz = m[2], ir = m[3];
  if (kind == NWM_LAMB) { /* material.h:45-55 */
    const NV rs = fast_in_sphere_direct(g);
    const NV pn = nv(rec->p.x + rec->n.x, rec->p.y + rec->n.y, rec->p.z + rec->n.z);
    const NV target = nv(pn.x + rs.x, pn.y + rs.y, pn.z + rs.z);
    *dir = nv(target.x - rec->p.x, target.y - rec->p.y, target.z - rec->p.z);
    *atten = nw_tex_value(s, tex, rec->u, rec->v, rec->p);
    return 1;
  }
  if (kind == NWM_METAL) { /* material.h:72-86 */
    const NV refl = fast_reflect(fast_unit(din), rec->n);
    const NV rs = fast_in_sphere_direct(g);
    *dir = nv(fmaf(fuzz, rs.x, refl.x), fmaf(fuzz, rs.y, refl.y), fmaf(fuzz, rs.z, refl.z));
    *atten = nw_tex_value(s, tex, rec->u, rec->v, rec->p);
    return ndot(*dir, rec->n) > 0.0f;
  }
  if (kind == NWM_DIEL) { /* material.h:119-148, refract :103-114 */
    const NV n = rec->n;
    const NV reflected = fast_reflect(din, n);
    *atten = nv(1.0f, 1.0f, 1.0f);
    const float dn = ndot(din, n);
    const float dlen = sqrtf(ndot(din, din));
    NV outward;
    float ni, cosine;
    if (dn > 0.0f) {
      outward = nv(-n.x, -n.y, -n.z);
      ni = ir;
      cosine = dn / dlen;
      cosine = sqrtf(1.0f - (ir * ir) * fmaf(-cosine, cosine, 1.0f));
    } else {
      outward = n;
      ni = 1.0f / ir;
      cosine = -dn / dlen;
    }
    const NV uv = fast_unit(din);
    const float dt = ndot(uv, outward);
    const float disc = 1.0f - (ni * ni) * fmaf(-dt, dt, 1.0f);
    NV refracted = nv(0.0f, 0.0f, 0.0f);
    float reflect_prob = 1.0f;
    if (disc > 0.0f) {
      const float sq = sqrtf(disc);
      refracted = nv(fmaf(-outward.x, sq, ni * fmaf(-outward.x, dt, uv.x)),
                     fmaf(-outward.y, sq, ni * fmaf(-outward.y, dt, uv.y)),
                     fmaf(-outward.z, sq, ni * fmaf(-outward.z, dt, uv.z)));
      reflect_prob = nw_schlick(cosine, ir);
    }
    *dir = xo_uni(g) < reflect_prob ? reflected : refracted;
    return 1;
  }
  if (kind == NWM_ISO) { /* material.h:180-190 */
    *dir = fast_in_sphere_direct(g);
    *atten = nw_tex_value(s, tex, rec->u, rec->v, rec->p);
    return 1;
  }
  return 0; /* diffuse_light */
}

/* ---- one camera sample: get_color main.cu:47-101 (forward form) ---------- */
static NV nw_sample(const or_nw_scene *s, const int32_t *med_list, int32_t nmed, const fast_cam *k, float t0,
                    float t1, int32_t W, int32_t H, int32_t max_depth, int32_t i, int32_t j, xo *g, int64_t *segs,
                    int64_t *won /* NW_KINDS + 1: segment winners by kind, then misses */) {
  float ju, jv;
  xo_pair(g, &ju, &jv);
  const float u = ((float)i + ju) / (float)W, v = ((float)j + jv) / (float)H;
  NV o, d;
  fast_get_ray(k, u, v, g, &o, &d);
  const float time = fmaf(xo_uni(g), t1 - t0, t0);
  NV T = nv(1.0f, 1.0f, 1.0f);
  for (int32_t depth = 0;;) {
    (*segs)++;
    const uint64_t seg_key = nmed > 0 ? xo_next(g) : 0ull;
    float t;
    int face;
    const int32_t kk = nw_hit_world(s, med_list, nmed, o, d, time, seg_key, &t, &face);
    if (kk < 0) {
      won[NW_KINDS]++;
      return nv(T.x * s->bg[0], T.y * s->bg[1], T.z * s->bg[2]);
    }
    const nw_obj ob = nw_load(s, kk);
    won[ob.kind]++;
    const nw_rec rec = nw_make_rec(s, kk, &ob, o, d, time, t, face);
    const float *m = s->mat + 4 * (size_t)rec.mat;
    if (nw_ibits(m[0]) == NWM_LIGHT) {
      const NV e = nw_tex_value(s, nw_ibits(m[1]), rec.u, rec.v, rec.p);
      return nv(T.x * e.x, T.y * e.y, T.z * e.z);
    }
    NV at, nd;
    if (!nw_scatter(s, &rec, d, g, &at, &nd)) return nv(0.0f, 0.0f, 0.0f);
    T = nv(T.x * at.x, T.y * at.y, T.z * at.z);
    o = rec.p;
    d = nd;
    if (++depth >= max_depth) return nv(s->bg[0], s->bg[1], s->bg[2]);
  }
}

/* Rows row0 + r*row_step (r < nrows) of a W x H image: per-pixel sums over
 * spp samples (int64 fixed point, then float), same stream keys as the GPU.
 * Returns 0, or -1 on a bad argument or an object kind this file does not
 * know; *segments = world.hit calls; winners (null, or NW_KINDS + 1 counts):
 * over all those calls, the winners by object kind, then the misses. */
int32_t or_nw_render_winners(const or_nw_scene *s, const or_camera *c, double time0, double time1, int32_t W, int32_t H,
                             int32_t spp, int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step,
                             int32_t nrows, float *out, int64_t *segments, int64_t *winners) {
  if (!s || !c || W < 1 || H < 1 || spp < 1 || spp >= (1 << 24) || max_depth < 1 || nrows < 0) return -1;
  if (nw_scene_known(s) != 0) return -1;
  fast_cam k;
  fast_build_cam(c, &k);
  int32_t med_list[64], nmed = 0;
  for (int32_t q = 0; q < s->n_obj; q++)
    if (nw_load(s, q).kind == NW_MEDIUM) {
      if (nmed == 64) return -1;
      med_list[nmed++] = q;
    }
  const float t0 = (float)time0, t1 = (float)time1;
  int64_t total = (int64_t)nrows * W, segs = 0;
  int64_t won[NW_KINDS + 1] = {0};
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : segs, won[:NW_KINDS + 1])
  for (int64_t q = 0; q < total; q++) {
    const int32_t r = (int32_t)(q / W), i = (int32_t)(q % W);
    const int32_t j = row0 + r * row_step;
    int64_t acc[3] = {0, 0, 0};
    if (j >= 0 && j < H) {
      const uint64_t pixel = (uint64_t)j * (uint64_t)W + (uint64_t)i;
      for (int32_t smp = 0; smp < spp; smp++) {
        xo g;
        xo_init(&g, seed, pixel, (uint32_t)smp);
        const NV col = nw_sample(s, med_list, nmed, &k, t0, t1, W, H, max_depth, i, j, &g, &segs, won);
        acc[0] += to_fixed(col.x);
        acc[1] += to_fixed(col.y);
        acc[2] += to_fixed(col.z);
      }
    }
    for (int ch = 0; ch < 3; ch++) out[3 * q + ch] = from_fixed(acc[ch]);
  }
  if (segments) *segments = segs;
  if (winners) memcpy(winners, won, sizeof won);
  return 0;
}
int32_t or_nw_render(const or_nw_scene *s, const or_camera *c, double time0, double time1, int32_t W, int32_t H,
                     int32_t spp, int32_t max_depth, uint64_t seed, int32_t row0, int32_t row_step, int32_t nrows,
                     float *out, int64_t *segments) {
  return or_nw_render_winners(s, c, time0, time1, W, H, spp, max_depth, seed, row0, row_step, nrows, out, segments, 0);
}

/* Function hooks for tests: the transcendentals on n inputs
 * (fn 0 sin, 1 log, 2 atan2(x, y pairs: in[2i], in[2i+1]), 3 acos). */
void or_nw_math(int32_t fn, int32_t n, const float *in, float *out) {
  for (int32_t i = 0; i < n; i++) {
    if (fn == 0) out[i] = nw_sin(in[i]);
    else if (fn == 1) out[i] = nw_log(in[i]);
    else if (fn == 2) out[i] = nw_atan2(in[2 * i], in[2 * i + 1]);
    else out[i] = nw_acos(in[i]);
  }
}

/* Test hook: the box hit (box.h over aarect.h, tmin 0.001, tmax inf) of n
 * rays {o.xyz, d.xyz} against n boxes {p0.xyz, p1.xyz}, in the reference's
 * division form (nw_hit_box) and in the reciprocal form the kernels and the
 * fast oracle use (nw_hit_box_inv): t and face of each (face -1: miss).  It
 * keeps the "<= 1 ulp in the plane parameter" statement about the
 * reciprocal form tested (DESIGN.md §9). */
void or_nw_box_forms(int32_t n, const float *rays, const float *boxes, float *t_div, int32_t *f_div, float *t_inv,
                     int32_t *f_inv) {
  for (int32_t i = 0; i < n; i++) {
    const float *r = rays + 6 * i, *b = boxes + 6 * i;
    const NV o = {r[0], r[1], r[2]}, d = {r[3], r[4], r[5]};
    const NV inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    const float p0[4] = {b[0], b[1], b[2], 0.0f}, p1[4] = {b[3], b[4], b[5], 0.0f};
    f_div[i] = nw_hit_box(o, d, p0, p1, 0.001f, INFINITY, &t_div[i]);
    f_inv[i] = nw_hit_box_inv(o, d, inv, p0, p1, 0.001f, INFINITY, &t_inv[i]);
  }
}

/* Debug mirror of rt_nw_debug_trace: the segments of one camera sample
 * (their number; -1: an object kind this file does not know). */
int32_t or_nw_trace(const or_nw_scene *s, const or_camera *c, double time0, double time1, int32_t W, int32_t H,
                    int32_t max_depth, uint64_t seed, int32_t i, int32_t j, int32_t smp, float *rec, int32_t cap) {
  if (nw_scene_known(s) != 0) return -1;
  fast_cam k;
  fast_build_cam(c, &k);
  int32_t med_list[64], nmed = 0;
  for (int32_t q = 0; q < s->n_obj && nmed < 64; q++)
    if (nw_load(s, q).kind == NW_MEDIUM) med_list[nmed++] = q;
  xo g;
  xo_init(&g, seed, (uint64_t)j * (uint64_t)W + (uint64_t)i, (uint32_t)smp);
  float ju, jv;
  xo_pair(&g, &ju, &jv);
  NV o, d;
  fast_get_ray(&k, ((float)i + ju) / (float)W, ((float)j + jv) / (float)H, &g, &o, &d);
  const float t0 = (float)time0, t1 = (float)time1;
  const float time = fmaf(xo_uni(&g), t1 - t0, t0);
  int32_t n = 0;
  for (int32_t depth = 0; depth < max_depth && n < cap; depth++) {
    const uint64_t seg_key = nmed > 0 ? xo_next(&g) : 0ull;
    float t;
    int face;
    const int32_t kk = nw_hit_world(s, med_list, nmed, o, d, time, seg_key, &t, &face);
    float *r = rec + 12 * n++;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; r[6] = t;
    r[7] = nw_fbits(kk);
    r[8] = r[9] = r[10] = 0.0f;
    r[11] = nw_fbits(face);
    if (kk < 0) break;
    const nw_obj ob = nw_load(s, kk);
    const nw_rec rc = nw_make_rec(s, kk, &ob, o, d, time, t, face);
    r[8] = rc.n.x; r[9] = rc.n.y; r[10] = rc.n.z;
    const float *m = s->mat + 4 * (size_t)rc.mat;
    NV at, nd;
    if (nw_ibits(m[0]) == NWM_LIGHT || !nw_scatter(s, &rc, d, &g, &at, &nd)) break;
    o = rc.p;
    d = nd;
  }
  return n;
}

/* Closest hit of n given rays by brute force over the list (nw_hit_world):
 * the checker of rt_nw_debug_hits.  rays: {o.xyz, d.xyz, time, unused} per
 * ray; keys: the segments' medium keys (null: 0).  Out: insertion index
 * (-1: miss), t, box face (-1: none).  Returns 0, or -1 for an object kind
 * this file does not know. */
int32_t or_nw_hits(const or_nw_scene *s, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id,
                   float *out_t, int32_t *out_face) {
  if (nw_scene_known(s) != 0) return -1;
  int32_t med_list[64], nmed = 0;
  for (int32_t q = 0; q < s->n_obj && nmed < 64; q++)
    if (nw_load(s, q).kind == NW_MEDIUM) med_list[nmed++] = q;
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; i++) {
    const float *r = rays + 8 * (size_t)i;
    NV o, d;
    o.x = r[0]; o.y = r[1]; o.z = r[2];
    d.x = r[3]; d.y = r[4]; d.z = r[5];
    float t;
    int face;
    out_id[i] = nw_hit_world(s, med_list, nmed, o, d, r[6], keys ? keys[i] : 0ull, &t, &face);
    out_t[i] = t;
    out_face[i] = face;
  }
  return 0;
}

/* Mirror of rt_nw_debug_records: the closest hit of each ray as or_nw_hits
 * finds it, then the record a render makes of it.  Out per ray: insertion
 * index, t, {p.xyz, n.xyz, u, v} (world space) and the material; a miss writes
 * index -1 and zeros.  Returns 0, or -1 for an unknown object kind. */
int32_t or_nw_records(const or_nw_scene *s, const float *rays, const uint64_t *keys, int32_t n, int32_t *out_id,
                      float *out_t, float *out_pnuv, int32_t *out_mat) {
  if (nw_scene_known(s) != 0) return -1;
  int32_t med_list[64], nmed = 0;
  for (int32_t q = 0; q < s->n_obj && nmed < 64; q++)
    if (nw_load(s, q).kind == NW_MEDIUM) med_list[nmed++] = q;
#pragma omp parallel for schedule(static)
  for (int32_t i = 0; i < n; i++) {
    const float *r = rays + 8 * (size_t)i;
    float *q = out_pnuv + 8 * (size_t)i;
    const NV o = nv(r[0], r[1], r[2]), d = nv(r[3], r[4], r[5]);
    float t;
    int face;
    const int32_t kk = nw_hit_world(s, med_list, nmed, o, d, r[6], keys ? keys[i] : 0ull, &t, &face);
    out_id[i] = kk;
    if (kk < 0) {
      out_t[i] = 0.0f;
      out_mat[i] = 0;
      for (int c = 0; c < 8; c++) q[c] = 0.0f;
      continue;
    }
    const nw_obj ob = nw_load(s, kk);
    const nw_rec rc = nw_make_rec(s, kk, &ob, o, d, r[6], t, face);
    out_t[i] = t;
    out_mat[i] = rc.mat;
    q[0] = rc.p.x; q[1] = rc.p.y; q[2] = rc.p.z;
    q[3] = rc.n.x; q[4] = rc.n.y; q[5] = rc.n.z;
    q[6] = rc.u; q[7] = rc.v;
  }
  return 0;
}
