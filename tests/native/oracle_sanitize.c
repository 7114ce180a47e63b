/* oracle_sanitize.c — TEST INFRASTRUCTURE: drives the oracle (the checker,
 * oracle/rt_oracle.c) under ASan + UBSan, and its OpenMP fast mode under
 * ThreadSanitizer (oracle/Makefile targets asan / tsan; tests/test_sanitize.py).
 * Small renders in ref and fast mode, the function KATs' entry points, the
 * NaN/inf guard, the RNG helpers and a Next-Week scene of triangles.  Exit
 * 0 = every check passed and the sanitizers reported nothing (they abort on
 * the first report). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../oracle/rt_oracle.h"

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

int main(void) {
  static double g[4 * 600], m[4 * 600];
  static int32_t k[600];
  or_glibc rs;
  or_glibc_seed(&rs, 1);
  const int32_t n = or_final_scene(&rs, g, k, m, 600);
  CHECK(n == 487);
  CHECK(or_final_scene(&rs, g, k, m, 10) == -1);
  or_scene sc = {n, g, k, m};
  or_camera cam;
  const double lf[3] = {13, 2, 3}, la[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  or_camera_make(&cam, lf, la, up, 20, 1.5, 0.1, 10);
  /* fast mode, OpenMP over pixels (TSan build: data races would be reported) */
  enum { W = 24, H = 16, S = 4 };
  static float out[W * H * 3];
  CHECK(or_fast_render(&sc, &cam, W, H, S, 50, 1984, 0, 1, H, out) == 0);
  static float strip[5 * W * 3];
  CHECK(or_fast_render(&sc, &cam, W, H, S, 50, 1984, 3, 4, 5, strip) == 0);  /* rows 3..19: past H zero-filled */
  for (int r = 0; r < 4; ++r) CHECK(memcmp(strip + r * W * 3, out + (3 + 4 * r) * W * 3, sizeof(float) * W * 3) == 0);
  for (int i = 0; i < W * 3; ++i) CHECK(strip[4 * W * 3 + i] == 0.0f);
  static int64_t fx[W * H * 3];
  CHECK(or_fast_render_fixed(&sc, &cam, W, H, S, 50, 1984, 0, 1, H, fx) == 0);
  CHECK(or_fast_segments(&sc, &cam, W, H, S, 50, 1984, 0, 1, H) > W * H * S);
  float one[3];
  CHECK(or_fast_sample(&sc, &cam, W, H, 50, 1984, 3, 4, 0, one) >= 1);
  /* ref mode: a few pixels single-threaded from the glibc stream */
  static double ref[8 * 3];
  or_glibc_seed(&rs, 7);
  CHECK(or_ref_worker(&sc, &cam, W, H, 2, 50, 100, 108, &rs, ref) > 0);
  for (int i = 0; i < 24; ++i) CHECK(isfinite(ref[i]) && ref[i] >= 0);
  double kat[3];
  (void)or_ref_kat(&sc, &cam, W, H, 50, 5, 6, 3, kat);
  /* function entry points */
  const double c0[3] = {0, 0, -1}, o[3] = {0, 0, 0}, d[3] = {0, 0, -1};
  double t, p[3], nrm[3];
  int32_t front;
  CHECK(or_ref_sphere_hit(c0, 0.5, o, d, 0.001, INFINITY, &t, p, nrm, &front) == 1 && t == 0.5);
  CHECK(or_ref_sphere_hit(c0, -0.4, o, d, 0.001, INFINITY, &t, p, nrm, &front) == 1);
  double rr[3];
  or_ref_refract(d, nrm, 1.5, rr);
  or_ref_reflect(d, nrm, rr);
  CHECK(or_ref_reflectance(0.5, 1.5) > 0);
  const double z[3] = {0, 0, 0};
  CHECK(or_ref_near_zero(z) == 1);
  double at[3], so[3], sd[3];
  int32_t nx;
  const double mat[4] = {0.5, 0.5, 0.5, 0.3};
  for (int kind = 0; kind < 3; ++kind) (void)or_ref_scatter(kind, mat, d, p, nrm, 1, 11, at, so, sd, &nx);
  uint64_t rng[8];
  or_fast_rng(1984, 12345, 7, 8, rng);
  static float dirs[4 * 300 * 3];
  for (int kind = 0; kind < 4; ++kind) or_fast_dirs(kind, 5, 300, dirs + kind * 900);
  /* non-finite path colours: the guarded fixed-point conversion */
  static double g2[4 * 8], m2[4 * 8];
  static int32_t k2[8];
  const int32_t n2 = or_learn_scene(g2, k2, m2, 8);
  m2[4 * 1 + 0] = NAN;
  m2[4 * 4 + 0] = m2[4 * 4 + 1] = m2[4 * 4 + 2] = 1e30;
  or_scene s2 = {n2, g2, k2, m2};
  or_camera c2;
  const double lf2[3] = {3, 3, 2}, la2[3] = {0, 0, -1};
  or_camera_make(&c2, lf2, la2, up, 20, 16.0 / 9.0, 0.5, sqrt(9 + 9 + 9));
  static float o2[16 * 9 * 3];
  CHECK(or_fast_render(&s2, &c2, 16, 9, 4, 50, 1984, 0, 1, 9, o2) == 0);
  for (int i = 0; i < 16 * 9 * 3; ++i) CHECK(isfinite(o2[i]));
  /* Next-Week oracle, triangles: one under an instance with an attribute
   * record (smooth normals + uvs, an image-textured lambertian), one plain
   * (metal), one collinear (never hit), over a ground sphere; 8 x 8 x 2 */
  {
    union { int32_t i; float f; } b;
#define IB(x) (b.i = (x), b.f)
    static float obj[4 * 16], inst[8], mat[3 * 4], tex[3 * 8], attr[16], pvec[4], rays[64 * 8];
    static int32_t attr_of[4] = {0, -1, -1, -1}, pperm[4], idesc[4] = {0, 2, 2, 0};
    static const uint8_t px[12] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 200, 200, 200};
    const float tri[3][9] = {{-2, -1, 0, 2, -1, 0.5f, 0, 2, -0.5f}, {1, -1, 1, 3, -1, 1, 2, 1.5f, 0.5f}, {0, 0, 0, 1, 1, 1, 2, 2, 2}};
    for (int q = 0; q < 3; ++q) {
      memcpy(obj + 16 * q, tri[q], sizeof tri[q]);
      obj[16 * q + 12] = IB(7);
      obj[16 * q + 13] = IB(q == 1 ? 1 : 0);
      obj[16 * q + 14] = IB(q == 0 ? 0 : -1);
    }
    float *gs = obj + 16 * 3; /* ground sphere */
    gs[1] = -1001.5f; gs[3] = 1000.0f; gs[12] = IB(0); gs[13] = IB(2); gs[14] = IB(-1);
    inst[0] = 0.9396926f; inst[1] = 0.3420201f; inst[2] = 0.2f; inst[3] = 0.1f; inst[4] = -0.3f; inst[5] = IB(3);
    mat[0] = IB(0); mat[1] = IB(0);                                  /* lambertian(image) */
    mat[4] = IB(1); mat[5] = IB(1); mat[6] = 0.2f;                    /* metal(solid), fuzz */
    mat[8] = IB(0); mat[9] = IB(2);                                  /* lambertian(solid) */
    tex[0] = IB(3); tex[1] = IB(0);
    tex[8] = IB(0); tex[12] = 0.8f; tex[13] = 0.8f; tex[14] = 0.9f;
    tex[16] = IB(0); tex[20] = 0.5f; tex[21] = 0.5f; tex[22] = 0.5f;
    const float nrm[9] = {-0.4f, -0.3f, 0.86f, 0.4f, -0.3f, 0.86f, 0, 0.5f, 0.86f}, uv[6] = {0, 0, 1, 0, 0.5f, 1};
    memcpy(attr, nrm, sizeof nrm);
    memcpy(attr + 9, uv, sizeof uv);
    attr[15] = IB(3);
#undef IB
    or_nw_scene ns = {4, 1, obj, inst, mat, tex, pvec, pperm, idesc, px, {0.7f, 0.8f, 1.0f}, 1, attr, attr_of};
    or_camera nc;
    const double nlf[3] = {0.5, 0.5, 6}, nla[3] = {0.5, 0, 0};
    or_camera_make(&nc, nlf, nla, up, 40, 1.0, 0.05, 6);
    static float nout[8 * 8 * 3];
    int64_t nsegs = 0, won[9];
    CHECK(or_nw_render_winners(&ns, &nc, 0.0, 1.0, 8, 8, 2, 50, 1984, 0, 1, 8, nout, &nsegs, won) == 0);
    CHECK(won[7] > 0 && won[0] > 0 && won[5] == 0 && nsegs > 8 * 8 * 2);
    for (int i = 0; i < 8 * 8 * 3; ++i) CHECK(isfinite(nout[i]) && nout[i] >= 0);
    /* a ray at the instanced triangle, one along the collinear triangle's line,
     * then a fan of rays from the camera's side (the OpenMP loops of
     * or_nw_hits and or_nw_records get work for every thread) */
    enum { NR = 64 };
    const float r0[8] = {0.3f, 0.2f, 5, 0, 0, -1, 0.5f, 0}, r1[8] = {-1, -1, -1, 1, 1, 1, 0.5f, 0};
    memcpy(rays, r0, sizeof r0);
    memcpy(rays + 8, r1, sizeof r1);
    for (int q = 2; q < NR; ++q) {
      float *r = rays + 8 * q;
      r[0] = 0.5f; r[1] = 0.5f; r[2] = 6.0f;
      r[3] = 0.1f * (float)(q % 8) - 0.35f; r[4] = 0.1f * (float)(q / 8) - 0.45f; r[5] = -1.0f;
      r[6] = (float)q / NR;
    }
    static int32_t hid[NR], hface[NR], hmat[NR], rid[NR];
    static float ht[NR], rt[NR], hrec[8 * NR];
    CHECK(or_nw_hits(&ns, rays, 0, NR, hid, ht, hface) == 0 && hid[0] == 0 && hid[1] != 2);
    CHECK(or_nw_records(&ns, rays, 0, NR, rid, rt, hrec, hmat) == 0 && rid[0] == 0 && hmat[0] == 0);
    int on_tri = 0;
    for (int q = 0; q < NR; ++q) {
      CHECK(rid[q] == hid[q] && hid[q] != 2 && hface[q] == -1);
      on_tri += hid[q] == 0 || hid[q] == 1;
    }
    CHECK(on_tri >= 8);
    static float trace[12 * 8];
    CHECK(or_nw_trace(&ns, &nc, 0.0, 1.0, 8, 8, 50, 1984, 4, 4, 0, trace, 8) >= 1);
    obj[16 * 2 + 12] = nrm[8]; /* an unknown kind (the bits of 0.86f) is refused */
    CHECK(or_nw_render(&ns, &nc, 0.0, 1.0, 8, 8, 2, 50, 1984, 0, 1, 8, nout, &nsegs) == -1);
    CHECK(or_nw_hits(&ns, rays, 0, NR, hid, ht, hface) == -1);
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("oracle_sanitize: all checks passed\n");
  return failures ? 1 : 0;
}
