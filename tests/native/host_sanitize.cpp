// host_sanitize.cpp — drives librtmi's HOST code under AddressSanitizer +
// UndefinedBehaviorSanitizer (built by `make -C a_dive_into_ray_tracing_amd/csrc
// asan`; run by tests/test_sanitize.py, CPU only).  Covers the scene
// generator, scene text files (valid and malformed), camera, PPM (P3/P6), PFM,
// quantisation, the builders of the acceleration structures (BVH, grid, tile
// tables, the grid's global-memory image: rtmi_accel_build.cpp, through its
// rt_debug_* entry points), the Next-Week scene builder, presets and
// flattening, and the error paths of each.  No GPU call is made.  Exit 0 =
// every check passed and the sanitizers reported nothing (they abort on the
// first report).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtmi.h"
#include "../../include/rtmi_nw.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static void write_file(const std::string &p, const char *text) {
  FILE *f = std::fopen(p.c_str(), "wb");
  std::fputs(text, f);
  std::fclose(f);
}

// the validation entry points of rtmi_accel_build.cpp (exported, not in rtmi.h)
extern "C" {
int rt_debug_grid_strides(const int32_t *n3, uint32_t *strides2);
int rt_debug_grid_layout(const rt_scene *scene, int32_t *dims3, uint32_t *strides2, float *box6);
int rt_debug_tile_list(const rt_scene *scene, const rt_camera *camera, int32_t W, int32_t H, int32_t row0,
                       int32_t row_step, int32_t nrows, int32_t tile_w, int32_t tile, int32_t cap, int32_t *out_indices,
                       int32_t *out_count);
int rt_debug_tile_big(const rt_scene *scene, const rt_camera *camera, int32_t W, int32_t H, int32_t row0,
                      int32_t row_step, int32_t nrows, int32_t tile_w, int32_t tile, int32_t *out_indices,
                      int32_t *out_count);
int rt_debug_accel_digest(const rt_scene *scene, uint64_t *out8);
}

// n lambertian spheres, sphere i's {centre, radius} written by fill(i, c); the
// arrays live until the next call
template <class Fill> static rt_scene plain_scene(int32_t n, Fill fill) {
  static std::vector<double> cr, mp;
  static std::vector<int32_t> kd;
  cr.assign(4 * size_t(n), 0.0);
  mp.assign(4 * size_t(n), 0.5);
  kd.assign(size_t(n), RT_MAT_LAMBERTIAN);
  for (int32_t i = 0; i < n; ++i) fill(i, cr.data() + 4 * size_t(i));
  return rt_scene{n, cr.data(), kd.data(), mp.data()};
}

// Every builder entry point on one scene: the digest (all of build_accel and
// the grid image), the grid layout, and the tile lists of every tile shape on a
// strided strip (rows 3, 7, .. of 48 x 32) and of one tile of the whole image.
// grid: the scene has a grid (else the three grid entry points refuse it);
// many_big: more than kTileBigMax big spheres, every big count is -1.
static void accel_checks(const rt_scene &sc, const rt_camera &cam, bool grid, bool many_big) {
  uint64_t dg[8] = {0};
  CHECK(rt_debug_accel_digest(&sc, dg) == 0 && dg[1] != 0);
  int32_t dims[3] = {0, 0, 0};
  uint32_t st[2] = {0, 0};
  float box[6];
  CHECK((rt_debug_grid_layout(&sc, dims, st, box) == 0) == grid);
  if (grid) CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && st[0] == 4u * dims[0] && st[1] == st[0] * dims[1]);
  const int caps[] = {32, 5};
  for (int tw : {0, 8, 16, 32, 64})
    for (int cap : caps) {
      const int W = 48, H = 32, tiles = 8;  // at most 8 tiles: 8 strip rows of 48 pixels
      std::vector<int32_t> idx(size_t(tiles) * 32, -7), cnt(tiles, -7), bidx(size_t(tiles) * 8, -7), bcnt(tiles, -7);
      CHECK((rt_debug_tile_list(&sc, &cam, W, H, 3, 4, H, tw, -1, cap, idx.data(), cnt.data()) == 0) == grid);
      CHECK((rt_debug_tile_big(&sc, &cam, W, H, 3, 4, H, tw, -1, bidx.data(), bcnt.data()) == 0) == grid);
      if (!grid) continue;
      const int ntiles = tw == 32 || tw == 64 ? 8 : 6;
      for (int t = 0; t < ntiles; ++t) {
        CHECK(cnt[t] >= -1 && cnt[t] <= cap);
        for (int i = 0; i < cnt[t]; ++i) CHECK(idx[size_t(t) * cap + i] >= 0 && idx[size_t(t) * cap + i] < sc.n);
        CHECK(many_big ? bcnt[t] == -1 : bcnt[t] >= 0 && bcnt[t] <= 8);
        for (int i = 0; i < bcnt[t]; ++i) CHECK(bidx[size_t(t) * 8 + i] >= 0 && bidx[size_t(t) * 8 + i] < sc.n);
      }
      for (int t = ntiles; t < tiles; ++t) CHECK(cnt[t] == -7 && bcnt[t] == -7);  // nothing written past the strip's tiles
    }
  int32_t one[32], c1 = -7;
  CHECK((rt_debug_tile_list(&sc, &cam, 48, 32, 0, 1, 32, 0, 5, 32, one, &c1) == 0) == grid);
  CHECK((rt_debug_tile_big(&sc, &cam, 48, 32, 0, 1, 32, 0, 5, one, &c1) == 0) == grid);
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  // --- scenes ---------------------------------------------------------------
  std::vector<double> g(4 * 600), m(4 * 600);
  std::vector<int32_t> k(600);
  int32_t n = 0;
  CHECK(rt_scene_random(1, g.data(), k.data(), m.data(), 600, &n) == 0 && n == 487);
  CHECK(rt_scene_random(1, g.data(), k.data(), m.data(), 10, &n) != 0);  // cap too small
  int32_t nl = 0;
  CHECK(rt_scene_learn(g.data(), k.data(), m.data(), 600, &nl) == 0 && nl == 5);
  CHECK(rt_scene_random(1, g.data(), k.data(), m.data(), 600, &n) == 0);
  rt_scene sc{n, g.data(), k.data(), m.data()};
  const std::string sf = dir + "/scene.txt";
  CHECK(rt_scene_write(sf.c_str(), &sc) == 0);
  int32_t n2 = -1;
  CHECK(rt_scene_read(sf.c_str(), nullptr, nullptr, nullptr, 0, &n2) != 0 && n2 == n);  // sizing call
  std::vector<double> g2(4 * size_t(n)), m2(4 * size_t(n));
  std::vector<int32_t> k2(n);
  CHECK(rt_scene_read(sf.c_str(), g2.data(), k2.data(), m2.data(), n, &n2) == 0 && n2 == n);
  CHECK(std::memcmp(g2.data(), g.data(), g2.size() * sizeof(double)) == 0);
  CHECK(std::memcmp(m2.data(), m.data(), m2.size() * sizeof(double)) == 0);
  CHECK(std::memcmp(k2.data(), k.data(), k2.size() * sizeof(int32_t)) == 0);
  CHECK(rt_scene_write((dir + "/no/such/dir/x.txt").c_str(), &sc) != 0);
  CHECK(rt_scene_read((dir + "/missing.txt").c_str(), g2.data(), k2.data(), m2.data(), n, &n2) != 0);
  // malformed scene files: each must fail cleanly (no read past a buffer)
  const char *bad[] = {
      "",                                   // empty
      "3\n0 0 0 1 0 0.5 0.5 0.5 0\n",       // count larger than the rows
      "-5\n",                               // negative count
      "99999999999999999999\n",             // count overflow
      "1\n0 0 0 1 7 0.5 0.5 0.5 0\n",       // unknown material kind
      "1\n0 0 zero 1 0 0.5 0.5 0.5 0\n",    // not a number
      "1\n0 0 0 1 0 0.5 0.5\n",             // short row
      "# only a comment\n",
      "2\n0 0 0 1 0 0.5 0.5 0.5 0\n1 1 1 1 1 0.1 0.2 0.3 5\n",  // valid: fuzz > 1 kept as written
  };
  for (size_t b = 0; b < sizeof(bad) / sizeof(bad[0]); ++b) {
    const std::string p = dir + "/bad" + std::to_string(b) + ".txt";
    write_file(p, bad[b]);
    int32_t nb = 0;
    std::vector<double> gb(8), mb(8);
    std::vector<int32_t> kb(2);
    const int rc = rt_scene_read(p.c_str(), gb.data(), kb.data(), mb.data(), 2, &nb);
    if (b == 8) CHECK(rc == 0 && nb == 2);
    else CHECK(rc != 0);
  }
  // --- camera, quantisation, image files --------------------------------------
  rt_camera cam;
  const double lf[3] = {13, 2, 3}, la[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  CHECK(rt_camera_init(&cam, lf, la, up, 20, 1.5, 0.1, 10) == 0);
  CHECK(rt_camera_init(&cam, lf, lf, up, 20, 1.5, 0.1, 10) != 0);  // lookfrom == lookat
  CHECK(rt_camera_init(nullptr, lf, la, up, 20, 1.5, 0.1, 10) != 0);
  const int W = 7, H = 5, S = 3;
  std::vector<float> sum(size_t(W) * H * 3);
  for (size_t i = 0; i < sum.size(); ++i) sum[i] = float(i % 13) * 0.37f;
  sum[4] = NAN;
  sum[5] = INFINITY;
  sum[6] = -1.0f;
  std::vector<uint8_t> rgb(sum.size());
  CHECK(rt_quantize(sum.data(), W, H, S, rgb.data()) == 0);
  CHECK(rt_quantize(sum.data(), 0, H, S, rgb.data()) != 0);
  CHECK(rt_quantize(sum.data(), W, H, 0, rgb.data()) != 0);
  CHECK(rt_write_ppm((dir + "/a.ppm").c_str(), sum.data(), W, H, S, 0) == 0);
  CHECK(rt_write_ppm((dir + "/b.ppm").c_str(), sum.data(), W, H, S, 1) == 0);
  CHECK(rt_write_ppm((dir + "/no/such/dir/b.ppm").c_str(), sum.data(), W, H, S, 1) != 0);
  CHECK(rt_write_pfm((dir + "/a.pfm").c_str(), sum.data(), W, H, S) == 0);
  CHECK(rt_write_pfm((dir + "/a.pfm").c_str(), sum.data(), W, -1, S) != 0);
  // --- Next-Week scene builder ------------------------------------------------
  for (int which = 1; which <= 8; ++which) {
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == 0);
    std::vector<uint8_t> img(16 * 8 * 3, 128);
    rt_nw_camera nc;
    CHECK(rt_nw_scene_preset(s, which, which == 4 || which == 8 ? img.data() : nullptr, 16, 8, 1.0, 0, &nc) == 0);
    rt_nw_flat f;
    CHECK(rt_nw_scene_flat(s, &f) == 0 && f.n_obj > 0);
    double acc = 0;  // touch every flattened array end to end
    for (int64_t i = 0; i < int64_t(f.n_obj) * 16; ++i) acc += f.obj[i] == f.obj[i];
    for (int64_t i = 0; i < int64_t(f.n_inst) * 8; ++i) acc += f.inst[i] == f.inst[i];
    for (int64_t i = 0; i < int64_t(f.n_mat) * 4; ++i) acc += f.mat[i] == f.mat[i];
    for (int64_t i = 0; i < int64_t(f.n_tex) * 8; ++i) acc += f.tex[i] == f.tex[i];
    for (int64_t i = 0; i < int64_t(f.n_perlin) * 1024; ++i) acc += f.perlin_vec[i] == f.perlin_vec[i];
    for (int64_t i = 0; i < int64_t(f.n_perlin) * 768; ++i) acc += f.perlin_perm[i] >= 0;
    for (int64_t i = 0; i < f.image_bytes; ++i) acc += f.image_px[i];
    CHECK(acc > 0);
    CHECK(rt_nw_scene_destroy(s) == 0);
  }
  {  // builder error paths: bad handles and indices
    rt_nw_scene *s = nullptr;
    CHECK(rt_nw_scene_create(&s) == 0);
    const double c[3] = {0, 0, 0}, c1[3] = {1, 1, 1};
    const int32_t t = rt_nw_tex_solid(s, 0.5, 0.5, 0.5);
    CHECK(t >= 0);
    CHECK(rt_nw_mat_lambertian(s, 99) < 0);
    const int32_t mat = rt_nw_mat_lambertian(s, t);
    CHECK(mat >= 0);
    CHECK(rt_nw_sphere(s, c, 1.0, 42) < 0);
    const int32_t sp = rt_nw_sphere(s, c, 1.0, mat);
    CHECK(sp >= 0);
    CHECK(rt_nw_rect(s, 7, 0, 1, 0, 1, 0, mat) < 0);
    CHECK(rt_nw_box(s, c, c1, mat) >= 0);
    CHECK(rt_nw_translate(s, 1000, c1) < 0);
    CHECK(rt_nw_rotate_y(s, -1, 15) < 0);
    CHECK(rt_nw_constant_medium(s, 1000, 0.1, t) < 0);
    const int32_t ids[2] = {sp, 12345};
    CHECK(rt_nw_group(s, ids, 2) < 0);
    CHECK(rt_nw_tex_image(s, nullptr, 4, 4) >= 0);  // no data: the reference's cyan (texture.h:96)
    const uint8_t px[3] = {1, 2, 3};
    CHECK(rt_nw_tex_image(s, px, 0, 4) < 0 && rt_nw_tex_image(s, px, 1 << 16, 1 << 16) < 0);
    CHECK(rt_nw_world_add(s, sp) == 0);
    rt_nw_flat f;
    CHECK(rt_nw_scene_flat(s, &f) == 0 && f.n_obj == 1);
    CHECK(rt_nw_scene_destroy(s) == 0);
  }
  // --- builders of the acceleration structures (rtmi_accel_build.cpp) ---------
  {
    CHECK(rt_scene_random(1, g.data(), k.data(), m.data(), 600, &n) == 0);
    accel_checks(rt_scene{n, g.data(), k.data(), m.data()}, cam, true, false);
    CHECK(rt_scene_learn(g.data(), k.data(), m.data(), 600, &nl) == 0);
    accel_checks(rt_scene{nl, g.data(), k.data(), m.data()}, cam, true, false);
    // one sphere; 64 spheres with one centre and radius (zero-extent boxes, the
    // 1e-6 floor of the grid's extent)
    accel_checks(plain_scene(1, [](int, double *c) { c[0] = 1; c[1] = 2; c[2] = 3; c[3] = 0.5; }), cam, true, false);
    accel_checks(plain_scene(64, [](int, double *c) { c[0] = c[1] = c[2] = 0.25; c[3] = 0.5; }), cam, true, false);
    // 100 small spheres and 9 big ones: more than kTileBigMax, no big table
    accel_checks(plain_scene(109, [](int i, double *c) {
      const bool big = i % 12 == 0;  // 0, 12, .. 96: nine of them
      c[0] = big ? 3.0 * i - 140 : 0.7 * (i % 10) - 3;
      c[1] = big ? 10 : 0.1;
      c[2] = big ? 40 - i : 0.7 * (i / 10) - 3;
      c[3] = big ? 10 : 0.1;
    }), cam, true, true);
    // 70 000 spheres: over the grid's 65 535 (16-bit references), the BVH alone
    accel_checks(plain_scene(70000, [](int i, double *c) {
      c[0] = 0.5 * (i % 300); c[1] = 0.2 * ((i * 7) % 11); c[2] = 0.5 * (i / 300); c[3] = 0.2;
    }), cam, false, false);
    // refused arguments
    CHECK(rt_scene_random(1, g.data(), k.data(), m.data(), 600, &n) == 0);
    rt_scene fin{n, g.data(), k.data(), m.data()};
    int32_t n3[3] = {20, 1, 20}, dims[3], idx[32 * 8], cnt[8];
    uint32_t st[2];
    uint64_t dg[8];
    CHECK(rt_debug_grid_strides(n3, st) == 0 && st[0] == 80 && st[1] == 80);
    CHECK(rt_debug_grid_strides(nullptr, st) != 0 && rt_debug_grid_strides(n3, nullptr) != 0);
    n3[1] = 65536;
    CHECK(rt_debug_grid_strides(n3, st) != 0);
    n3[0] = 4096; n3[1] = 1024;
    CHECK(rt_debug_grid_strides(n3, st) != 0);
    rt_scene none = fin, empty = fin;
    none.center_radius = nullptr;
    empty.n = 0;
    CHECK(rt_debug_grid_layout(nullptr, dims, st, nullptr) != 0 && rt_debug_grid_layout(&none, dims, st, nullptr) != 0);
    CHECK(rt_debug_grid_layout(&empty, dims, st, nullptr) != 0 && rt_debug_grid_layout(&fin, nullptr, st, nullptr) != 0);
    CHECK(rt_debug_grid_layout(&fin, dims, nullptr, nullptr) != 0);
    CHECK(rt_debug_accel_digest(nullptr, dg) != 0 && rt_debug_accel_digest(&fin, nullptr) != 0);
    CHECK(rt_debug_accel_digest(&none, dg) != 0 && rt_debug_accel_digest(&empty, dg) != 0);
    k[3] = 7;  // an unknown material kind
    CHECK(rt_debug_accel_digest(&fin, dg) != 0);
    k[3] = 0;
    auto list = [&](const rt_scene *s, const rt_camera *c, int W, int H, int row0, int step, int rows, int tw, int tile,
                    int cap) { return rt_debug_tile_list(s, c, W, H, row0, step, rows, tw, tile, cap, idx, cnt); };
    auto big = [&](const rt_scene *s, const rt_camera *c, int W, int H, int row0, int step, int rows, int tw, int tile) {
      return rt_debug_tile_big(s, c, W, H, row0, step, rows, tw, tile, idx, cnt);
    };
    CHECK(list(&fin, &cam, 16, 8, 0, 1, 8, 0, 0, 32) == 0 && big(&fin, &cam, 16, 8, 0, 1, 8, 0, 0) == 0);
    CHECK(list(nullptr, &cam, 16, 8, 0, 1, 8, 0, 0, 32) != 0 && big(nullptr, &cam, 16, 8, 0, 1, 8, 0, 0) != 0);
    CHECK(list(&fin, nullptr, 16, 8, 0, 1, 8, 0, 0, 32) != 0 && big(&fin, nullptr, 16, 8, 0, 1, 8, 0, 0) != 0);
    CHECK(list(&none, &cam, 16, 8, 0, 1, 8, 0, 0, 32) != 0 && big(&empty, &cam, 16, 8, 0, 1, 8, 0, 0) != 0);
    CHECK(rt_debug_tile_list(&fin, &cam, 16, 8, 0, 1, 8, 0, 0, 32, nullptr, cnt) != 0);
    CHECK(rt_debug_tile_big(&fin, &cam, 16, 8, 0, 1, 8, 0, 0, idx, nullptr) != 0);
    CHECK(list(&fin, &cam, 1, 8, 0, 1, 8, 0, 0, 32) != 0 && big(&fin, &cam, 16, 1, 0, 1, 8, 0, 0) != 0);    // image
    CHECK(list(&fin, &cam, 16, 8, -1, 1, 8, 0, 0, 32) != 0 && big(&fin, &cam, 16, 8, 8, 1, 8, 0, 0) != 0);   // row0
    CHECK(list(&fin, &cam, 16, 8, 0, 0, 8, 0, 0, 32) != 0 && big(&fin, &cam, 16, 8, 0, 1, 0, 0, 0) != 0);    // step, rows
    CHECK(list(&fin, &cam, 16, 8, 0, 1, 8, 12, 0, 32) != 0 && big(&fin, &cam, 16, 8, 0, 1, 8, 128, 0) != 0); // tile shape
    CHECK(list(&fin, &cam, 16, 8, 0, 1, 8, 0, 0, 0) != 0 && list(&fin, &cam, 16, 8, 0, 1, 8, 0, 0, 33) != 0); // cap
    CHECK(list(&fin, &cam, 16, 8, 0, 1, 8, 0, -2, 32) != 0 && big(&fin, &cam, 16, 8, 0, 1, 8, 0, 2) != 0);   // tile
  }
  std::vector<float> u(3000);
  CHECK(rt_nw_xorwow_uniforms(1984, 3000, u.data()) == 0);
  for (float x : u) CHECK(x > 0.0f && x <= 1.0f);
  if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
  else std::printf("host_sanitize: all checks passed\n");
  return failures ? 1 : 0;
}
