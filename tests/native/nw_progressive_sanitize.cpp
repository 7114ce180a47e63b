// nw_progressive_sanitize.cpp — stand-alone driver of tests/test_nw_progressive.py's
// sanitizer run: rt_nw_scene_hash and the checkpoint header code of the
// progressive accumulator (rtmi_nw_scene.cpp: ckpt_write, ckpt_read,
// rt_nw_accum_info) under ASan + UBSan (host code only, no device).
//  - three small scenes — a flat mesh, a moving placement, an affine placement
//    of a shared mesh — hash to the same value when built twice, to different
//    values from each other and after one changed offset, and the hash leaves a
//    flat view taken at another time as it was;
//  - checkpoint files written and read back: header and sums return; files cut
//    inside the header, cut inside the body, longer than their header states,
//    with a header that states more than any file holds, with another magic or
//    missing are RT_EIO, and nothing is read or allocated out of bounds;
//  - everything is destroyed (leaks are errors).
//   nw_progressive_sanitize DIRECTORY
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

// an octahedron about (0, 1, 0)
static const double kVerts[18] = {1, 1, 0, -1, 1, 0, 0, 2, 0, 0, 0, 0, 0, 1, 1, 0, 1, -1};
static const int32_t kTris[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};

// kind 0: the mesh flattened; 1: shared, under a move to (dx, 0.5, 0); 2: shared, under a transform with offset dx
static rt_nw_scene *build(int kind, double dx) {
  rt_nw_scene *s = nullptr;
  CHECK(rt_nw_scene_create(&s) == RT_OK);
  const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.6, 0.5, 0.4));
  CHECK(mat >= 0);
  const int mesh = rt_nw_mesh(s, kVerts, 6, kTris, 8, nullptr, 0, nullptr, mat);
  CHECK(mesh >= 0);
  int top = mesh;
  if (kind == 1) {
    const double o0[3] = {0, 0, 0}, o1[3] = {dx, 0.5, 0};
    top = rt_nw_move(s, rt_nw_rotate_y(s, rt_nw_shared(s, mesh), 30.0), o0, o1, 0.0, 1.0);
  } else if (kind == 2) {
    const double m[12] = {1.5, 0.2, 0, dx, 0, 0.8, 0, 0.25, 0, 0.1, 1.1, -0.5};
    top = rt_nw_transform(s, rt_nw_shared(s, mesh), m);
  }
  CHECK(top >= 0);
  CHECK(rt_nw_world_add(s, top) == RT_OK);
  const double c[3] = {0, -1000, 0};
  CHECK(rt_nw_world_add(s, rt_nw_sphere(s, c, 1000, mat)) == RT_OK);
  CHECK(rt_nw_set_background(s, 0.7, 0.8, 1.0) == RT_OK);
  return s;
}

static uint64_t hash_of(rt_nw_scene *s) {
  uint64_t h = 0, again = 0;
  CHECK(rt_nw_scene_hash(s, &h) == RT_OK);
  CHECK(rt_nw_scene_hash(s, &again) == RT_OK && again == h);
  return h;
}

static void write_bytes(const std::string &path, const void *p, size_t n) {
  FILE *f = std::fopen(path.c_str(), "wb");
  CHECK(f != nullptr);
  CHECK(n == 0 || std::fwrite(p, 1, n, f) == n);
  CHECK(std::fclose(f) == 0);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s DIRECTORY\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];

  // ---- hashes ----
  uint64_t h[3];
  for (int kind = 0; kind < 3; ++kind) {
    rt_nw_scene *a = build(kind, 0.75), *b = build(kind, 0.75), *c = build(kind, 0.75 + 1e-6);
    h[kind] = hash_of(a);
    CHECK(hash_of(b) == h[kind]);
    CHECK((hash_of(c) != h[kind]) == (kind != 0));  // (kind 0 does not use dx)
    if (kind == 1) {  // a flat view at another time survives the hash
      rt_nw_flat f0, f1;
      CHECK(rt_nw_scene_flat_at(a, 0.5, &f0) == RT_OK);
      std::vector<float> inst(f0.inst, f0.inst + 8 * f0.n_inst);
      CHECK(hash_of(a) == h[kind]);
      CHECK(rt_nw_scene_flat_at(a, 0.5, &f1) == RT_OK);
      CHECK(f1.n_inst == f0.n_inst && std::memcmp(inst.data(), f1.inst, inst.size() * sizeof(float)) == 0);
      int32_t st[2];
      CHECK(rt_nw_scene_motion_stats(a, st) == RT_OK && st[0] == 1);
    }
    CHECK(rt_nw_scene_destroy(a) == RT_OK && rt_nw_scene_destroy(b) == RT_OK && rt_nw_scene_destroy(c) == RT_OK);
  }
  CHECK(h[0] != h[1] && h[1] != h[2] && h[0] != h[2]);
  uint64_t out = 0;
  CHECK(rt_nw_scene_hash(nullptr, &out) == RT_EINVAL);

  // ---- checkpoint files ----
  const int W = 5, nrows = 3;
  std::vector<int64_t> raw(size_t(W) * nrows * 3);
  for (size_t i = 0; i < raw.size(); ++i) raw[i] = int64_t(i) * 0x100000001ll - 7;
  CkptHeader hd{};
  hd.W = W; hd.H = 9; hd.row0 = 1; hd.row_step = 3; hd.nrows = nrows; hd.spp_done = 12; hd.max_depth = 50;
  hd.seed = 1984; hd.scene_hash = h[2]; hd.camera_hash = 0x0123456789abcdefull;
  const std::string good = dir + "/good.ckpt";
  CHECK(ckpt_write(good.c_str(), hd, raw.data()) == RT_OK);
  CkptHeader back{};
  std::vector<int64_t> body;
  CHECK(ckpt_read(good.c_str(), back, &body) == RT_OK);
  CHECK(std::memcmp(back.magic, "RTMINWA1", 8) == 0 && back.W == W && back.H == 9 && back.row0 == 1 && back.row_step == 3 &&
        back.nrows == nrows && back.spp_done == 12 && back.max_depth == 50 && back.zero == 0 && back.seed == 1984 &&
        back.scene_hash == h[2] && back.camera_hash == 0x0123456789abcdefull);
  CHECK(body == raw);
  int32_t v8[8];
  uint64_t v3[3];
  CHECK(rt_nw_accum_info(good.c_str(), v8, v3) == RT_OK && v8[0] == W && v8[4] == nrows && v8[5] == 12 && v3[1] == h[2]);
  CHECK(rt_nw_accum_info(nullptr, v8, v3) == RT_EINVAL && rt_nw_accum_info(good.c_str(), nullptr, v3) == RT_EINVAL &&
        rt_nw_accum_info(good.c_str(), v8, nullptr) == RT_EINVAL);
  {  // the temporary file is gone
    FILE *f = std::fopen((good + ".tmp").c_str(), "rb");
    CHECK(f == nullptr);
  }

  std::vector<unsigned char> bytes(sizeof(CkptHeader) + raw.size() * sizeof(int64_t));
  std::memcpy(bytes.data(), &back, sizeof back);
  std::memcpy(bytes.data() + sizeof back, raw.data(), raw.size() * sizeof(int64_t));
  const std::string bad = dir + "/bad.ckpt";
  // cut inside the header: nothing of it is a checkpoint
  for (size_t n : {size_t(0), size_t(7), size_t(8), size_t(63)}) {
    write_bytes(bad, bytes.data(), n);
    CHECK(ckpt_read(bad.c_str(), back, nullptr) == RT_EIO && ckpt_read(bad.c_str(), back, &body) == RT_EIO);
    CHECK(rt_nw_accum_info(bad.c_str(), v8, v3) == RT_EIO);
  }
  // the header alone, a body cut short, one byte short, one byte long
  for (size_t n : {sizeof(CkptHeader), sizeof(CkptHeader) + 8, bytes.size() - 1}) {
    write_bytes(bad, bytes.data(), n);
    CHECK(ckpt_read(bad.c_str(), back, nullptr) == RT_OK && back.spp_done == 12);
    CHECK(ckpt_read(bad.c_str(), back, &body) == RT_EIO);
  }
  {
    std::vector<unsigned char> longer = bytes;
    longer.push_back(0);
    write_bytes(bad, longer.data(), longer.size());
    CHECK(ckpt_read(bad.c_str(), back, &body) == RT_EIO);
  }
  // headers that state more than any file holds, or nonsense: refused before anything is allocated
  for (int k = 0; k < 4; ++k) {
    CkptHeader big = hd;
    std::memcpy(big.magic, "RTMINWA1", 8);
    if (k == 0) { big.W = 0x7fffffff; big.nrows = 0x7fffffff; }
    if (k == 1) { big.W = 1 << 20; big.nrows = 1 << 19; }
    if (k == 2) big.W = -5;
    if (k == 3) big.nrows = -1;
    std::vector<unsigned char> b2 = bytes;
    std::memcpy(b2.data(), &big, sizeof big);
    write_bytes(bad, b2.data(), b2.size());
    CHECK(ckpt_read(bad.c_str(), back, nullptr) == RT_OK);
    CHECK(ckpt_read(bad.c_str(), back, &body) == RT_EIO);
  }
  // another magic (the One-Weekend file's among them), a missing file
  for (const char *magic : {"RTMIACC1", "RTMINWA2", "P6\n1 1\n2"}) {
    std::vector<unsigned char> b2 = bytes;
    std::memcpy(b2.data(), magic, 8);
    write_bytes(bad, b2.data(), b2.size());
    CHECK(ckpt_read(bad.c_str(), back, &body) == RT_EIO && rt_nw_accum_info(bad.c_str(), v8, v3) == RT_EIO);
  }
  CHECK(ckpt_read((dir + "/none.ckpt").c_str(), back, &body) == RT_EIO);
  CHECK(ckpt_write((dir + "/no/such/dir.ckpt").c_str(), hd, raw.data()) == RT_EIO);
  // an empty strip writes and reads a header alone
  hd.nrows = 0;
  CHECK(ckpt_write(bad.c_str(), hd, raw.data()) == RT_OK && ckpt_read(bad.c_str(), back, &body) == RT_OK && body.empty());
  std::remove(bad.c_str());
  std::remove(good.c_str());
  std::printf("all checks passed\n");
  return 0;
}
