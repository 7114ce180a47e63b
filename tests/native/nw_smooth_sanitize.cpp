// nw_smooth_sanitize.cpp — stand-alone driver of tests/test_nw_smooth.py's
// sanitizer run: the attribute mesh builder (rt_nw_mesh_attr), the OBJ
// reader's vt / t handling (rt_nw_load_obj_attr, rt_nw_scene_obj_stage_attr)
// and rt_nw_scene_flat_attr of rtmi_nw_scene.cpp under ASan + UBSan (host code
// only, no device).
//   nw_smooth_sanitize DIR   (DIR holds cube.obj; scratch files are written there)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtmi_nw.h"

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "%s:%d: check failed: %s (%s)\n", __FILE__, __LINE__, #cond, rt_last_error()); \
      std::exit(1);                                                                      \
    }                                                                                    \
  } while (0)

static std::string write_file(const std::string &dir, const char *name, const std::string &text) {
  const std::string path = dir + "/" + name;
  FILE *f = std::fopen(path.c_str(), "wb");
  CHECK(f != nullptr);
  std::fwrite(text.data(), 1, text.size(), f);
  std::fclose(f);
  return path;
}

int main(int argc, char **argv) {
  CHECK(argc == 2);
  const std::string dir = argv[1];
  rt_nw_scene *s = nullptr;
  CHECK(rt_nw_scene_create(&s) == RT_OK);
  const int mat = rt_nw_mat_lambertian(s, rt_nw_tex_solid(s, 0.5, 0.5, 0.5));
  CHECK(mat >= 0);
  const uint32_t ALL = RT_NW_MESH_SMOOTH | RT_NW_MESH_UV | RT_NW_MESH_GEN_NORMALS;

  // meshes from arrays: every array read to its end, indices at and past the ends
  const double v[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double nrm[12] = {0, 0, 1, 0, 0.1, 1, 0.1, 0, 1, 0, 0, 1};
  const double uv[8] = {0, 0, 1, 0, 0, 1, 1, 1};
  const int32_t ok[6] = {0, 1, 2, 1, 2, 3}, past[6] = {0, 1, 2, 1, 2, 4}, neg[6] = {0, 1, 2, 1, -1, 3};
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, uv, 4, nullptr, ALL, mat) >= 0);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, ok, uv, 4, ok, RT_NW_MESH_SMOOTH | RT_NW_MESH_UV, mat) >= 0);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nullptr, 0, nullptr, nullptr, 0, nullptr, RT_NW_MESH_SMOOTH | RT_NW_MESH_GEN_NORMALS, mat) >= 0);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, mat) >= 0);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, uv, 3, nullptr, ALL, mat) == RT_EINVAL);   // vertex 3 has no uv
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, uv, 4, past, ALL, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, uv, 4, neg, ALL, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, past, uv, 4, nullptr, ALL, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, past, 2, nrm, 4, nullptr, uv, 4, nullptr, ALL, mat) == RT_EINVAL);  // (the generated sums skip it)
  CHECK(rt_nw_mesh_attr(s, v, 4, neg, 2, nullptr, 0, nullptr, nullptr, 0, nullptr, ALL & ~RT_NW_MESH_UV, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, nullptr, 0, nullptr, RT_NW_MESH_UV, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, nullptr, 0, ok, 0, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nrm, 4, nullptr, uv, 4, nullptr, 64, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(s, v, 4, ok, 0, nrm, 4, nullptr, uv, 4, nullptr, ALL, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh_attr(nullptr, v, 4, ok, 2, nrm, 4, nullptr, uv, 4, nullptr, ALL, mat) == RT_EINVAL);
  {
    double bad[12];
    std::memcpy(bad, nrm, sizeof bad);
    bad[3] = bad[4] = bad[5] = 0;  // zero length
    CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, bad, 4, nullptr, nullptr, 0, nullptr, RT_NW_MESH_SMOOTH, mat) == RT_EINVAL);
    bad[4] = NAN;
    CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, bad, 4, nullptr, nullptr, 0, nullptr, RT_NW_MESH_SMOOTH, mat) == RT_EINVAL);
    bad[4] = 1e300;  // finite as a double only
    CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, bad, 4, nullptr, nullptr, 0, nullptr, RT_NW_MESH_SMOOTH, mat) == RT_EINVAL);
    bad[4] = 1e-300;  // zero as a float, a direction in double
    CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, bad, 4, nullptr, nullptr, 0, nullptr, RT_NW_MESH_SMOOTH, mat) >= 0);
    double buv[8];
    std::memcpy(buv, uv, sizeof buv);
    buv[7] = INFINITY;
    CHECK(rt_nw_mesh_attr(s, v, 4, ok, 2, nullptr, 0, nullptr, buv, 4, nullptr, RT_NW_MESH_UV, mat) == RT_EINVAL);
  }

  // the reader: a valid file (quads, negative indices, CR LF, a/t/n)
  int32_t n = 0;
  const std::string cube_path = dir + "/cube.obj";
  const int cube = rt_nw_load_obj_attr(s, cube_path.c_str(), mat, ALL, &n);
  CHECK(cube >= 0 && n == 12);
  CHECK(rt_nw_world_add(s, cube) == RT_OK);
  CHECK(rt_nw_load_obj_attr(s, cube_path.c_str(), mat, 0, &n) >= 0 && n == 12);
  CHECK(rt_nw_load_obj_attr(s, cube_path.c_str(), mat, 64, &n) == RT_EINVAL);
  CHECK(rt_nw_load_obj_attr(s, nullptr, mat, ALL, &n) == RT_EINVAL);
  CHECK(rt_nw_load_obj_attr(s, (dir + "/missing.obj").c_str(), mat, ALL, &n) == RT_EIO);
  const std::string tri = "v 0 0 0\nv 1 0 0\nv 0 1 0\n";
  const char *good[] = {"vt 0.5\nf 1/1 2/1 3/1\n", "vt 0.5 0.5 0.5\nf 1/-1 2/-1 3/-1", "vt 1 1\nf 1/1 2 3/1\n", "f 1 2 3\nvt",
                        "vt 0 0\nvn 0 0 -1\nf 1/1/1 2/1/1 3/1/1\n"};
  for (int k = 0; k < 5; ++k) {
    const std::string path = write_file(dir, "good.obj", tri + good[k]);
    const bool vt_last = k == 3;  // a bare "vt" is malformed under UV only
    CHECK((rt_nw_load_obj_attr(s, path.c_str(), mat, ALL, &n) >= 0) == !vt_last);
    CHECK(rt_nw_load_obj_attr(s, path.c_str(), mat, RT_NW_MESH_SMOOTH, &n) >= 0 && n == 1);
    CHECK(rt_nw_load_obj(s, path.c_str(), mat, &n) >= 0 && n == 1);
  }
  const char *bad[] = {"vt\nf 1 2 3\n", "vt x\nf 1 2 3\n", "vt 1 2 3 4\nf 1 2 3\n", "vt 0 0\nf 1/2 2/1 3/1\n", "vt 0 0\nf 1/0 2/1 3/1\n",
                       "vt 0 0\nf 1/-2 2/1 3/1\n", "f 1/1 2/1 3/1\nvt 0 0\n", "vt 0 0\nf 1/99999999999999999999 2/1 3/1\n",
                       "vt 1e999 0\nf 1/1 2/1 3/1\n", "vt 0 0\nf 1/1/ 2/1 3/1\n", "vt 0 0\nf 1/1x 2/1 3/1\n"};
  for (const char *text : bad) {
    const std::string path = write_file(dir, "bad.obj", tri + text);
    CHECK(rt_nw_load_obj_attr(s, path.c_str(), mat, RT_NW_MESH_UV, &n) == RT_EINVAL);
    CHECK(std::strstr(rt_last_error(), "line ") != nullptr);
  }
  {  // many vt on a many-cornered polygon
    std::string text;
    const int corners = 3000;
    for (int k = 0; k < corners; ++k) {
      const double a = 6.283185307179586 * k / corners;
      text += "v " + std::to_string(std::cos(a)) + " " + std::to_string(std::sin(a)) + " 0\n";
      text += "vt " + std::to_string(0.5 + 0.5 * std::cos(a)) + " " + std::to_string(0.5 + 0.5 * std::sin(a)) + "\n";
    }
    text += "f";
    for (int k = 1; k <= corners; ++k) text += " " + std::to_string(k) + "/" + std::to_string(k - corners - 1);
    const std::string path = write_file(dir, "fan.obj", text);
    const int fan = rt_nw_load_obj_attr(s, path.c_str(), mat, ALL, &n);
    CHECK(fan >= 0 && n == corners - 2);
    const double off[3] = {3, 0, 0};
    CHECK(rt_nw_world_add(s, rt_nw_translate(s, rt_nw_rotate_y(s, fan, 40), off)) == RT_OK);
  }

  rt_nw_flat fl;
  CHECK(rt_nw_scene_flat(s, &fl) == RT_OK);
  int32_t n_attr = 0;
  const float *attr = nullptr;
  const int32_t *of = nullptr;
  CHECK(rt_nw_scene_flat_attr(s, &n_attr, &attr, &of) == RT_OK);
  CHECK(rt_nw_scene_flat_attr(s, nullptr, &attr, &of) == RT_EINVAL);
  CHECK(fl.n_obj == 12 + 2998 && n_attr > fl.n_obj);
  double sum = 0;
  for (int k = 0; k < n_attr * 16; ++k) sum += std::isfinite(attr[k]) ? 1 : 0;  // every float read
  for (int k = 0; k < fl.n_obj; ++k) {
    CHECK(of[k] >= 0 && of[k] < n_attr);
    sum += of[k];
  }
  CHECK(sum > 0);
  int32_t dims[3], mc, nb, nr;
  CHECK(rt_nw_scene_grid_stats(s, dims, &mc, &nb, &nr) == RT_OK);
  CHECK(rt_nw_scene_destroy(s) == RT_OK);

  // the stage: with and without an image, the refusals
  const uint8_t px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
  rt_nw_camera cam;
  for (int kind : {RT_NW_LAMBERTIAN, RT_NW_METAL}) {
    CHECK(rt_nw_scene_create(&s) == RT_OK);
    CHECK(rt_nw_scene_obj_stage_attr(s, cube_path.c_str(), kind, ALL, px, 2, 2, 1.5, &cam, &n) == RT_OK && n == 12);
    CHECK(rt_nw_scene_flat_attr(s, &n_attr, &attr, &of) == RT_OK && n_attr == 12);
    CHECK(rt_nw_scene_destroy(s) == RT_OK);
  }
  CHECK(rt_nw_scene_create(&s) == RT_OK);
  CHECK(rt_nw_scene_obj_stage_attr(s, cube_path.c_str(), RT_NW_DIELECTRIC, ALL, px, 2, 2, 1.5, &cam, &n) == RT_EINVAL);
  CHECK(rt_nw_scene_obj_stage_attr(s, cube_path.c_str(), RT_NW_METAL, ALL, px, 0, 2, 1.5, &cam, &n) == RT_EINVAL);
  CHECK(rt_nw_scene_obj_stage_attr(s, cube_path.c_str(), RT_NW_METAL, 64, nullptr, 0, 0, 1.5, &cam, &n) == RT_EINVAL);
  CHECK(rt_nw_scene_obj_stage_attr(s, cube_path.c_str(), RT_NW_DIELECTRIC, RT_NW_MESH_SMOOTH, nullptr, 0, 0, 1.5, &cam, &n) == RT_OK);
  CHECK(rt_nw_scene_destroy(s) == RT_OK);
  std::printf("all checks passed\n");
  return 0;
}
