// nw_mesh_sanitize.cpp — stand-alone driver of tests/test_nw_mesh.py's
// sanitizer run: the triangle / mesh builders and the Wavefront OBJ reader of
// rtmi_nw_scene.cpp under ASan + UBSan (host code only, no device).
//   nw_mesh_sanitize DIR   (DIR holds cube.obj; scratch files are written there)
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

  // the reader: a valid file (quads, negative indices, CR LF)
  int32_t n = 0;
  const int cube = rt_nw_load_obj(s, (dir + "/cube.obj").c_str(), mat, &n);
  CHECK(cube >= 0 && n == 12);
  CHECK(rt_nw_world_add(s, cube) == RT_OK);
  // ... and malformed ones: each refused, nothing read out of bounds
  const char *bad[] = {
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "v 0 0\n", "v 1 2 z\n", "f\n",
      "f 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/ 2/ 3/\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\n",
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 99999999999999999999 1 2\n",
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3 //\n", "v 1e999 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", "vn\nv\nf", "\n\n\n",
      "v 0 0 0\nv 1 0 0\nv 1 0 0\nf 1 2 3"};
  for (const char *text : bad) {
    const std::string path = write_file(dir, "bad.obj", text);
    CHECK(rt_nw_load_obj(s, path.c_str(), mat, &n) == RT_EINVAL);
    CHECK(std::strlen(rt_last_error()) > 0);
  }
  {  // bytes that are not text, a NUL among them, no final newline
    std::string blob = "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1\0002 3";
    blob += std::string("\xff\xfe\x80 1 2", 7);
    const std::string path = write_file(dir, "blob.obj", blob);
    CHECK(rt_nw_load_obj(s, path.c_str(), mat, &n) == RT_EINVAL);
  }
  {  // a long line and a many-cornered polygon
    std::string text;
    const int corners = 5000;
    for (int k = 0; k < corners; ++k)
      text += "v " + std::to_string(std::cos(6.283185307179586 * k / corners)) + " " +
              std::to_string(std::sin(6.283185307179586 * k / corners)) + " 0\n";
    text += "f";
    for (int k = 1; k <= corners; ++k) text += " " + std::to_string(k);
    const std::string path = write_file(dir, "fan.obj", text);
    const int fan = rt_nw_load_obj(s, path.c_str(), mat, &n);
    CHECK(fan >= 0 && n == corners - 2);
  }
  CHECK(rt_nw_load_obj(s, (dir + "/missing.obj").c_str(), mat, &n) == RT_EIO);
  CHECK(rt_nw_load_obj(s, nullptr, mat, &n) == RT_EINVAL);
  CHECK(rt_nw_load_obj(s, (dir + "/cube.obj").c_str(), 12345, nullptr) == RT_EINVAL);

  // meshes from arrays: indices at and past the ends
  const double v[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double nrm[6] = {0, 0, 1, 0, 0, -1};
  const int32_t ok[6] = {0, 1, 2, 1, 2, 3}, past[3] = {0, 1, 4}, neg[3] = {0, -1, 2}, nbad[6] = {0, 0, 2, 0, 0, 0},
                nok[6] = {0, 0, 0, 1, 1, 1};
  CHECK(rt_nw_mesh(s, v, 4, past, 1, nullptr, 0, nullptr, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh(s, v, 4, neg, 1, nullptr, 0, nullptr, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh(s, v, 4, ok, 2, nrm, 2, nbad, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh(s, v, 4, ok, 2, nrm, 2, nullptr, mat) == RT_EINVAL);  // per-vertex normals: only two given
  CHECK(rt_nw_mesh(s, v, 4, ok, 2, nullptr, 0, nok, mat) == RT_EINVAL);
  CHECK(rt_nw_mesh(s, v, 4, ok, 0, nullptr, 0, nullptr, mat) == RT_EINVAL);
  const int mesh = rt_nw_mesh(s, v, 4, ok, 2, nrm, 2, nok, mat);
  CHECK(mesh >= 0);
  const double off[3] = {3, 0, 0};
  CHECK(rt_nw_world_add(s, rt_nw_translate(s, rt_nw_rotate_y(s, mesh, 40), off)) == RT_OK);
  const double nanv[3] = {0, NAN, 0};
  CHECK(rt_nw_triangle(s, v, v + 3, nanv, mat) == RT_EINVAL);
  CHECK(rt_nw_triangle(s, v, v, v + 3, mat) == RT_EINVAL);
  CHECK(rt_nw_triangle(s, v, v + 3, nullptr, mat) == RT_EINVAL);
  const int tri = rt_nw_triangle(s, v, v + 3, v + 6, mat);
  CHECK(tri >= 0);
  CHECK(rt_nw_constant_medium(s, tri, 0.1, 0) == RT_EUNSUPPORTED);

  rt_nw_flat fl;
  CHECK(rt_nw_scene_flat(s, &fl) == RT_OK);
  CHECK(fl.n_obj == 12 + 2 && fl.n_inst == 1);
  double sum = 0;
  for (int k = 0; k < fl.n_obj * 16; ++k) sum += std::isfinite(fl.obj[k]) ? 1 : 0;  // every float read
  CHECK(sum > 0);
  int32_t dims[3], mc, nb, nr;
  CHECK(rt_nw_scene_grid_stats(s, dims, &mc, &nb, &nr) == RT_OK);
  CHECK(rt_nw_scene_destroy(s) == RT_OK);
  std::printf("all checks passed\n");
  return 0;
}
