// rtmi_nw_cli.cpp — rtmi_nw_render, the Next-Week host driver: the reference's
// rt_next_week/cuda/main.cu main() (main.cu:492-600) with create_world's
// scene switch as a flag and the render on librtmi (C ABI only).  Defaults
// are the reference's constants: scene 8 (the final scene, `switch (0)` falls
// to `default: case 8`), 800x800, 5000 spp, depth 50.
//
//   rtmi_nw_render [--scene 1..8|final|cornell_box|...] [--width W] [--height H]
//                  [--spp S] [--depth D] [--seed N] [--texture FILE.ppm]
//                  [--out FILE|-] [--p6] [--rtl]
//   rtmi_nw_render --obj FILE.obj [--obj-mat lambertian|metal|glass] [--obj-smooth] [--obj-gen-normals]
//                  [--obj-texture FILE.ppm] [--obj-copies N] [--obj-move DX,DY,DZ] [--obj-tumble] [--width W] ...
//   either form: [--shutter T0,T1] [--pass-spp N] [--checkpoint FILE] [--time-limit SECONDS] [--pfm FILE]
//                [--adaptive THRESHOLD [--min-spp N] [--spp-map FILE.pfm]]
//                [--denoise [--denoise-iters N] [--features-spp N]] [--aov PREFIX]
//
// --denoise writes the filtered image (rt_nw_render_denoised: first-hit features
// of --features-spp samples per pixel, default 16, the variance of the adaptive
// accumulator and --denoise-iters a-trous levels, default 5) to --out / --pfm.
// The variance needs the second moments, so without --adaptive the render goes
// through the adaptive accumulator with every pixel active (threshold 0: the
// plain render of --spp samples, in passes of --pass-spp, default kDefaultPassSpp).
// --aov PREFIX writes PREFIX_albedo.pfm, PREFIX_normal.pfm, PREFIX_depth.pfm (the
// depth in all three channels) and, with --denoise, PREFIX_noisy.pfm.
//
// --adaptive THRESHOLD samples every pixel until the relative standard error of
// its mean (rt_nw_adapt_criterion, floor 0.03, dilation 1) is at most THRESHOLD
// (rt_nw_render_adaptive): at least --min-spp samples (default 16), at most
// --spp, in passes of --pass-spp (default kDefaultAdaptPassSpp) over the pixels
// still active.  --checkpoint (an adaptive checkpoint, rt_nw_adapt_save),
// --time-limit, --out and --pfm work as above; --spp-map FILE.pfm writes the
// per-pixel sample counts (the count in all three channels).  stderr carries
// the total samples and the share of pixels at the maximum.
//
// --pass-spp N renders in passes of N samples (rt_nw_render_pass), each a
// bounded kernel launch; the image is bit for bit the one of a single render of
// --spp samples.  --checkpoint FILE saves the accumulator after every pass
// (rt_nw_accum_save) and resumes from the file when it exists: a second run
// with a larger --spp continues where the first ended.  --time-limit SECONDS
// starts no new pass once that much time has passed since the first one began
// (at least one pass always runs); the run then saves, writes the image of the
// samples it has, reports their count and exits 0.  --checkpoint or
// --time-limit without --pass-spp: passes of kDefaultPassSpp.  stderr carries
// {"pass_done_spp": n} per pass.  --pfm FILE writes the mean image (floats).
//
// --obj (exclusive with --scene) renders a Wavefront OBJ mesh
// (rt_nw_scene_obj_stage): scaled and centred into the box [-1, 1] x [0, 2] x
// [-1, 1] on a checker ground, one 3 x 3 light of emission 6 at y = 5,
// background (0.05, 0.07, 0.12), camera from (3.2, 2.4, 4.8) at (0, 1, 0),
// vfov 30, no aperture.  --obj-smooth shades with the file's vn interpolated
// (--obj-gen-normals: area-weighted vertex normals where the file has none),
// --obj-texture maps a binary PPM (P6, read as --texture is) onto the mesh by
// the file's vt (lambertian or metal); none of the three is valid with --scene.
// --obj-copies N stages the model as one shared mesh (rt_nw_shared) placed
// N x N times on the ground (rt_nw_scene_obj_stage_copies; 1: the stage above).
// --obj-move DX,DY,DZ makes every placement move by that vector over the times
// [0, 1] (rt_nw_move, rt_nw_scene_obj_stage_moving; with one copy the model is
// one moving placement).  --obj-tumble makes every copy an affine placement
// (rt_nw_transform, rt_nw_scene_obj_stage_tumbled): scaled, turned about a skew
// axis and stood on the ground; it combines with --obj-move.  --shutter T0,T1 (0 <= T0 <= T1 <= 1) replaces the
// camera's shutter interval, [0, 1] in every scene here.
//
// --texture is the earth image as a binary PPM (P6; the reference decodes
// earthmap.jpeg with stb_image, main.cu:497-510 — convert it once, e.g. with
// PIL).  The P3 output follows main.cu:563-575: int(255.99 * sqrt(mean)) per
// channel, top row first, NOT clamped (lights print values above 255, as the
// reference does); --p6 clamps to bytes.  Timing goes to stderr as JSON.
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtmi_nw.h"

// Default --pass-spp.  Measured at 800 x 800 x 1024 against one rt_nw_render (profiles/progressive/README.md): the
// final scene in passes of 1024 / 256 / 64 / 16 samples costs -0.2 / +14 / +42 / +175 %, a 4 x 4 field of a
// 5 120-triangle mesh -0.1 / +5.5 / +25 / +121 % — a small pass gives the persistent kernels few, short work
// items.  1024 is free and still a pass of about a second on those scenes.
static const int kDefaultPassSpp = 1024;
// Default --pass-spp under --adaptive: the criterion is looked at after every pass, so a pass is the grain of the
// sample-count map; late passes hold few tiles and their work items shrink with them (the chunk rule takes the
// active tile count).
static const int kDefaultAdaptPassSpp = 64;

static int die(const char *what, int rc) {
  std::fprintf(stderr, "rtmi_nw_render: %s failed (%d): %s\n", what, rc, rt_last_error());
  return 1;
}

// binary PPM (P6, maxval 255) -> rgb bytes, row 0 at the top
static bool read_p6(const char *path, std::vector<uint8_t> &px, int &w, int &h) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  char magic[3] = {0};
  int maxv = 0;
  bool ok = std::fscanf(f, "%2s", magic) == 1 && !std::strcmp(magic, "P6");
  auto skip = [&] {  // whitespace and '#' comments between header fields
    int c;
    while ((c = std::fgetc(f)) != EOF) {
      if (c == '#') {
        while ((c = std::fgetc(f)) != EOF && c != '\n') {}
      } else if (!std::isspace(c)) {
        std::ungetc(c, f);
        return;
      }
    }
  };
  if (ok) { skip(); ok = std::fscanf(f, "%d", &w) == 1; }
  if (ok) { skip(); ok = std::fscanf(f, "%d", &h) == 1; }
  if (ok) { skip(); ok = std::fscanf(f, "%d", &maxv) == 1 && maxv == 255 && w > 0 && h > 0 && w <= 65536 && h <= 65536; }
  if (ok) ok = std::fgetc(f) != EOF;  // the single whitespace byte before the raster
  if (ok) {
    px.resize(size_t(w) * h * 3);
    ok = std::fread(px.data(), 1, px.size(), f) == px.size();
  }
  std::fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  std::string scene = "8", out = "-", texture, obj, obj_mat = "lambertian", obj_texture, checkpoint, pfm, spp_map;
  int pass_spp = 0, min_spp = 16;
  double time_limit = -1, adaptive = -1;
  bool min_given = false, denoise = false;
  int denoise_iters = 5, features_spp = 16;
  std::string aov;
  bool scene_given = false, obj_smooth = false, obj_gen = false;
  int W = 800, H = -1, spp = 5000, depth = 50, p6 = 0, rtl = 0, obj_copies = 1;
  bool copies_given = false, move_given = false, shutter_given = false, tumble = false;
  double obj_move[3] = {0, 0, 0}, shutter[2] = {0, 1};
  // "a,b[,c]": exactly n finite numbers separated by commas
  auto numbers = [](const char *txt, double *out, int n) {
    for (int k = 0; k < n; ++k) {
      char *end = nullptr;
      out[k] = std::strtod(txt, &end);
      if (end == txt || !std::isfinite(out[k]) || *end != (k + 1 < n ? ',' : '\0')) return false;
      txt = end + 1;
    }
    return true;
  };
  unsigned long long seed = 1984;
  for (int a = 1; a < argc; a++) {
    auto need = [&](const char *f) -> const char * {
      if (a + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", f); std::exit(2); }
      return argv[++a];
    };
    if (!std::strcmp(argv[a], "--scene")) { scene = need("--scene"); scene_given = true; }
    else if (!std::strcmp(argv[a], "--obj")) obj = need("--obj");
    else if (!std::strcmp(argv[a], "--obj-mat")) obj_mat = need("--obj-mat");
    else if (!std::strcmp(argv[a], "--obj-smooth")) obj_smooth = true;
    else if (!std::strcmp(argv[a], "--obj-gen-normals")) obj_gen = true;
    else if (!std::strcmp(argv[a], "--obj-texture")) obj_texture = need("--obj-texture");
    else if (!std::strcmp(argv[a], "--obj-copies")) { obj_copies = std::atoi(need("--obj-copies")); copies_given = true; }
    else if (!std::strcmp(argv[a], "--obj-move")) {
      move_given = true;
      if (!numbers(need("--obj-move"), obj_move, 3)) { std::fprintf(stderr, "--obj-move takes DX,DY,DZ\n"); return 2; }
    } else if (!std::strcmp(argv[a], "--shutter")) {
      shutter_given = true;
      if (!numbers(need("--shutter"), shutter, 2) || !(shutter[0] >= 0 && shutter[0] <= shutter[1] && shutter[1] <= 1)) {
        std::fprintf(stderr, "--shutter takes T0,T1 with 0 <= T0 <= T1 <= 1\n");
        return 2;
      }
    }
    else if (!std::strcmp(argv[a], "--obj-tumble")) tumble = true;
    else if (!std::strcmp(argv[a], "--width")) W = std::atoi(need("--width"));
    else if (!std::strcmp(argv[a], "--height")) H = std::atoi(need("--height"));
    else if (!std::strcmp(argv[a], "--spp")) spp = std::atoi(need("--spp"));
    else if (!std::strcmp(argv[a], "--depth")) depth = std::atoi(need("--depth"));
    else if (!std::strcmp(argv[a], "--seed")) seed = std::strtoull(need("--seed"), nullptr, 10);
    else if (!std::strcmp(argv[a], "--texture")) texture = need("--texture");
    else if (!std::strcmp(argv[a], "--out")) out = need("--out");
    else if (!std::strcmp(argv[a], "--p6")) p6 = 1;
    else if (!std::strcmp(argv[a], "--rtl")) rtl = 1;
    else if (!std::strcmp(argv[a], "--pass-spp")) pass_spp = std::atoi(need("--pass-spp"));
    else if (!std::strcmp(argv[a], "--checkpoint")) checkpoint = need("--checkpoint");
    else if (!std::strcmp(argv[a], "--pfm")) pfm = need("--pfm");
    else if (!std::strcmp(argv[a], "--spp-map")) spp_map = need("--spp-map");
    else if (!std::strcmp(argv[a], "--min-spp")) { min_spp = std::atoi(need("--min-spp")); min_given = true; }
    else if (!std::strcmp(argv[a], "--denoise")) denoise = true;
    else if (!std::strcmp(argv[a], "--denoise-iters")) denoise_iters = std::atoi(need("--denoise-iters"));
    else if (!std::strcmp(argv[a], "--features-spp")) features_spp = std::atoi(need("--features-spp"));
    else if (!std::strcmp(argv[a], "--aov")) aov = need("--aov");
    else if (!std::strcmp(argv[a], "--adaptive")) {
      if (!numbers(need("--adaptive"), &adaptive, 1) || adaptive < 0) { std::fprintf(stderr, "--adaptive takes THRESHOLD >= 0\n"); return 2; }
    }
    else if (!std::strcmp(argv[a], "--time-limit")) {
      if (!numbers(need("--time-limit"), &time_limit, 1) || time_limit < 0) { std::fprintf(stderr, "--time-limit takes SECONDS >= 0\n"); return 2; }
    }
    else {
      std::fprintf(stderr, "usage: %s [--scene 1..8|name] [--width W] [--height H] [--spp S] [--depth D]\n"
                           "          [--seed N] [--texture FILE.ppm] [--out FILE|-] [--p6] [--rtl]\n"
                           "       %s --obj FILE.obj [--obj-mat lambertian|metal|glass] [--obj-smooth] [--obj-gen-normals]\n"
                           "          [--obj-texture FILE.ppm] [--obj-copies N] [--obj-move DX,DY,DZ] [--obj-tumble]\n"
                           "          [--width W] [--height H] ...\n"
                           "       either form: [--shutter T0,T1] (the camera's shutter, 0 <= T0 <= T1 <= 1; default 0,1)\n"
                           "                    [--pass-spp N] [--checkpoint FILE] [--time-limit SECONDS] [--pfm FILE]\n"
                           "  --pass-spp N: render in passes of N samples, the same image bit for bit; --checkpoint FILE: save\n"
                           "         after every pass and resume from FILE when it exists (a larger --spp continues a run);\n"
                           "         --time-limit SECONDS: start no new pass after that long (one always runs), then save, write\n"
                           "         the image of the samples so far and exit 0.  Without --pass-spp the last two use passes of\n"
                           "         %d samples.  Measured cost of splitting 1024 spp at 800 x 800 into passes of 1024 / 256 / 64 /\n"
                           "         16 samples: final scene -0.2 / +14 / +42 / +175 %%, a 4 x 4 mesh field -0.1 / +5.5 / +25 / +121 %%\n"
                           "  --pfm FILE: the mean image as floats\n"
                           "  --adaptive THRESHOLD [--min-spp N] [--spp-map FILE.pfm]: sample each pixel until the relative standard\n"
                           "         error of its mean is at most THRESHOLD, between --min-spp (default 16) and --spp samples, in\n"
                           "         passes of --pass-spp (default %d) over the pixels still active; --checkpoint, --time-limit,\n"
                           "         --out and --pfm as above; --spp-map: the per-pixel sample counts as a PFM\n"
                           "  --denoise [--denoise-iters N] [--features-spp N]: write the image filtered by the edge-avoiding a-trous\n"
                           "         wavelet (N levels, 1..8, default 5) guided by first-hit features of N samples per pixel (1..1024,\n"
                           "         default 16) and the per-pixel variance.  The variance needs the adaptive accumulator's second\n"
                           "         moments: without --adaptive the render goes through that accumulator with every pixel active\n"
                           "         (the plain render of --spp samples, --spp >= 2, in passes of --pass-spp, default %d)\n"
                           "  --aov PREFIX: PREFIX_albedo.pfm, PREFIX_normal.pfm, PREFIX_depth.pfm and, with --denoise, PREFIX_noisy.pfm\n"
                           "  --obj: the mesh scaled and centred into the box [-1,1] x [0,2] x [-1,1] on a checker\n"
                           "         ground, one 3 x 3 light (emission 6) at y = 5, background (0.05, 0.07, 0.12);\n"
                           "         camera from (3.2, 2.4, 4.8) at (0, 1, 0), vfov 30, no aperture; not with --scene\n"
                           "  --obj-smooth: interpolated vn (--obj-gen-normals: generated where missing);\n"
                           "  --obj-texture: a P6 image mapped by vt (lambertian, metal); all three need --obj\n"
                           "  --obj-copies N (1..256, needs --obj): the model as one shared mesh placed N x N times, 3 units\n"
                           "         apart, each copy turned and nudged by a fixed formula; the camera backs away with N\n"
                           "  --obj-move DX,DY,DZ (needs --obj): every placement of the model moves by that vector over the\n"
                           "         times [0, 1] (motion blur under the default shutter)\n"
                           "  --obj-tumble (needs --obj): every copy as an affine placement of the shared mesh, scaled by\n"
                           "         0.75 + 0.25 sin(2.9 q), turned 37 q degrees about a skew axis and stood on the ground\n",
                   argv[0], argv[0], kDefaultPassSpp, kDefaultAdaptPassSpp, kDefaultPassSpp);
      return 2;
    }
  }
  static const char *names[] = {"", "random", "two_spheres", "two_perlin_spheres", "earth", "simple_light",
                                "cornell_box", "cornell_smoke", "final"};
  int which = std::atoi(scene.c_str());
  for (int k = 1; k <= 8; ++k)
    if (scene == names[k]) which = k;
  if (!obj.empty() && scene_given) { std::fprintf(stderr, "--scene and --obj are exclusive\n"); return 2; }
  if (obj.empty() && (obj_smooth || obj_gen || !obj_texture.empty())) {
    std::fprintf(stderr, "--obj-smooth, --obj-gen-normals and --obj-texture need --obj (not valid with --scene)\n");
    return 2;
  }
  if (copies_given && (obj.empty() || obj_copies < 1 || obj_copies > 256)) {
    std::fprintf(stderr, "--obj-copies needs --obj and a count in 1..256\n");
    return 2;
  }
  if (tumble && obj.empty()) {
    std::fprintf(stderr, "--obj-tumble needs --obj\n");
    return 2;
  }
  if (move_given && obj.empty()) {
    std::fprintf(stderr, "--obj-move needs --obj\n");
    return 2;
  }
  const int obj_kind = obj_mat == "lambertian" ? RT_NW_LAMBERTIAN : obj_mat == "metal" ? RT_NW_METAL : obj_mat == "glass" ? RT_NW_DIELECTRIC : -1;
  if (obj_kind < 0) { std::fprintf(stderr, "unknown --obj-mat %s (lambertian, metal, glass)\n", obj_mat.c_str()); return 2; }
  if (obj.empty() && (which < 1 || which > 8)) { std::fprintf(stderr, "unknown scene %s\n", scene.c_str()); return 2; }
  if (!obj.empty()) which = 0;
  if (H < 0) H = W;  // aspect_ratio = 1.0, main.cu:517-519
  if (pass_spp < 0) { std::fprintf(stderr, "--pass-spp takes a count >= 1\n"); return 2; }
  if (adaptive < 0 && (min_given || !spp_map.empty())) { std::fprintf(stderr, "--min-spp and --spp-map need --adaptive\n"); return 2; }
  if (denoise && (denoise_iters < 1 || denoise_iters > 8 || features_spp < 1 || features_spp > 1024)) {
    std::fprintf(stderr, "--denoise-iters takes 1..8 and --features-spp 1..1024\n");
    return 2;
  }
  if (!aov.empty() && (features_spp < 1 || features_spp > 1024)) { std::fprintf(stderr, "--features-spp takes 1..1024\n"); return 2; }
  const bool all_active = denoise && adaptive < 0;  // the plain render through the adaptive accumulator
  if (all_active) {
    if (spp < 2) { std::fprintf(stderr, "--denoise needs --spp >= 2\n"); return 2; }
    if (pass_spp == 0) pass_spp = kDefaultPassSpp;
    adaptive = 0;
    min_spp = spp;
  }
  if (adaptive >= 0 && pass_spp == 0) pass_spp = kDefaultAdaptPassSpp;
  if (adaptive >= 0 && (min_spp < 0 || min_spp > spp || spp < 2)) { std::fprintf(stderr, "--adaptive needs 0 <= --min-spp <= --spp and --spp >= 2\n"); return 2; }
  if (pass_spp == 0 && (!checkpoint.empty() || time_limit >= 0)) pass_spp = kDefaultPassSpp;
  if (pass_spp > 0 && spp < 1) { std::fprintf(stderr, "--spp takes a count >= 1\n"); return 2; }
  std::vector<uint8_t> img;
  int iw = 0, ih = 0;
  if (!texture.empty() && !read_p6(texture.c_str(), img, iw, ih)) {
    std::fprintf(stderr, "cannot read P6 texture %s\n", texture.c_str());
    return 2;
  }

  std::vector<uint8_t> oimg;
  int ow = 0, oh = 0;
  if (!obj_texture.empty() && !read_p6(obj_texture.c_str(), oimg, ow, oh)) {
    std::fprintf(stderr, "cannot read P6 texture %s\n", obj_texture.c_str());
    return 2;
  }
  if (!oimg.empty() && obj_kind == RT_NW_DIELECTRIC) { std::fprintf(stderr, "--obj-texture needs --obj-mat lambertian or metal\n"); return 2; }

  rt_nw_scene *s = nullptr;
  rt_nw_camera cam;
  int rc;
  if ((rc = rt_nw_scene_create(&s))) return die("rt_nw_scene_create", rc);
  if (!obj.empty()) {
    const uint32_t flags = (obj_smooth ? RT_NW_MESH_SMOOTH : 0) | (obj_gen ? RT_NW_MESH_GEN_NORMALS : 0) | (oimg.empty() ? 0 : RT_NW_MESH_UV);
    if (tumble) {
      if ((rc = rt_nw_scene_obj_stage_tumbled(s, obj.c_str(), obj_kind, flags, oimg.empty() ? nullptr : oimg.data(), ow, oh, obj_copies,
                                              move_given ? obj_move : nullptr, double(W) / H, &cam, nullptr)))
        return die("rt_nw_scene_obj_stage_tumbled", rc);
    } else if (move_given) {
      if ((rc = rt_nw_scene_obj_stage_moving(s, obj.c_str(), obj_kind, flags, oimg.empty() ? nullptr : oimg.data(), ow, oh, obj_copies,
                                             obj_move, double(W) / H, &cam, nullptr)))
        return die("rt_nw_scene_obj_stage_moving", rc);
    } else if (obj_copies > 1) {
      if ((rc = rt_nw_scene_obj_stage_copies(s, obj.c_str(), obj_kind, flags, oimg.empty() ? nullptr : oimg.data(), ow, oh, obj_copies,
                                             double(W) / H, &cam, nullptr)))
        return die("rt_nw_scene_obj_stage_copies", rc);
    } else if (!flags) {
      if ((rc = rt_nw_scene_obj_stage(s, obj.c_str(), obj_kind, double(W) / H, &cam, nullptr))) return die("rt_nw_scene_obj_stage", rc);
    } else if ((rc = rt_nw_scene_obj_stage_attr(s, obj.c_str(), obj_kind, flags, oimg.empty() ? nullptr : oimg.data(), ow, oh,
                                                double(W) / H, &cam, nullptr))) {
      return die("rt_nw_scene_obj_stage_attr", rc);
    }
  } else if ((rc = rt_nw_scene_preset(s, which, img.empty() ? nullptr : img.data(), iw, ih, double(W) / H,
                                      rtl ? RT_NW_ARGS_RTL : 0, &cam))) {
    return die("rt_nw_scene_preset", rc);
  }
  if (shutter_given) {
    cam.time0 = shutter[0];
    cam.time1 = shutter[1];
  }
  rt_nw_ctx *ctx = nullptr;
  if ((rc = rt_nw_ctx_create(0, &ctx))) return die("rt_nw_ctx_create", rc);
  if ((rc = rt_nw_ctx_set_scene(ctx, s))) return die("rt_nw_ctx_set_scene", rc);
  std::vector<float> sum(size_t(W) * H * 3);
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t segs = 0;
  int spp_resumed = 0;
  int div = 0;              // what the sums are divided by for the image: spp, or 1 where sum holds means (--adaptive)
  double rendered = -1;     // samples this run rendered
  std::vector<int32_t> counts;
  std::vector<float> filtered;  // --denoise: the filtered means (sum then holds the noisy ones)
  if (adaptive >= 0) {
    counts.resize(size_t(W) * H);
    rt_nw_adapt_stats st{};
    if (denoise) {
      rt_nw_denoise_params dp;
      if ((rc = rt_nw_denoise_params_default(&dp))) return die("rt_nw_denoise_params_default", rc);
      dp.iterations = denoise_iters;
      filtered.resize(sum.size());
      if ((rc = rt_nw_render_denoised(ctx, s, &cam, W, H, min_spp, spp, pass_spp, adaptive, 0.03, 1, depth, seed,
                                      checkpoint.empty() ? nullptr : checkpoint.c_str(), time_limit, sum.data(), counts.data(), nullptr,
                                      &st, nullptr, nullptr, features_spp, &dp, filtered.data())))
        return die("rt_nw_render_denoised", rc);
    } else if ((rc = rt_nw_render_adaptive(ctx, s, &cam, W, H, min_spp, spp, pass_spp, adaptive, 0.03, 1, depth, seed,
                                           checkpoint.empty() ? nullptr : checkpoint.c_str(), time_limit, sum.data(), counts.data(),
                                           nullptr, &st, nullptr, nullptr))) {
      return die("rt_nw_render_adaptive", rc);
    }
    std::fprintf(stderr, "{\"adaptive\": %g, \"passes\": %d, \"stopped_by_time_limit\": %d, \"total_samples\": %lld, "
                         "\"mean_spp\": %.3f, \"share_at_max\": %.4f}\n",
                 adaptive, st.passes, st.stopped, (long long)st.total_samples, double(st.total_samples) / (double(W) * H),
                 double(st.pixels_at_max) / (double(W) * H));
    div = 1;  // (sum holds the per-pixel means; "spp" below stays the maximum)
    rendered = double(st.samples);
    segs = uint64_t(st.segments);
    if (st.passes == 0) rendered = 0;  // (a finished checkpoint: nothing was rendered)
  } else if (pass_spp > 0) {
    if ((rc = rt_nw_accum_reset(ctx, W, H))) return die("rt_nw_accum_reset", rc);
    int done = 0;
    if (!checkpoint.empty()) {
      if (FILE *probe = std::fopen(checkpoint.c_str(), "rb")) {
        std::fclose(probe);
        if ((rc = rt_nw_accum_load(ctx, checkpoint.c_str(), s, &cam, W, H, 0, 1, H, depth, seed, &done))) return die("rt_nw_accum_load", rc);
        spp_resumed = done;
      }
    }
    bool first = true;
    while (done < spp) {
      const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (!first && time_limit >= 0 && elapsed >= time_limit) break;
      first = false;
      const int k = std::min(pass_spp, spp - done);
      if ((rc = rt_nw_render_pass(ctx, &cam, W, H, done, k, depth, seed, 0, 1, H, nullptr))) return die("rt_nw_render_pass", rc);
      done += k;
      uint64_t ps = 0;  // (waits for the pass)
      if ((rc = rt_nw_ctx_last_segments(ctx, &ps))) return die("rt_nw_ctx_last_segments", rc);
      segs += ps;
      if (!checkpoint.empty() && (rc = rt_nw_accum_save(ctx, checkpoint.c_str(), s, &cam, H, 0, 1, depth, seed))) return die("rt_nw_accum_save", rc);
      std::fprintf(stderr, "{\"pass_done_spp\": %d}\n", done);
    }
    if ((rc = rt_nw_accum_resolve(ctx, nullptr, sum.data(), nullptr))) return die("rt_nw_accum_resolve", rc);
    spp = done;  // (under --time-limit: the samples the image holds)
  } else {
    if ((rc = rt_nw_render(ctx, &cam, W, H, spp, depth, seed, sum.data()))) return die("rt_nw_render", rc);
    rt_nw_ctx_last_segments(ctx, &segs);
  }
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (!div) div = spp;
  if (rendered < 0) rendered = double(W) * H * std::max(spp - spp_resumed, 0);
  std::fprintf(stderr,
               "{\"scene\": %d, \"width\": %d, \"height\": %d, \"spp\": %d, \"depth\": %d, \"seconds\": %.6f, "
               "\"msamples_per_s\": %.3f, \"segments_per_sample\": %.4f}\n",
               which, W, H, spp, depth, seconds, rendered / seconds / 1e6, rendered > 0 ? double(segs) / rendered : 0.0);
  if (!aov.empty()) {
    std::vector<float> feat(size_t(W) * H * 8), plane(size_t(W) * H * 3);
    if ((rc = rt_nw_render_features(ctx, &cam, W, H, features_spp, seed, nullptr, feat.data(), nullptr))) return die("rt_nw_render_features", rc);
    static const char *const kinds[3] = {"_albedo.pfm", "_normal.pfm", "_depth.pfm"};
    for (int k = 0; k < 3; ++k) {
      for (size_t p = 0; p < size_t(W) * H; ++p)
        for (int c = 0; c < 3; ++c) plane[3 * p + c] = feat[8 * p + (k < 2 ? 3 * k + c : 6)];
      if ((rc = rt_write_pfm((aov + kinds[k]).c_str(), plane.data(), W, H, 1))) return die("rt_write_pfm", rc);
    }
    if (denoise && (rc = rt_write_pfm((aov + "_noisy.pfm").c_str(), sum.data(), W, H, div ? div : spp))) return die("rt_write_pfm", rc);
  }
  if (denoise) sum.swap(filtered);  // (--out and --pfm carry the filtered image)
  rt_nw_ctx_destroy(ctx);
  rt_nw_scene_destroy(s);

  FILE *f = out == "-" ? stdout : std::fopen(out.c_str(), "wb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", out.c_str()); return 1; }
  std::fprintf(f, p6 ? "P6\n%d %d\n255\n" : "P3\n%d %d\n255\n", W, H);
  for (int j = H - 1; j >= 0; j--)  // main.cu:567-575
    for (int i = 0; i < W; i++) {
      int v[3];
      for (int c = 0; c < 3; c++) {
        const float mean = sum[(size_t(j) * W + i) * 3 + c] / float(div);
        v[c] = int(255.99 * double(std::sqrt(mean)));
      }
      if (p6) {
        for (int c = 0; c < 3; c++) std::fputc(v[c] < 0 ? 0 : v[c] > 255 ? 255 : v[c], f);
      } else {
        std::fprintf(f, "%d %d %d\n", v[0], v[1], v[2]);
      }
    }
  if (f != stdout) std::fclose(f);
  if (!pfm.empty() && (rc = rt_write_pfm(pfm.c_str(), sum.data(), W, H, div))) return die("rt_write_pfm", rc);
  if (!spp_map.empty()) {
    std::vector<float> cnt(size_t(W) * H * 3);
    for (size_t p = 0; p < counts.size(); ++p) cnt[3 * p] = cnt[3 * p + 1] = cnt[3 * p + 2] = float(counts[p]);
    if ((rc = rt_write_pfm(spp_map.c_str(), cnt.data(), W, H, 1))) return die("rt_write_pfm", rc);
  }
  return 0;
}
