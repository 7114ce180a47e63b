"""GPU parity: the HIP path (through the C ABI) against the oracle.

Three tiers:
  1. exact replay: the double-precision kernel instantiation, fed the
     reference's own rand() stream, reproduces the reference's KATs and
     single-threaded images BIT-EXACTLY;
  2. fast path: the production float kernel equals the oracle's fast-mode
     restatement BIT-EXACTLY (stricter than the 1e-4 per-channel tolerance
     north_star states) at sizes the oracle finishes in seconds, over every
     tile shape, chunking, edge tiles and depth edge cases;
  3. statistics: at config 2 (1200x800x500) the image sits at the reference's
     own Monte-Carlo noise floor against gallery/final.png, the reference's
     output (BASELINE.md §5 thresholds).
Plus size-independent properties at full size: determinism and partition /
tiling invariance.
"""
import ctypes as C
import os

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
import oracle_py as O
from conftest import record_parity_stats

pytestmark = pytest.mark.gpu
GOLD = O.GOLDEN
SEED = 1984


@pytest.fixture(scope="module")
def final_world():
    return rt.random_scene()


@pytest.fixture(scope="module")
def final_renderer(final_world):
    r = rt.Renderer(final_world, 0)
    r.set_accel("none")  # brute force unless a test selects a structure
    yield r
    r.close()


@pytest.fixture(scope="module")
def learn_renderer():
    r = rt.Renderer(rt.learn_scene(), 0)
    r.set_accel("none")
    yield r
    r.close()


def o_cam(cam):
    c = O.OrCamera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
    return c


def o_scene(world):
    return O.Scene(world.center_radius, world.mat_kind, world.mat_params)


# ------------------------------------------------------------ tier 1 -------
def glibc_stream(seed, n, skip_scene=False):
    g = O.OrGlibc()
    O.lib().or_glibc_seed(C.byref(g), seed)
    if skip_scene:  # the final scene's draws come first in a fresh process
        geom, kind, mat = np.zeros(4 * 600), np.zeros(600, np.int32), np.zeros(4 * 600)
        O.lib().or_final_scene(C.byref(g), O.dptr(geom), kind.ctypes.data_as(O._ip), O.dptr(mat), 600)
    return np.array([O.lib().or_glibc_rand(C.byref(g)) for _ in range(n)], np.int32)


@pytest.mark.parametrize("name", ["final", "learn"])
def test_exact_replay_reproduces_reference_kats(name, final_renderer, learn_renderer):
    r = final_renderer if name == "final" else learn_renderer
    cam = rt.final_camera() if name == "final" else rt.learn_camera()
    lines = open(os.path.join(GOLD, f"kats_{name}.txt")).read().split("\n")
    n, W, H = map(int, lines[0].split())
    kats = [ln.split() for ln in lines[1 : 1 + n]]
    jobs, streams = [], []
    for t in kats:
        k, i, j = int(t[0]), int(t[1]), int(t[2])
        jobs.append((j * W + i, j * W + i + 1))
        streams.append(glibc_stream(k, 2048))
    out, used = r.replay_worker(cam, W, H, 1, 50, jobs, streams)
    out = out.reshape(n, 3)
    for q, t in enumerate(kats):
        assert out[q].tolist() == [float(x) for x in t[3:6]], t[0]
        assert streams[q][used[q]] == int(t[6]), t[0]  # the next rand() the reference drew


@pytest.mark.parametrize("name,W,H,S", [("final", 24, 16, 8), ("learn", 32, 18, 16)])
def test_exact_replay_reproduces_reference_image(name, W, H, S, final_renderer, learn_renderer):
    r = final_renderer if name == "final" else learn_renderer
    cam = rt.final_camera(W / H) if name == "final" else rt.learn_camera(W / H)
    stream = glibc_stream(1, 200_000, skip_scene=(name == "final"))
    out, used = r.replay_worker(cam, W, H, S, 50, [(0, W * H)], [stream])
    gold = np.fromfile(os.path.join(GOLD, f"image_{name}_{W}x{H}x{S}.f64"), dtype="<f8")
    assert np.array_equal(out, gold)


# ------------------------------------------------------------ tier 2 -------
@pytest.mark.parametrize("kernel", ["persistent", "grid"])
@pytest.mark.parametrize("tile_w", [0, 8, 16, 32, 64])
@pytest.mark.parametrize("chunk", [0, 3, 1000])
def test_fast_kernel_bit_exact_vs_oracle_final(kernel, tile_w, chunk, final_world, final_renderer):
    W, H, S = 48, 32, 8
    cam = rt.final_camera(W / H)
    final_renderer.set_tuning(tile_w, chunk)
    final_renderer.set_kernel(kernel)
    try:
        got = final_renderer.render(cam, W, H, S, 50, SEED)
    finally:
        final_renderer.set_tuning(0, 0)
        final_renderer.set_kernel("auto")
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(got, want), np.abs(got - want).max()


@pytest.mark.parametrize("W,H,S,depth", [(37, 23, 5, 50), (64, 36, 16, 50), (20, 11, 3, 1), (16, 16, 4, 2), (9, 7, 1, 50)])
def test_fast_kernel_bit_exact_vs_oracle_learn(W, H, S, depth, learn_renderer):
    """Edge tiles (W, H not multiples of the tile), spp=1, max_depth 1 and 2,
    the hollow negative-radius sphere."""
    world = rt.learn_scene()
    cam = rt.learn_camera(W / H)
    got = learn_renderer.render(cam, W, H, S, depth, SEED)
    want = O.fast_render(o_scene(world), o_cam(cam), W, H, S, depth, SEED)
    assert np.array_equal(got, want), np.abs(got - want).max()


@pytest.mark.parametrize("W,H,S", [(2, 2, 3), (2, 17, 5), (97, 2, 4), (2, 2, 33), (3, 65, 17), (2, 2, 70000)])
def test_degenerate_shapes_bit_exact_vs_oracle(W, H, S, final_world):
    """The smallest images the reference's camera allows (u, v divide by W - 1
    and H - 1: at least 2 x 2; one pixel wide or tall is RT_EINVAL), tiles
    mostly empty, and 2 x 2 pixels at 70 000 spp (more than the 65 535
    samples an item may hold: two items each), through the default path
    (uniform grid, cost-ordered, the probe for spp >= 16), against the
    oracle; twice, so the second render runs on the first one's cost map."""
    cam = rt.final_camera(W / H)
    r = rt.Renderer(final_world, 0)
    try:
        for w, h in ((1, H), (W, 1)):
            with pytest.raises(rt.RTError, match="RT_EINVAL"):
                r.render(cam, w, h, S, 50, SEED)
        first = r.render(cam, W, H, S, 50, SEED)
        second = r.render(cam, W, H, S, 50, SEED)
        segs = r.last_segments()
        sch = r.last_schedule()
    finally:
        r.close()
    assert sch["bvh"] == 2 and sch["chunk"] <= 65535, sch
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(first, want) and np.array_equal(second, want)
    assert segs == O.fast_segments(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)


@pytest.mark.parametrize("case", ["pinhole", "inside_glass", "vfov_1", "vfov_170", "seed_0", "seed_max", "depth_500",
                                  "below_ground"])
def test_camera_seed_depth_edge_cases_bit_exact_vs_oracle(case, final_world):
    """Cameras and arguments away from the reference's defaults, through the
    default path (grid, cost-ordered) against the oracle: a pinhole (aperture
    0, rays from one point), the eye inside the big glass sphere (every
    primary ray starts inside a dielectric), a 1° and a 170° field of view,
    seeds 0 and 2^64 - 1, depth 500 (deep glass paths), and the eye inside
    the ground sphere looking up (every ray leaves the R = 1000 sphere from
    inside).  The world.hit count is compared too."""
    W, H, S, depth, seed = 48, 32, 6, 50, SEED
    lookfrom, lookat, vfov, aperture, focus = (13, 2, 3), (0, 0, 0), 20.0, 0.1, 10.0
    if case == "pinhole":
        aperture = 0.0
    elif case == "inside_glass":
        lookfrom, lookat, focus = (0, 1.2, 0.3), (4, 1, 0), 4.0
    elif case == "vfov_1":
        vfov = 1.0
    elif case == "vfov_170":
        vfov = 170.0
    elif case == "seed_0":
        seed = 0
    elif case == "seed_max":
        seed = 2**64 - 1
    elif case == "depth_500":
        depth = 500
    elif case == "below_ground":
        lookfrom, lookat, focus = (1, -3, 2), (0, 5, 0), 8.0
    cam = rt.camera(lookfrom, lookat, (0, 1, 0), vfov, W / H, aperture, focus)
    r = rt.Renderer(final_world, 0)
    try:
        got = r.render(cam, W, H, S, depth, seed)
        segs = r.last_segments()
    finally:
        r.close()
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, depth, seed)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert segs == O.fast_segments(o_scene(final_world), o_cam(cam), W, H, S, depth, seed)


@pytest.mark.parametrize("n", [3000, 70000])
def test_large_scenes_bit_exact_vs_oracle(n):
    """Scenes far larger than the final scene's 487 spheres: neither the grid
    nor the BVH fits its LDS budget, so each is walked in global memory (the
    schedule's "bvh" field: 4 = the grid in global memory, 1 = the BVH); the
    grid's 16-bit indices stop at 65 535 spheres, where the grid setting falls
    back to the BVH; brute force on request.  The image and world.hit count
    equal the oracle's for every accel setting."""
    g = np.random.default_rng(n)
    c = np.column_stack([g.uniform(-40, 40, n), g.uniform(0.05, 0.3, n), g.uniform(-40, 40, n)])
    rad = g.uniform(0.03, 0.2, n)
    kinds = g.integers(0, 3, n).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, n))])
    cr = np.vstack([[0, -1000, 0, 1000], np.column_stack([c, rad])])
    kinds = np.concatenate([[0], kinds]).astype(np.int32)
    params = np.vstack([[0.5, 0.5, 0.5, 0], params])
    world = rt.World(cr, kinds, params)
    W, H, S = 24, 16, 2
    cam = rt.camera((20, 3, 12), (0, 0, 0), (0, 1, 0), 30.0, W / H, 0.05, 20.0)
    want = O.fast_render(o_scene(world), o_cam(cam), W, H, S, 50, SEED)
    want_segs = O.fast_segments(o_scene(world), o_cam(cam), W, H, S, 50, SEED)
    r = rt.Renderer(world, 0)
    ran = set()
    try:
        for accel in ("grid", "bvh", "none"):
            r.set_accel(accel)
            got = r.render(cam, W, H, S, 50, SEED)
            ran.add((accel, r.last_schedule()["bvh"]))
            assert np.array_equal(got, want), (accel, np.abs(got - want).max())
            assert r.last_segments() == want_segs, accel
        # the validation entry point takes the walk these renders take (the
        # global grid, or past 65 535 spheres the global BVH):
        # 20 000 rays through the sphere layer, closest hit == brute force
        r.set_accel("grid")
        L = rt.load()
        L.rt_ctx_debug_hits.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_float)]
        m = 20_000
        o = np.column_stack([g.uniform(-45, 45, m), g.uniform(0.0, 3.0, m), g.uniform(-45, 45, m)])
        dv = g.normal(size=(m, 3)) * [1.0, 0.2, 1.0]
        rays = np.ascontiguousarray(np.column_stack([o, dv]).astype(np.float32))
        idx, t = np.zeros(2 * m, np.int32), np.zeros(2 * m, np.float32)
        rc = L.rt_ctx_debug_hits(r._h, rays.ctypes.data_as(C.POINTER(C.c_float)), m,
                                 idx.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_float)))
    finally:
        r.close()
    assert ran == {("grid", 4 if n <= 65535 else 1), ("bvh", 1), ("none", 0)}, ran
    assert rc == 0
    idx, t = idx.reshape(m, 2), t.reshape(m, 2)
    assert (idx[:, 0] >= 0).mean() > 0.2 and (idx[:, 0] > 0).mean() > 0.05  # (index 0: the ground)
    assert np.array_equal(idx[:, 0], idx[:, 1]) and np.array_equal(t[:, 0], t[:, 1])


def test_max_depth_limit(learn_renderer):
    """max_depth lives in the low 24 bits of a path's register: 2^24 - 1 is
    accepted, 2^24 refused (RT_EINVAL), as is a negative depth."""
    cam = rt.learn_camera(2.0)
    learn_renderer.render(cam, 4, 2, 1, (1 << 24) - 1, SEED)
    for bad in (1 << 24, -1):
        with pytest.raises(rt.RTError, match="RT_EINVAL"):
            learn_renderer.render(cam, 4, 2, 1, bad, SEED)


def test_max_depth_zero_is_black(learn_renderer):
    got = learn_renderer.render(rt.learn_camera(), 16, 9, 4, 0, SEED)
    assert not got.any()


def test_seed_changes_image(learn_renderer):
    cam = rt.learn_camera(2.0)
    a = learn_renderer.render(cam, 32, 16, 4, 50, 1)
    b = learn_renderer.render(cam, 32, 16, 4, 50, 2)
    assert not np.array_equal(a, b)


def test_config1_fast_vs_oracle_bit_exact(learn_renderer):
    """Config 1 (400x225x100, learn) whole image vs the fast-mode oracle."""
    world = rt.learn_scene()
    cam = rt.learn_camera(400 / 225)
    got = learn_renderer.render(cam, 400, 225, 100, 50, SEED)
    want = O.fast_render(o_scene(world), o_cam(cam), 400, 225, 100, 50, SEED)
    assert np.array_equal(got, want)
    # tolerance stated by north_star, for the record: <= 1e-4 per channel on sum/spp
    assert np.abs(got / 100 - want / 100).max() <= 1e-4


def test_rows_strips_equal_full_image(final_renderer):
    torch = pytest.importorskip("torch")
    W, H, S, G = 40, 30, 4, 4
    cam = rt.final_camera(W / H)
    full = final_renderer.render(cam, W, H, S, 50, SEED)
    nrows = (H + G - 1) // G
    dev = torch.device("cuda", 0)
    for g in range(G):
        strip = torch.full((nrows, W, 3), -1.0, dtype=torch.float32, device=dev)
        final_renderer.render_rows(cam, W, H, S, 50, SEED, g, G, nrows, strip.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        s = strip.cpu().numpy()
        for k in range(nrows):
            j = g + k * G
            if j < H:
                assert np.array_equal(s[k], full[j]), (g, k)
            else:
                assert not s[k].any()


def test_render_multi_one_gpu_equals_render(final_world, final_renderer):
    W, H, S = 40, 30, 4
    cam = rt.final_camera(W / H)
    a = final_renderer.render(cam, W, H, S, 50, SEED)
    b = rt.render_multi(W, H, S, 50, final_world, cam, SEED, n_gpus=1)
    assert np.array_equal(a, b)


def test_multi_renderer_reuses_contexts_passes_and_times(final_world, final_renderer):
    """rt_multi_*: contexts, scene and communicator made once and reused by
    two renders; progressive passes on the device set resolve to the same
    bits; per-device strip and gather times are reported."""
    W, H, S = 40, 30, 6
    cam = rt.final_camera(W / H)
    want = final_renderer.render(cam, W, H, S, 50, SEED)
    m = rt.MultiRenderer(final_world, n_gpus=1)
    try:
        for _ in range(2):
            assert np.array_equal(m.render(cam, W, H, S, 50, SEED), want)
        strip_ms, gather_ms = m.last_timing()
        assert len(strip_ms) == 1 and strip_ms[0] > 0 and gather_ms >= 0
        m.accum_reset(W, H)
        m.render_pass(cam, 0, 2)
        m.render_pass(cam, 2, 4)
        assert np.array_equal(m.accum_resolve(), want)
    finally:
        m.close()


def test_multi_create_fails_cleanly_after_partial_setup(final_world, final_renderer):
    """rt_multi_create with a scene that the device context rejects (an
    unknown material kind: rt_ctx_set_scene fails after rt_ctx_create has
    made device 0's context) returns the error with no handle and leaves
    nothing behind: a good device set made next renders the same bits."""
    bad = rt.World(final_world.center_radius.copy(), final_world.mat_kind.copy(), final_world.mat_params.copy())
    bad.mat_kind[7] = 9
    L = rt.load()
    h = C.c_void_p()
    sc = bad.c_struct()
    rc = L.rt_multi_create(C.byref(sc), 1, C.byref(h))
    assert rc == -4 and not h.value  # RT_EUNSUPPORTED
    assert b"material kind" in L.rt_last_error()
    W, H, S = 24, 16, 3
    cam = rt.final_camera(W / H)
    m = rt.MultiRenderer(final_world, n_gpus=1)
    try:
        assert np.array_equal(m.render(cam, W, H, S, 50, SEED), final_renderer.render(cam, W, H, S, 50, SEED))
    finally:
        m.close()


def test_multi_failed_pass_invalidates_the_accumulators(final_world, final_renderer):
    """A progressive pass that fails on a device leaves the device set's
    accumulators covering different sample ranges: rt_multi_accum_resolve
    refuses them until rt_multi_accum_reset, and a reset set
    resolves to the one-render bits again."""
    W, H = 24, 16
    cam = rt.final_camera(W / H)
    m = rt.MultiRenderer(final_world, n_gpus=1)
    try:
        m.accum_reset(W, H)
        m.render_pass(cam, 0, 2)
        with pytest.raises(RuntimeError):
            m.render_pass(cam, 2, 2, max_depth=-1)  # rejected on device 0
        with pytest.raises(RuntimeError):
            m.accum_resolve()
        m.accum_reset(W, H)
        m.render_pass(cam, 0, 2)
        m.render_pass(cam, 2, 2)
        assert np.array_equal(m.accum_resolve(), final_renderer.render(cam, W, H, 4, 50, SEED))
    finally:
        m.close()


# ---------------------------------------------------- full-size properties -
@pytest.fixture(scope="module")
def config2(final_renderer):
    cam = rt.final_camera(1.5)
    final_renderer.set_tuning(8, 0)
    img = final_renderer.render(cam, 1200, 800, 500, 50, SEED)
    return cam, img


def test_config2_deterministic_and_tiling_invariant(config2, final_renderer):
    """Same image from the other kernel shape, another tile and a two-phase
    schedule (long items, then a 60-spp tail of 7-sample items)."""
    cam, img = config2
    final_renderer.set_tuning(64, 100)
    final_renderer.set_schedule(100, 60, 7)
    final_renderer.set_kernel("persistent")
    try:
        again = final_renderer.render(cam, 1200, 800, 500, 50, SEED)
    finally:
        final_renderer.set_tuning(8, 0)
        final_renderer.set_schedule(0, -1, 0)
        final_renderer.set_kernel("auto")
    assert np.array_equal(img, again)


@pytest.mark.parametrize("sched", [(2, 0, 0), (3, 37, 1)])
def test_persistent_schedules_bit_exact_vs_oracle(sched, final_world, final_renderer):
    """The persistent kernel with many more items than resident waves and a
    short-item tail phase (items of two sizes in flight in one wave)."""
    W, H, S = 160, 96, 64
    cam = rt.final_camera(W / H)
    final_renderer.set_schedule(*sched)  # 7680 / 12240 items: several per resident wave
    final_renderer.set_kernel("persistent")
    try:
        got = final_renderer.render(cam, W, H, S, 50, SEED)
    finally:
        final_renderer.set_schedule(0, -1, 0)
        final_renderer.set_kernel("auto")
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(got, want), np.abs(got - want).max()


def test_config2_sampled_pixels_bit_exact_vs_oracle(config2, final_world):
    """A strip of config 2 (rows 0, 97, 194, ...: every 97th row, 9 rows)
    against the oracle at full width and spp."""
    cam, img = config2
    want = O.fast_render(o_scene(final_world), o_cam(cam), 1200, 800, 500, 50, SEED, row0=0, row_step=97, nrows=9)
    assert np.array_equal(img[0::97][:9], want)


def _png_rgb(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64)


def test_config2_statistics_vs_reference_gallery(config2):
    """reference-vs-reference noise at config 2 is bias 0.0014,
    MAE 1.064, RMSE 1.795, 40x40-tile max |d| 0.254 levels.  Thresholds from
    SURVEY §8(c): |bias| < 0.05, MAE <= 1.2, RMSE <= 2.0, tile max <= 0.4."""
    _, img = config2
    ours = rt.quantize(img, 500).astype(np.float64)
    ref = _png_rgb(os.path.join(GOLD, "gallery_final.png"))
    d = ours - ref
    bias, mae, rmse = d.mean(), np.abs(d).mean(), np.sqrt((d * d).mean())
    tiles = ours.reshape(20, 40, 30, 40, 3).mean(axis=(1, 3))
    tile_max = np.abs(tiles - np.load(os.path.join(GOLD, "gallery_final_tiles40.npy"))).max()
    print(f"config2 vs gallery: bias {bias:.4f} MAE {mae:.3f} RMSE {rmse:.3f} tile max {tile_max:.3f}")
    record_parity_stats("config2_vs_gallery_final", {
        "bias": bias, "mae": mae, "rmse": rmse, "tile40_max_abs": tile_max,
        "frac_gt_1": (np.abs(d) > 1).mean(), "frac_gt_2": (np.abs(d) > 2).mean(), "frac_gt_4": (np.abs(d) > 4).mean(),
        "frac_gt_8": (np.abs(d) > 8).mean(),
        "thresholds": "SURVEY 8(c): |bias| < 0.05, MAE <= 1.2, RMSE <= 2.0, tile max <= 0.4",
        "reference_vs_reference_floor": "BASELINE.md 5: bias 0.0014, MAE 1.064, RMSE 1.795, tile max 0.254"})
    assert abs(bias) < 0.05 and mae <= 1.2 and rmse <= 2.0 and tile_max <= 0.4


def test_config1_statistics_vs_reference_image(learn_renderer):
    """Config 1 GPU image vs the reference's config-1 image, against the
    reference's own noise (ref mode, a different rand() seed)."""
    cam = rt.learn_camera(400 / 225)
    ours = rt.quantize(learn_renderer.render(cam, 400, 225, 100, 50, SEED), 100).astype(np.float64)
    raw = open(os.path.join(GOLD, "learn_400x225x100.ppm"), "rb").read()
    gold = np.frombuffer(raw[len(b"P6\n400 225\n255\n"):], np.uint8).reshape(225, 400, 3).astype(np.float64)
    g = O.OrGlibc()
    O.lib().or_glibc_seed(C.byref(g), 7)
    other, _ = O.ref_worker(O.learn_scene(), O.learn_camera(400 / 225), 400, 225, 100, 50, 0, 400 * 225, g)
    noise = rt.quantize(other.reshape(225, 400, 3).astype(np.float32), 100).astype(np.float64)
    floor = np.sqrt(((noise - gold) ** 2).mean())
    rmse = np.sqrt(((ours - gold) ** 2).mean())
    print(f"config1 RMSE ours {rmse:.3f} vs reference-vs-reference {floor:.3f}")
    record_parity_stats("config1_vs_reference_image", {
        "rmse": rmse, "reference_vs_reference_rmse": floor, "ratio": rmse / floor, "bias": (ours - gold).mean(),
        "thresholds": "RMSE <= 1.15 x the reference's own seed-to-seed RMSE, |bias| < 0.1"})
    assert rmse <= 1.15 * floor and abs((ours - gold).mean()) < 0.1


def test_segment_count_matches_oracle(final_world, final_renderer):
    """The GPU's world.hit counter (the roofline's work unit) equals the
    oracle's count for the same render: same paths, same lengths."""
    W, H, S = 48, 32, 8
    cam = rt.final_camera(W / H)
    final_renderer.render(cam, W, H, S, 50, SEED)
    assert final_renderer.last_segments() == O.fast_segments(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)


# ------------------------------------------------------------ BVH ----------
@pytest.mark.parametrize("accel", ["bvh", "grid"])
@pytest.mark.parametrize("kernel", ["grid", "persistent"])
def test_bvh_bit_exact_vs_oracle_final(kernel, accel, final_world, final_renderer):
    """RT_ACCEL_BVH and RT_ACCEL_GRID find the same closest hit as the
    brute-force loop, so the image equals the (brute-force) oracle bit for bit."""
    W, H, S = 96, 64, 8
    cam = rt.final_camera(W / H)
    nb, nn = final_renderer.accel_info()
    assert nb == 4 and nn > 100  # ground + the three r=1 spheres stay brute force
    dims, nrefs, lds = final_renderer.grid_info()
    # the record slots + 1.5 KB of shared accumulators + ~0.2 KB of static LDS
    # must stay within 20 KB per 4-wave block: 8 blocks per CU
    assert dims[1] == 1 and dims[0] * dims[2] >= 400 and nrefs >= 483 and lds + 1536 + 256 <= 20480, (dims, nrefs, lds)
    final_renderer.set_accel(accel)
    final_renderer.set_kernel(kernel)
    try:
        got = final_renderer.render(cam, W, H, S, 50, SEED)
        segs = final_renderer.last_segments()
    finally:
        final_renderer.set_accel("none")
        final_renderer.set_kernel("auto")
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert segs == O.fast_segments(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_bvh_learn_scene_edge_cases(accel, learn_renderer):
    world = rt.learn_scene()
    for (W, H, S, depth) in [(37, 23, 5, 50), (20, 11, 3, 1), (9, 7, 1, 50)]:
        cam = rt.learn_camera(W / H)
        learn_renderer.set_accel(accel)
        try:
            got = learn_renderer.render(cam, W, H, S, depth, SEED)
        finally:
            learn_renderer.set_accel("none")
        want = O.fast_render(o_scene(world), o_cam(cam), W, H, S, depth, SEED)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("accel", ["bvh", "grid"])
@pytest.mark.parametrize("seed,scale,shift", [(1, 1.0, 0.0), (2, 1.0, 0.0), (3, 1.0, 0.0), (4, 3000.0, 50000.0)])
def test_bvh_random_scenes_equal_brute_force(seed, scale, shift, accel):
    """Random scenes: radii over three decades, overlaps, hollow (negative
    radius) spheres, huge spheres, coincident centres; BVH == brute force.
    The last case is scaled and shifted so that node bounds leave the half
    range (boxes stored as halves rounded outward become infinite on that
    side) and lose most of their precision: still the same image."""
    g = np.random.default_rng(seed)
    n = 300
    c = g.uniform(-8, 8, (n, 3))
    c[:, 1] = g.uniform(-0.5, 3, n)
    r = np.exp(g.uniform(np.log(0.01), np.log(1.5), n))
    r[g.random(n) < 0.05] *= -1  # hollow shells
    c[10] = c[11]  # coincident pair, equal radii: ties decided by index
    r[10] = r[11] = 0.3
    kinds = g.integers(0, 3, n).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, n))])
    cr = np.column_stack([c, r])
    cr = np.vstack([[0, -1000, 0, 1000], [0, 1, 40, 30], cr])  # ground + one more big sphere
    kinds = np.concatenate([[0, 1], kinds]).astype(np.int32)
    params = np.vstack([[0.5, 0.5, 0.5, 0], [0.7, 0.6, 0.5, 0.1], params])
    cr = cr * scale
    cr[:, 0] += shift
    world = rt.World(cr, kinds, params)
    look_from = (13 * scale + shift, 2 * scale, 3 * scale)
    cam = rt.camera(look_from, (shift, 0, 0), (0, 1, 0), 40.0, 1.5, 0.1 * scale, 10.0 * scale)
    r_ = rt.Renderer(world, 0)
    try:
        r_.set_accel("none")
        want = r_.render(cam, 72, 48, 6, 50, SEED)
        r_.set_accel(accel)
        got = r_.render(cam, 72, 48, 6, 50, SEED)
        # (the grid in LDS, or in global memory when its image would cost occupancy)
        assert r_.last_schedule()["bvh"] in {"bvh": (1,), "grid": (2, 4)}[accel]
    finally:
        r_.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_bvh_config2_equals_brute_force(accel, config2, final_renderer):
    cam, img = config2
    final_renderer.set_accel(accel)
    try:
        got = final_renderer.render(cam, 1200, 800, 500, 50, SEED)
    finally:
        final_renderer.set_accel("none")
    assert np.array_equal(got, img)


@pytest.mark.parametrize("accel", ["bvh", "grid"])
def test_global_structures_config2_equal_frame(accel, config2, final_world, monkeypatch):
    """The BVH / the grid walked in global memory (the paths of scenes whose
    structure is over the LDS budget, forced by RTMI_BVH_GLOBAL=1 /
    RTMI_GRID_GLOBAL=1): config 2 equals the frame."""
    cam, img = config2
    monkeypatch.setenv("RTMI_BVH_GLOBAL" if accel == "bvh" else "RTMI_GRID_GLOBAL", "1")
    r = rt.Renderer(final_world, 0)
    try:
        r.set_accel(accel)
        got = r.render(cam, 1200, 800, 500, 50, SEED)
        assert r.last_schedule()["bvh"] == {"bvh": 1, "grid": 4}[accel]
    finally:
        r.close()
    assert np.array_equal(got, img)


@pytest.mark.parametrize("accel", ["bvh", "grid", "bvh_global", "grid_global"])
def test_bvh_adversarial_rays_equal_brute_force(accel, final_world, monkeypatch):
    """1M random rays: origins in the field and just off sphere surfaces
    (both sides), directions with exactly-zero components (+0.0 and -0.0)
    and along cell planes; the BVH's / grid's closest hit (index and t) equals the
    brute-force loop's for every ray (rt_ctx_debug_hits, a validation entry
    point).  *_global: the structure walked in global memory, the path of
    scenes whose structure is over the LDS budget (forced here by
    RTMI_BVH_GLOBAL=1 / RTMI_GRID_GLOBAL=1)."""
    if accel.endswith("_global"):
        monkeypatch.setenv(f"RTMI_{accel.split('_')[0].upper()}_GLOBAL", "1")
    r = rt.Renderer(final_world, 0)
    r.set_accel(accel.split("_")[0])
    L = rt.load()
    L.rt_ctx_debug_hits.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    n = 1_000_000
    g = np.random.default_rng(11)
    o = np.column_stack([g.uniform(-13, 13, n), g.uniform(-0.1, 3, n), g.uniform(-13, 13, n)])
    k = g.integers(0, len(final_world), n // 2)
    c, rad = final_world.center_radius[k, :3], np.abs(final_world.center_radius[k, 3])
    u = g.normal(size=(n // 2, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[: n // 2] = c + u * (rad[:, None] * (1 + g.choice([1e-3, 1e-4, -1e-4, 1e-6, 0.0], n // 2)[:, None]))
    dv = g.normal(size=(n, 3)) * g.choice([0.3, 1.0, 3.0], n)[:, None]
    z = g.random((n, 3)) < 0.03
    dv[z] = np.where(g.random(int(z.sum())) < 0.5, 0.0, -0.0)  # exact zeros of both signs
    # grazing rays inside the sphere layer (long DDA walks) and rays from
    # integer grid-like coordinates
    m = n // 8
    o[-m:, 1] = g.uniform(0.0, 0.45, m)
    dv[-m:, 1] = g.choice([0.0, -0.0, 1e-3, -1e-3, 0.05], m)
    o[-2 * m:-m, [0, 2]] = np.round(o[-2 * m:-m, [0, 2]] * 2) / 2
    dv[np.all(dv == 0, axis=1)] = [0, -1, 0]  # no zero directions (not a ray)
    rays = np.ascontiguousarray(np.column_stack([o, dv]).astype(np.float32))
    idx = np.zeros(2 * n, np.int32)
    t = np.zeros(2 * n, np.float32)
    try:
        rc = L.rt_ctx_debug_hits(r._h, rays.ctypes.data_as(C.POINTER(C.c_float)), n, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                 t.ctypes.data_as(C.POINTER(C.c_float)))
    finally:
        r.close()
    assert rc == 0
    idx, t = idx.reshape(n, 2), t.reshape(n, 2)
    assert (idx[:, 0] >= 0).mean() > 0.5
    bad = np.nonzero((idx[:, 0] != idx[:, 1]) | (t[:, 0] != t[:, 1]))[0]
    if bad.size:  # kept for diagnosis (merged back from the GPU box)
        os.makedirs(os.path.join(O.REPO, "gpurun_out"), exist_ok=True)
        np.savez(os.path.join(O.REPO, "gpurun_out", f"mismatch_{accel}.npz"), rays=rays[bad], idx=idx[bad], t=t[bad])
    assert np.array_equal(idx[:, 0], idx[:, 1]), f"{bad.size} rays differ"
    assert np.array_equal(t[:, 0], t[:, 1])


def test_grid_general_and_one_layer_walks(final_world):
    """The grid kernel has two walks: the one-layer walk for
    grids with a single cell layer in y (the final scene: asserted) and the
    general 3D walk (a scene of spheres filling a cube: asserted ny > 1).
    For the 3D scene, 200 k adversarial rays through rt_ctx_debug_hits (the
    walk the renders use) give the brute-force loop's index and t, and a
    render equals the brute-force render bit for bit."""
    r = rt.Renderer(final_world, 0)
    try:
        r.set_accel("grid")
        assert r.grid_info()[0][1] == 1
    finally:
        r.close()
    g = np.random.default_rng(5)
    n = 400
    c = g.uniform(-4, 4, (n, 3))
    rad = np.exp(g.uniform(np.log(0.05), np.log(0.4), n))
    kinds = g.integers(0, 3, n).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, n))])
    cr = np.vstack([[0, -1000, 0, 1000], np.column_stack([c, rad])])
    kinds = np.concatenate([[0], kinds]).astype(np.int32)
    params = np.vstack([[0.5, 0.5, 0.5, 0], params])
    world = rt.World(cr, kinds, params)
    cam = rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.1, 10.0)
    r = rt.Renderer(world, 0)
    L = rt.load()
    L.rt_ctx_debug_hits.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    try:
        r.set_accel("none")
        want = r.render(cam, 64, 48, 6, 50, SEED)
        r.set_accel("grid")
        dims = r.grid_info()[0]
        assert dims[1] > 1, dims
        got = r.render(cam, 64, 48, 6, 50, SEED)
        assert r.last_schedule()["bvh"] == 2
        m = 200_000
        o = g.uniform(-5, 5, (m, 3))
        k = g.integers(1, n + 1, m // 2)
        u = g.normal(size=(m // 2, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o[: m // 2] = cr[k, :3] + u * (cr[k, 3:4] * (1 + g.choice([1e-3, 1e-4, -1e-4, 0.0], m // 2)[:, None]))
        dv = g.normal(size=(m, 3))
        z = g.random((m, 3)) < 0.03
        dv[z] = np.where(g.random(int(z.sum())) < 0.5, 0.0, -0.0)  # exact zeros of both signs
        dv[np.all(dv == 0, axis=1)] = [0, -1, 0]
        rays = np.ascontiguousarray(np.column_stack([o, dv]).astype(np.float32))
        idx = np.zeros(2 * m, np.int32)
        t = np.zeros(2 * m, np.float32)
        rc = L.rt_ctx_debug_hits(r._h, rays.ctypes.data_as(C.POINTER(C.c_float)), m, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                 t.ctypes.data_as(C.POINTER(C.c_float)))
    finally:
        r.close()
    assert rc == 0
    assert np.array_equal(got, want)
    idx, t = idx.reshape(m, 2), t.reshape(m, 2)
    assert (idx[:, 0] >= 0).mean() > 0.3
    assert np.array_equal(idx[:, 0], idx[:, 1]) and np.array_equal(t[:, 0], t[:, 1])


@pytest.mark.parametrize("kernel,accel", [("grid", "none"), ("persistent", "none"), ("grid", "bvh"), ("persistent", "bvh"),
                                          ("grid", "grid"), ("persistent", "grid")])
def test_cost_ordered_dispatch_same_image(kernel, accel, final_world, final_renderer):
    """RT_ORDER_COST: the second render of a layout dispatches tiles by the
    first one's per-tile cost; the image is the same bit for bit (and equals
    the oracle's)."""
    W, H, S = 120, 72, 12
    cam = rt.final_camera(W / H)
    final_renderer.set_kernel(kernel)
    final_renderer.set_accel(accel)
    try:
        final_renderer.set_ordering("none")
        plain = final_renderer.render(cam, W, H, S, 50, SEED)
        final_renderer.set_ordering("cost")
        first = final_renderer.render(cam, W, H, S, 50, SEED)
        ordered = final_renderer.render(cam, W, H, 2 * S, 50, SEED + 1)  # same layout: ordered by `first`
        again = final_renderer.render(cam, W, H, S, 50, SEED)
    finally:
        final_renderer.set_kernel("auto")
        final_renderer.set_accel("none")
        final_renderer.set_ordering("cost")
    assert np.array_equal(first, plain) and np.array_equal(again, plain)
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, 2 * S, 50, SEED + 1)
    assert np.array_equal(ordered, want)


@pytest.mark.parametrize("probe_spp,probe_depth", [("1", "0"), ("2", "0"), ("5", "0"), ("1", "50"), ("2", "2")])
def test_probe_samples_do_not_change_the_image(probe_spp, probe_depth, final_world, monkeypatch):
    """The cost probe of a one-shot render (RTMI_PROBE_SPP samples per pixel,
    paths cut at RTMI_PROBE_DEPTH segments, into the output, counting
    world.hit per tile) only orders the tiles: the image and the world.hit
    count of the render equal the unordered render's and the oracle's,
    whatever the probe's sample count and depth (0: the default, 8)."""
    W, H, S = 64, 40, 20
    cam = rt.final_camera(W / H)
    monkeypatch.setenv("RTMI_PROBE_SPP", probe_spp)
    monkeypatch.setenv("RTMI_PROBE_DEPTH", probe_depth)
    r = rt.Renderer(final_world, 0)
    try:
        r.set_accel("grid")
        r.set_ordering("none")
        plain = r.render(cam, W, H, S, 50, SEED)
        plain_segs = r.last_segments()
        r.set_ordering("cost")  # no map of this layout: probe first
        got = r.render(cam, W, H, S, 50, SEED)
        segs = r.last_segments()
    finally:
        r.close()
    assert np.array_equal(got, plain) and segs == plain_segs
    assert np.array_equal(got, O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED))


@pytest.mark.parametrize("accel", ["none", "bvh", "grid"])
@pytest.mark.parametrize("W,H,S", [(40, 24, 37), (29, 19, 37), (29, 19, 5)])
def test_block_flush_same_image(accel, W, H, S, final_world, monkeypatch):
    """The automatic grid schedule gives every block exactly 4 items of one
    tile and flushes the block's summed accumulators once — here the block
    owns its tile and writes the floats itself (RTMI_BLOCK_OWNS=0: through
    the accumulator); RTMI_BLOCK_FLUSH=0 flushes per wave.  Same image and world.hit count
    bit for bit, equal to the oracle.  37 spp: items of 10/10/10/7 samples;
    29x19: partial tiles (automatic 16x4 shape); 29x19 at 5 spp: items of
    2/2/1/0 samples (the empty item's wave only joins the flush).  The launch
    schedule is read back, so the test cannot pass on a path it skipped."""
    cam = rt.final_camera(W / H)
    imgs, segs = [], []
    for flush, owns in (("1", "1"), ("0", "1"), ("1", "0")):
        monkeypatch.setenv("RTMI_BLOCK_FLUSH", flush)
        monkeypatch.setenv("RTMI_BLOCK_OWNS", owns)
        r = rt.Renderer(final_world, 0)
        try:
            r.set_kernel("grid")
            r.set_accel(accel)
            imgs.append(r.render(cam, W, H, S, 50, SEED))
            segs.append(r.last_segments())
            sch = r.last_schedule()
        finally:
            r.close()
        assert sch["items_per_tile"] == 4 and sch["persistent"] == 0, sch
        # 4 items per tile on 4-wave blocks: the block owns its tile (2)
        assert sch["block_flush"] == (0 if flush == "0" else (2 if owns == "1" else 1)), sch
        assert sch["ray_pool"] == 1, sch
        if S == 5:
            assert sch["chunk"] == 2  # 2, 2, 1, 0 samples
    assert all(np.array_equal(imgs[0], im) for im in imgs[1:])
    assert all(sg == segs[0] for sg in segs)
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(imgs[0], want)


@pytest.mark.parametrize("accel", ["none", "grid"])
@pytest.mark.parametrize("tail", [5, 40])
def test_block_flush_with_tail_phase(accel, tail, final_world, final_renderer):
    """A short-item tail phase with automatic item sizes keeps a multiple of
    the block's 4 waves items per tile in BOTH phases, so every block still
    covers one tile and flushes once (through the accumulator: no block owns
    its tile).  Bit-exact vs the oracle; the schedule is read back."""
    W, H, S = 40, 24, 130
    cam = rt.final_camera(W / H)
    final_renderer.set_accel(accel)
    final_renderer.set_kernel("grid")
    final_renderer.set_schedule(0, tail, 0)
    try:
        got = final_renderer.render(cam, W, H, S, 50, SEED)
        sch = final_renderer.last_schedule()
    finally:
        final_renderer.set_schedule(0, -1, 0)
        final_renderer.set_kernel("auto")
        final_renderer.set_accel("none")
    assert sch["items_per_tile"] % 4 == 0 and sch["tail_items_per_tile"] % 4 == 0, sch
    assert sch["tail_items_per_tile"] > 0 and sch["block_flush"] == 1, sch
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("accel", ["none", "bvh", "grid"])
def test_cost_probe_same_image_and_count(accel, final_world, final_renderer):
    """A render with no cost map of its layout (set_ordering forgets it) runs a
    probe pass of 1-2 spp into its own output first: the image and the
    world.hit count are the render's alone (the probe's are not added)."""
    W, H, S = 72, 40, 24
    cam = rt.final_camera(W / H)
    final_renderer.set_accel(accel)
    try:
        final_renderer.set_ordering("cost")
        got = final_renderer.render(cam, W, H, S, 50, SEED)
        segs = final_renderer.last_segments()
    finally:
        final_renderer.set_accel("none")
    want = O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)
    assert np.array_equal(got, want)
    assert segs == O.fast_segments(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED)


def test_non_finite_sample_colours_are_guarded():
    """A NaN albedo (and an overflowing one) make non-finite path colours; the
    fixed-point conversion maps NaN to 0 and clamps to [0, 64] on the GPU
    exactly as in the oracle, so the sums stay finite and bit-exact."""
    world = rt.learn_scene()
    world.mat_params[1, :3] = [np.nan, 0.5, 0.5]  # centre sphere: NaN red channel
    world.mat_params[4, :3] = [1e30, 1e30, 1e30]  # right (metal) sphere: attenuation overflows to inf
    world.mat_params[0, :3] = [-0.5, 0.5, 0.5]  # ground: negative red (clamped to 0 per sample)
    W, H, S = 40, 24, 8
    cam = rt.learn_camera(W / H)
    r = rt.Renderer(world, 0)
    try:
        got = r.render(cam, W, H, S, 50, SEED)
    finally:
        r.close()
    want = O.fast_render(o_scene(world), o_cam(cam), W, H, S, 50, SEED)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)
    assert got.max() == 64.0 * S or got.max() > 1.0 * S  # the clamp was reached somewhere
    assert got.min() >= 0.0


# ------------------------------------------------------------ config 5 -----
C5 = (3840, 2160, 2000)
C5_ROWS = (0, 1531)  # the bottom row and one through the spheres' band


@pytest.fixture(scope="module")
def config5_oracle_rows(final_world):
    """The oracle's two full-width config-5 rows at full spp (computed once
    for both accelerators)."""
    W, H, S = C5
    cam = rt.final_camera(W / H)
    return {j: O.fast_render(o_scene(final_world), o_cam(cam), W, H, S, 50, SEED, row0=j, row_step=1, nrows=1)[0]
            for j in C5_ROWS}


@pytest.fixture(scope="module", params=["grid", "bvh"])
def config5(request, final_renderer):
    """BASELINE config 5: the final scene at 3840x2160 (16:9 camera, the
    reference's defocus blur), 2000 spp, whole frame on one GPU — through the
    product's default uniform grid and through the BVH."""
    W, H, S = C5
    cam = rt.final_camera(W / H)
    final_renderer.set_accel(request.param)
    try:
        img = final_renderer.render(cam, W, H, S, 50, SEED)
        sch = final_renderer.last_schedule()
    finally:
        final_renderer.set_accel("none")
    return request.param, cam, img, sch


def test_config5_sampled_rows_bit_exact_vs_oracle(config5, config5_oracle_rows):
    """Two full-width rows of config 5 (row 0 and row 1531: bottom and the
    spheres' band) against the oracle at full spp, bit for bit, with the grid
    (the default path) and with the BVH."""
    accel, cam, img, sch = config5
    assert sch["bvh"] == {"bvh": 1, "grid": 2}[accel] and sch["tile_w"] in (8, 16)
    for j in C5_ROWS:
        assert np.array_equal(img[j], config5_oracle_rows[j]), (accel, j)


def test_config5_strip_of_8_equals_frame_rows(config5, final_renderer):
    """One rank's interleaved 1/8 strip of config 5 (rows 3, 11, ..., 270
    rows) rendered alone equals those rows of the whole frame; and the frame
    is finite, fully covered and at the expected brightness."""
    torch = pytest.importorskip("torch")
    accel, cam, img, _ = config5
    W, H, S = C5
    G, g = 8, 3
    nrows = H // G
    strip = torch.full((nrows, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
    final_renderer.set_accel(accel)
    try:
        final_renderer.render_rows(cam, W, H, S, 50, SEED, g, G, nrows, strip.data_ptr(), 0)
        final_renderer.synchronize()
        assert final_renderer.last_schedule()["bvh"] == {"bvh": 1, "grid": 2}[accel]
    finally:
        final_renderer.set_accel("none")
    assert np.array_equal(strip.cpu().numpy(), img[g::G])
    assert np.isfinite(img).all() and (img.reshape(H, -1).max(axis=1) > 0).all()
    mean = float(img.mean() / S)
    record_parity_stats(f"config5_frame_{accel}", {"mean_radiance": mean, "rows_checked_vs_oracle": "0, 1531",
                                                    "strip": "3 of 8"})
    assert 0.3 < mean < 0.9


def test_config5_every_64th_row_mean_matches_independent_oracle(config5, final_world):
    """The whole config-5 frame beyond its two bit-exact rows (VERDICT r04
    item 6): the mean radiance of every 64th row (34 rows x 3 channels) of
    the 2000-spp frame against the oracle's fast-mode render of the same rows
    at 64 spp under two other seeds, each within 5 sigma, sigma being the
    noise the oracle's own seed-to-seed difference measures for that row
    (O.row_mean_z), and the chi-square per row near 1.  Independent samples
    (other seeds), so this checks every sampled row statistically; camera and
    scene are the reference's at 16:9 (main.cpp:292-360)."""
    accel, cam, img, _ = config5
    W, H, S = C5
    rows = list(range(0, H, 64))
    sc, oc = o_scene(final_world), o_cam(cam)
    a = O.fast_render(sc, oc, W, H, 64, 50, 7, row0=0, row_step=64, nrows=len(rows))
    b = O.fast_render(sc, oc, W, H, 64, 50, 8, row0=0, row_step=64, nrows=len(rows))
    z, chi2 = O.row_mean_z(img[rows], S, a, b, 64)
    record_parity_stats(f"config5_row_means_{accel}", {"rows": len(rows), "max_abs_z": float(np.abs(z).max()),
                                                       "chi2_per_dof": float(chi2)})
    assert np.abs(z).max() < 5.0, (accel, np.abs(z).max(), np.unravel_index(np.abs(z).argmax(), z.shape))
    assert chi2 < 2.0, (accel, chi2)


def test_default_accel_is_grid(final_world):
    """A new context renders through the uniform grid (the fastest structure;
    same image as brute force): rt_render, the reference's surface, gets it."""
    r = rt.Renderer(final_world, 0)
    try:
        r.render(rt.final_camera(1.5), 24, 16, 2, 50, SEED)
        assert r.last_schedule()["bvh"] == 2
    finally:
        r.close()


@pytest.mark.parametrize("G", [2, 3, 4, 8])
def test_config3_strips_unpermute_to_config2_frame(G, config2, final_world):
    """BASELINE config 3's partition on one GPU: every rank's interleaved
    strip of config 2 (rank g renders rows g, g+G, ...; dist.strip_rows),
    rendered through the default (grid) path and un-permuted as rank 0 does
    after the gather (dist.unpermute), equals the one-GPU frame bit for bit —
    G = 3 leaves a ragged last strip (800 = 3 x 267 - 1)."""
    torch = pytest.importorskip("torch")
    from a_dive_into_ray_tracing_amd import dist as rdist

    cam, img = config2
    W, H, S = 1200, 800, 500
    r = rt.Renderer(final_world, 0)
    strips = []
    try:
        for g in range(G):
            row0, step, nrows = rdist.strip_rows(H, g, G)
            s = torch.full((nrows, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
            r.render_rows(cam, W, H, S, 50, SEED, row0, step, nrows, s.data_ptr(), 0)
            r.synchronize()
            assert r.last_schedule()["bvh"] == 2
            strips.append(s.cpu().numpy())
    finally:
        r.close()
    assert all(not s[-1].any() for s in strips[H % G or G:]), "rows past H must be zero-filled"
    assert np.array_equal(rdist.unpermute(strips, H), img)


def test_concurrent_contexts_with_different_scenes_and_paths():
    """Contexts run concurrently on their own streams (as bench.py's two
    contexts do), here with different scenes and closest-hit paths at once:
    the final scene through the LDS grid, the learn scene brute force, and a
    2 000-sphere scene through the grid in global memory, each launched
    several times back to back without synchronising; every image equals its
    oracle render."""
    torch = pytest.importorskip("torch")
    g = np.random.default_rng(5)
    n = 2000
    c = np.column_stack([g.uniform(-20, 20, n), np.full(n, 0.2), g.uniform(-20, 20, n)])
    kinds = g.integers(0, 3, n).astype(np.int32)
    params = np.column_stack([g.uniform(0.1, 0.9, (n, 3)), np.where(kinds == 2, 1.5, g.uniform(0, 0.5, n))])
    big = rt.World(np.vstack([[0, -1000, 0, 1000], np.column_stack([c, np.full(n, 0.2)])]),
                   np.concatenate([[0], kinds]).astype(np.int32), np.vstack([[0.5, 0.5, 0.5, 0], params]))
    W, H, S = 40, 24, 8
    jobs = [(rt.random_scene(), rt.final_camera(W / H), "grid"), (rt.learn_scene(), rt.learn_camera(W / H), "none"),
            (big, rt.camera((20, 3, 12), (0, 0, 0), (0, 1, 0), 30.0, W / H, 0.05, 20.0), "grid")]
    rs, outs, streams = [], [], []
    try:
        for world, cam, accel in jobs:
            r = rt.Renderer(world, 0)
            r.set_accel(accel)
            rs.append(r)
            streams.append(torch.cuda.Stream("cuda:0"))
            outs.append([torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(3)])
        for k in range(3):
            for i, (world, cam, _) in enumerate(jobs):
                rs[i].render_rows(cam, W, H, S, 50, SEED, 0, 1, H, outs[i][k].data_ptr(), streams[i].cuda_stream)
        torch.cuda.synchronize()
        paths = [r.last_schedule()["bvh"] for r in rs]
    finally:
        for r in rs:
            r.close()
    assert paths == [2, 0, 4], paths
    for i, (world, cam, _) in enumerate(jobs):
        want = O.fast_render(o_scene(world), o_cam(cam), W, H, S, 50, SEED)
        for k in range(3):
            assert np.array_equal(outs[i][k].cpu().numpy(), want), (i, k)


def test_overlapped_contexts_strips_equal_frame(config2, final_world):
    """bench.py --pipeline 2: two contexts with the overlap hint
    (rt_ctx_set_overlap: fewer, longer work items) render the 8 strips of
    config 2 on two streams, enqueued back to back so their launches run
    concurrently; the un-permuted strips are the one-GPU frame bit for bit."""
    torch = pytest.importorskip("torch")
    from a_dive_into_ray_tracing_amd import dist as rdist

    cam, img = config2
    W, H, S, G = 1200, 800, 500, 8
    rs = [rt.Renderer(final_world, 0) for _ in range(2)]
    streams = [torch.cuda.Stream("cuda:0") for _ in range(2)]
    strips, chunks = [], set()
    try:
        for x in rs:
            x.set_overlap(True)
        for g in range(G):
            row0, step, nrows = rdist.strip_rows(H, g, G)
            s = torch.full((nrows, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
            rs[g % 2].render_rows(cam, W, H, S, 50, SEED, row0, step, nrows, s.data_ptr(), streams[g % 2].cuda_stream)
            chunks.add(rs[g % 2].last_schedule()["chunk"])
            strips.append(s)
        torch.cuda.synchronize()
        assert rt.load().rt_ctx_set_overlap(rs[0]._h, 2) == -1  # RT_EINVAL: the hint is 0 or 1
    finally:
        for x in rs:
            x.close()
    assert chunks == {63}, chunks  # ~15 k items of >= 63 samples (the single-launch default: 21)
    assert np.array_equal(rdist.unpermute([s.cpu().numpy() for s in strips], H), img)


def test_bench_plain_run_dumps_the_timed_image(config2, tmp_path):
    """A plain `bench.py --steps 3 --warmup 1 --dump-outputs DIR` prints one
    line with the headline fields and none of the --full legs, and
    DIR/image.npy is the image its last timed step rendered (step 3 of the
    steps alternating over two contexts and buffers): the config-2 frame,
    bit for bit."""
    import json
    import subprocess
    import sys

    _, img = config2
    p = subprocess.run([sys.executable, os.path.join(O.REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f32" and d["unit"] == "Msamples/s"
    assert d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - 1200 * 800 * 500 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    assert d["one_shot"] is None and d["roofline"]["brute_force"] is None and "cpu_baseline" not in d
    assert d["roofline"]["achieved"] is None and d["roofline"]["kernel_ms"] > 0
    assert os.listdir(tmp_path / "out") == ["image.npy"]
    got = np.load(tmp_path / "out" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)


@pytest.mark.parametrize("which", [0, 1], ids=["sqrt", "reciprocal"])
def test_exact_math_exhaustive(which):
    """The kernels' short correctly rounded sqrt and reciprocal (rtmi_path.h
    sqrt_cr / rcp_cr: v_sqrt_f32 / v_rcp_f32 plus an exact-residual
    correction) equal the compiler's IEEE lowering — and so glibc's sqrtf
    and the division the oracle computes — for every one of the 2^32 float
    bit patterns (zeros, denormals, infinities and NaNs included)."""
    f = rt.load().rt_debug_exact_math
    f.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    v = (C.c_uint64 * 4)()
    rt.check(f(which, v), "rt_debug_exact_math")
    assert v[0] == 0, f"{v[0]} mismatches; first input {v[1]:#010x}: got {v[2]:#010x}, IEEE {v[3]:#010x}"


def test_max_depth_range(final_renderer):
    """max_depth must lie in [0, 2^24): the kernels keep a path's depth in 24
    bits (its pixel above them).  The largest value renders like any deep
    limit (every path ends long before it); 2^24 is rejected."""
    cam = rt.final_camera(16 / 8)
    deep = final_renderer.render(cam, 16, 8, 4, (1 << 24) - 1, SEED)
    assert np.array_equal(deep, final_renderer.render(cam, 16, 8, 4, 100000, SEED))
    with pytest.raises(rt.RTError) as e:
        final_renderer.render(cam, 16, 8, 4, 1 << 24, SEED)
    assert "RT_EINVAL" in str(e.value)
