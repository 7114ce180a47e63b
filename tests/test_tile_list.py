"""Tile lists of the grid kernel's primary batches, on the
host alone: rt_debug_tile_list runs the very test the kernel runs
(tile_bundle / tile_may_hit) and returns each tile's list as scene indices.

The check is independent of the bound: camera rays are built in numpy
float64 from the camera formulas (camera.h:56-62) — lens points on the
disk's rim at 16 angles and its centre, through the tile's four (s, t)
corners, edge midpoints and centre at the extreme jitters, and 200 seeded
random rays of the tile's own pixels — and every small sphere any of them
meets at any t > 0 (discriminant >= 0 and a positive root, not only the
closest hit) must be in the tile's list.  A tile over the cap has no list
(count -1: its batches walk the grid) and nothing to check."""
import ctypes as C

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
from test_grid_strides import stacked_scene

CAP = 32
BIG_FACTOR = 4  # RTMI_BIG_FACTOR: spheres over 4 x the median radius stay brute force


def tile_lists(world, cam, W, H, row0=0, row_step=1, nrows=None, tile_w=0, cap=CAP):
    """(indices [tiles, cap], counts [tiles], tile width) of every tile of the strip."""
    L = rt.load()
    L.rt_debug_tile_list.restype = C.c_int
    nrows = H if nrows is None else nrows
    nvalid = min(nrows, (H - row0 + row_step - 1) // row_step)
    tw = tile_w or rt.auto_tile_w(W, nvalid)
    th = 64 // tw
    tiles = -(-W // tw) * -(-nvalid // th)
    idx, cnt = np.full((tiles, cap), -1, np.int32), np.zeros(tiles, np.int32)
    sc = world.c_struct()
    ip = C.POINTER(C.c_int32)
    rc = L.rt_debug_tile_list(C.byref(sc), C.byref(cam), C.c_int32(W), C.c_int32(H), C.c_int32(row0), C.c_int32(row_step),
                              C.c_int32(nrows), C.c_int32(tile_w), C.c_int32(-1), C.c_int32(cap), idx.ctypes.data_as(ip),
                              cnt.ctypes.data_as(ip))
    assert rc == 0, L.rt_last_error()
    return idx, cnt, tw


def small_spheres(world):
    cr = np.asarray(world.center_radius, np.float64).reshape(-1, 4)
    rad = np.abs(cr[:, 3])
    med = np.sort(rad)[len(rad) // 2]
    return np.flatnonzero(rad <= BIG_FACTOR * med), cr


LENS = np.array([[0.0, 0.0]] + [[np.cos(a), np.sin(a)] for a in 2 * np.pi * np.arange(16) / 16])
GRID9 = np.array([[a, b] for a in (0.0, 0.5, 1.0) for b in (0.0, 0.5, 1.0)])


def check_strip(world, cam, W, H, row0=0, row_step=1, nrows=None, tile_w=0, seed=5):
    """Every tile of the strip; returns the counts (-1: over the cap)."""
    idx, cnt, tw = tile_lists(world, cam, W, H, row0, row_step, nrows, tile_w)
    nrows = H if nrows is None else nrows
    nvalid = min(nrows, (H - row0 + row_step - 1) // row_step)
    th, tiles_x = 64 // tw, -(-W // tw)
    small, cr = small_spheres(world)
    c, r = cr[small, :3], np.abs(cr[small, 3])
    # hb = (o - c).d and cc = |o - c|^2 - r^2 for unit d, each as one product
    hb_m = np.vstack([-c.T, np.ones(len(small))])
    cc_m = np.vstack([-2 * c.T, (c * c).sum(1) - r * r, np.ones(len(small))])
    v = lambda name: np.array(getattr(cam, name), np.float64)
    org, llc, hor, ver, cu, cv, lens = v("origin"), v("lower_left_corner"), v("horizontal"), v("vertical"), v("u"), v("v"), cam.lens_radius
    g = np.random.default_rng(seed)
    for t in range(len(cnt)):
        if cnt[t] < 0:
            continue
        ty, tx = divmod(t, tiles_x)
        x0, y0 = tx * tw, ty * th
        vw, vh = min(tw, W - x0), min(th, nvalid - y0)
        j_lo, j_hi = row0 + y0 * row_step, row0 + (y0 + vh - 1) * row_step
        # the structured rays: every lens point through every (s, t) point
        st = np.array([x0 / (W - 1), j_lo / (H - 1)]) + GRID9 * np.array([vw / (W - 1), (j_hi + 1 - j_lo) / (H - 1)])
        lp, sp = np.repeat(LENS, len(st), 0), np.tile(st, (len(LENS), 1))
        # the random rays: a pixel of the tile, a jitter, a lens point in the disk
        n = 200
        i = x0 + g.integers(0, vw, n) + g.random(n)
        j = row0 + (y0 + g.integers(0, vh, n)) * row_step + g.random(n)
        rr, ph = np.sqrt(g.random(n)), 2 * np.pi * g.random(n)
        lp = np.vstack([lp, np.column_stack([rr * np.cos(ph), rr * np.sin(ph)])])
        sp = np.vstack([sp, np.column_stack([i / (W - 1), j / (H - 1)])])
        off = lens * (lp[:, :1] * cu + lp[:, 1:] * cv)
        o = org + off
        d = llc + sp[:, :1] * hor + sp[:, 1:] * ver - org - off
        d /= np.sqrt((d * d).sum(1))[:, None]
        hb = np.column_stack([d, (o * d).sum(1)]) @ hb_m
        cc = np.column_stack([o, np.ones(len(o)), (o * o).sum(1)]) @ cc_m
        # disc >= 0 and the larger root (-hb + sqrt(disc)) positive: hb < 0, or the origin inside
        met = ((hb * hb - cc >= 0) & ((hb < 0) | (cc < 0))).any(0)
        missing = set(small[met]) - set(idx[t, :cnt[t]])
        assert not missing, (t, (x0, y0, vw, vh), sorted(missing), sorted(idx[t, :cnt[t]]))
    return cnt


def aperture2_camera(aspect):
    return rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, aspect, 2.0, 10.0)


def inside_camera(aspect):
    """Inside the layer of small spheres, spheres around and behind it."""
    return rt.camera((0.5, 0.2, 0.5), (4, 0.3, 1), (0, 1, 0), 60.0, aspect, 0.05, 3.0)


def test_final_scene_small_image():
    w = rt.random_scene()
    cnt = check_strip(w, rt.final_camera(48 / 32), 48, 32)
    assert (cnt > 0).any() and (cnt < 0).any()  # (tiles this large in space: the dense rows are over the cap)


def test_config2_every_tile():
    """The flagship frame, 1200 x 800 in 8 x 8 tiles: no tile over the cap, and
    at least a quarter of the tiles with an empty list."""
    w = rt.random_scene()
    cnt = check_strip(w, rt.final_camera(1200 / 800), 1200, 800)
    assert len(cnt) == 15000 and (cnt >= 0).all(), (len(cnt), int((cnt < 0).sum()))
    assert (cnt == 0).mean() >= 0.25, (cnt == 0).mean()
    print(f"config 2: mean {cnt.mean():.2f} max {cnt.max()} empty {(cnt == 0).mean():.3f}")


@pytest.mark.parametrize("tile_w", [16, 8])
def test_one_rank_strip(tile_w):
    """One rank's 1/8 strip of config 2 (rows 3, 11, ...: a tile's rows lie 8
    apart); in the automatic 16 x 4 tiles no tile is over the cap."""
    w = rt.random_scene()
    assert rt.auto_tile_w(1200, 100) == 16
    cnt = check_strip(w, rt.final_camera(1200 / 800), 1200, 800, row0=3, row_step=8, nrows=100, tile_w=tile_w)
    if tile_w == 16:
        assert (cnt >= 0).all(), int((cnt < 0).sum())
    print(f"strip {tile_w}: mean {cnt[cnt >= 0].mean():.2f} max {cnt.max()} over the cap {(cnt < 0).sum()}")


def test_partial_last_tile():
    w = rt.random_scene()
    cnt = check_strip(w, rt.final_camera(13 / 120), 13, 120, tile_w=8)  # tiles of 8 and 5 columns
    assert len(cnt) == 30 and (cnt >= 0).all() and (cnt > 0).any()


def test_learn_scene_wide_aperture():
    cnt = check_strip(rt.learn_scene(), rt.learn_camera(32 / 18), 32, 18)
    assert (cnt >= 0).any()


def test_aperture_2():
    """A lens disk of radius 1: bundles so wide that every tile of the final
    scene is over the cap (the walk runs); the learn scene's few spheres fit."""
    cnt = check_strip(rt.random_scene(), aperture2_camera(48 / 32), 48, 32)
    assert (cnt < 0).all()
    cnt = check_strip(rt.learn_scene(), aperture2_camera(48 / 32), 48, 32)
    assert (cnt >= 0).all() and (cnt > 0).any()


def test_camera_inside_the_layer():
    w = rt.random_scene()
    cnt = check_strip(w, inside_camera(48 / 32), 48, 32)
    assert (cnt > 0).any()


def test_stacked_scene():
    """A grid of several y layers (the general walk's scene)."""
    cam = rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 40.0, 48 / 32, 0.1, 10.0)
    cnt = check_strip(stacked_scene(), cam, 48, 32)
    assert (cnt >= 0).any()


def test_one_tile_equals_its_entry_of_all_tiles_and_the_cap_marks_no_list():
    w = rt.random_scene()
    cam = rt.final_camera(48 / 32)
    idx, cnt, _ = tile_lists(w, cam, 48, 32)
    L, sc, ip = rt.load(), w.c_struct(), C.POINTER(C.c_int32)
    for t in (0, 7, len(cnt) - 1):
        one, n = np.full(CAP, -1, np.int32), np.zeros(1, np.int32)
        assert L.rt_debug_tile_list(C.byref(sc), C.byref(cam), 48, 32, 0, 1, 32, 0, t, CAP, one.ctypes.data_as(ip),
                                    n.ctypes.data_as(ip)) == 0
        assert n[0] == cnt[t] and np.array_equal(one, idx[t])
    for cap in (1, 2):
        _, small_cnt, _ = tile_lists(w, cam, 48, 32, cap=cap)
        assert np.array_equal(small_cnt, np.where(cnt <= cap, cnt, -1))
    assert L.rt_debug_tile_list(C.byref(sc), C.byref(cam), 48, 32, 0, 1, 32, 0, len(cnt), CAP, idx.ctypes.data_as(ip),
                                cnt.ctypes.data_as(ip)) != 0
