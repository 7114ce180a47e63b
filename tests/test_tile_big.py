"""The big spheres in the tile lists, on the host alone:
rt_debug_tile_big runs the test the kernel's list build runs on the big
slots (tile_bundle / tile_may_hit on {centre, grown radius}) and returns, per
tile, the big spheres the kernel appends to the tile's list — the only big
spheres a primary batch of that tile then tests.

The check is test_tile_list.py's, on the big spheres: float64 camera rays of
each tile (the same lens points, the same (s, t) points, 200 seeded random
rays of the tile's own pixels), and every big sphere any of them meets at any
t > 0 must be in the tile's set.  A scene of more than 8 big spheres has no
such sets (count -1 in every tile: its batches run the big group as before)."""
import ctypes as C

import numpy as np
import pytest

import a_dive_into_ray_tracing_amd as rt
from test_grid_strides import stacked_scene
from test_tile_list import BIG_FACTOR, GRID9, LENS, aperture2_camera, inside_camera

BIG_MAX = 8  # kTileBigMax


def tile_big(world, cam, W, H, row0=0, row_step=1, nrows=None, tile_w=0, tile=-1):
    """(indices [tiles, 8], counts [tiles], tile width) of every tile of the strip (or of one tile)."""
    L = rt.load()
    L.rt_debug_tile_big.restype = C.c_int
    nrows = H if nrows is None else nrows
    nvalid = min(nrows, (H - row0 + row_step - 1) // row_step)
    tw = tile_w or rt.auto_tile_w(W, nvalid)
    th = 64 // tw
    tiles = -(-W // tw) * -(-nvalid // th) if tile < 0 else 1
    idx, cnt = np.full((tiles, BIG_MAX), -1, np.int32), np.zeros(tiles, np.int32)
    sc = world.c_struct()
    ip = C.POINTER(C.c_int32)
    rc = L.rt_debug_tile_big(C.byref(sc), C.byref(cam), C.c_int32(W), C.c_int32(H), C.c_int32(row0), C.c_int32(row_step),
                             C.c_int32(nrows), C.c_int32(tile_w), C.c_int32(tile), idx.ctypes.data_as(ip),
                             cnt.ctypes.data_as(ip))
    assert rc == 0, L.rt_last_error()
    return idx, cnt, tw


def big_spheres(world):
    cr = np.asarray(world.center_radius, np.float64).reshape(-1, 4)
    rad = np.abs(cr[:, 3])
    med = np.sort(rad)[len(rad) // 2]
    return np.flatnonzero(rad > BIG_FACTOR * med), cr


def check_strip(world, cam, W, H, row0=0, row_step=1, nrows=None, tile_w=0, seed=5):
    """Every tile of the strip; returns (indices, counts)."""
    idx, cnt, tw = tile_big(world, cam, W, H, row0, row_step, nrows, tile_w)
    nrows = H if nrows is None else nrows
    nvalid = min(nrows, (H - row0 + row_step - 1) // row_step)
    th, tiles_x = 64 // tw, -(-W // tw)
    big, cr = big_spheres(world)
    assert 0 < len(big) <= BIG_MAX and (cnt >= 0).all(), (len(big), cnt.min())
    c, r = cr[big, :3], np.abs(cr[big, 3])
    v = lambda name: np.array(getattr(cam, name), np.float64)
    org, llc, hor, ver, cu, cv, lens = v("origin"), v("lower_left_corner"), v("horizontal"), v("vertical"), v("u"), v("v"), cam.lens_radius
    g = np.random.default_rng(seed)
    for t in range(len(cnt)):
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
        # per sphere from o - c (the ground's |c|^2 is 1e6: no expanded form here)
        oc = o[:, None, :] - c[None, :, :]
        hb = (oc * d[:, None, :]).sum(2)
        cc = (oc * oc).sum(2) - r * r
        # disc >= 0 and the larger root (-hb + sqrt(disc)) positive: hb < 0, or the origin inside
        met = ((hb * hb - cc >= 0) & ((hb < 0) | (cc < 0))).any(0)
        missing = set(big[met]) - set(idx[t, :cnt[t]])
        assert not missing, (t, (x0, y0, vw, vh), sorted(missing), sorted(idx[t, :cnt[t]]))
    # the sets name big spheres, in scene order
    for t in range(len(cnt)):
        row = idx[t, :cnt[t]]
        assert set(row) <= set(big) and (np.diff(row) > 0).all(), (t, row)
    return idx, cnt


def test_config2_every_tile():
    """The flagship frame, 1200 x 800 in 8 x 8 tiles.  The sets must be small,
    so that listing everything cannot pass: a float64 run of the same bound
    gives a mean of 1.30 big spheres a tile and 10.1 % of the tiles with none."""
    w = rt.random_scene()
    idx, cnt = check_strip(w, rt.final_camera(1200 / 800), 1200, 800)
    big, _ = big_spheres(w)
    share = [float((idx == k).any(1).mean()) for k in big]
    print(f"config 2: mean {cnt.mean():.3f} empty {(cnt == 0).mean():.4f} only one {(cnt == 1).mean():.4f} per sphere "
          + " ".join(f"{k}:{s:.4f}" for k, s in zip(big, share)))
    assert len(cnt) == 15000 and len(big) == 4
    assert cnt.mean() <= 2.0, cnt.mean()
    assert (cnt == 0).mean() >= 0.05, (cnt == 0).mean()


@pytest.mark.parametrize("tile_w", [16, 8])
def test_one_rank_strip(tile_w):
    """One rank's 1/8 strip of config 2 (rows 3, 11, ...: a tile's rows lie 8 apart)."""
    w = rt.random_scene()
    _, cnt = check_strip(w, rt.final_camera(1200 / 800), 1200, 800, row0=3, row_step=8, nrows=100, tile_w=tile_w)
    print(f"strip {tile_w}: mean {cnt.mean():.3f} empty {(cnt == 0).mean():.4f}")


def test_partial_last_tile():
    _, cnt = check_strip(rt.random_scene(), rt.final_camera(13 / 120), 13, 120, tile_w=8)  # tiles of 8 and 5 columns
    assert len(cnt) == 30 and (cnt > 0).any()


def test_aperture_2():
    """A lens disk of radius 1.  Focused 10 away (test_tile_list's camera) the
    bundle's k stays below 1 and the sets are only checked; focused 0.9 away
    the lens is wider than the focus plane is far, k >= 1, and the test must
    pass everything."""
    check_strip(rt.random_scene(), aperture2_camera(48 / 32), 48, 32)
    near = rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 48 / 32, 2.0, 0.9)
    _, cnt = check_strip(rt.random_scene(), near, 48, 32)
    assert (cnt == 4).all(), cnt


def test_camera_inside_the_layer():
    _, cnt = check_strip(rt.random_scene(), inside_camera(48 / 32), 48, 32)
    assert (cnt > 0).all()  # on the ground, looking along it: the ground is met from every tile


def test_camera_inside_a_big_sphere():
    """From inside the glass sphere at (0, 1, 0): every ray leaves through it."""
    w = rt.random_scene()
    big, cr = big_spheres(w)
    glass = [k for k in big if np.allclose(cr[k], (0, 1, 0, 1))]
    assert len(glass) == 1
    cam = rt.camera((0.2, 1.1, 0.3), (4, 1, 0), (0, 1, 0), 50.0, 48 / 32, 0.05, 3.0)
    idx, cnt = check_strip(w, cam, 48, 32)
    assert (idx == glass[0]).any(1).all()


def many_big_scene(nbig, seed=11):
    """The ground, nbig - 1 spheres of radius 0.85 to 0.97 and 40 small ones."""
    g = np.random.default_rng(seed)
    n = 40
    small = np.column_stack([g.uniform(-5, 5, n), np.full(n, 0.2), g.uniform(-5, 5, n), np.full(n, 0.2)])
    large = [[-6 + 1.7 * i, 1.0, -2 + 0.9 * (i % 3), 0.85 + 0.03 * (i % 5)] for i in range(nbig - 1)]
    cr = np.vstack([[0, -1000, 0, 1000], small[:20], np.array(large).reshape(-1, 4), small[20:]])
    kinds = np.zeros(len(cr), np.int32)
    params = np.full((len(cr), 4), 0.5)
    return rt.World(cr, kinds, params)


def test_eight_big_spheres_have_sets_and_nine_have_none():
    cam = rt.final_camera(48 / 32)
    w8 = many_big_scene(8)
    assert len(big_spheres(w8)[0]) == 8
    _, cnt = check_strip(w8, cam, 48, 32)
    assert (cnt > 0).any()
    w9 = many_big_scene(9)
    assert len(big_spheres(w9)[0]) == 9
    _, cnt, _ = tile_big(w9, cam, 48, 32)
    assert (cnt == -1).all(), cnt


def test_stacked_scene():
    """A grid of several y layers (the general walk's scene).  Its radii spread
    over a factor of 45, so dozens of its spheres are big: no sets.  The ground
    and the spheres of radius 0.1 to 0.35 alone (none of them big) have them."""
    cam = rt.camera((13, 2, 3), (0, 0, 0), (0, 1, 0), 40.0, 48 / 32, 0.1, 10.0)
    w = stacked_scene()
    big, cr = big_spheres(w)
    assert len(big) > BIG_MAX
    _, cnt, _ = tile_big(w, cam, 48, 32)
    assert (cnt == -1).all(), cnt
    keep = np.flatnonzero((cr[:, 3] >= 0.1) & (cr[:, 3] <= 0.35) | (cr[:, 3] == 1000))
    w1 = rt.World(cr[keep], w.mat_kind[keep], w.mat_params[keep])
    assert len(big_spheres(w1)[0]) == 1
    _, cnt = check_strip(w1, cam, 48, 32)
    assert (cnt > 0).any()


def test_one_tile_equals_its_entry_of_all_tiles():
    w = rt.random_scene()
    cam = rt.final_camera(48 / 32)
    idx, cnt, _ = tile_big(w, cam, 48, 32)
    for t in (0, 7, len(cnt) - 1):
        one, n, _ = tile_big(w, cam, 48, 32, tile=t)
        assert n[0] == cnt[t] and np.array_equal(one[0], idx[t])
    L, sc, ip = rt.load(), w.c_struct(), C.POINTER(C.c_int32)
    assert L.rt_debug_tile_big(C.byref(sc), C.byref(cam), 48, 32, 0, 1, 32, 0, len(cnt), idx.ctypes.data_as(ip),
                               cnt.ctypes.data_as(ip)) != 0
