"""rt_nw_render_features on the GPU: every pixel of the feature buffers re-formed
in Python integers from the first segment of rt_nw_debug_trace of every camera
sample (o, d, t, winner, time) and rt_nw_debug_records on those rays (n, u, v,
p, material), through all five walks of the validation kernels.

The segment's medium key is not part of a trace, so the test restates the
sample's random stream (xoroshiro128+ from splitmix64, csrc/rtmi_path.h Xoro):
pixel jitter, lens, time, then the key.  The restated time must equal the
traced one bit for bit, which pins the order and number of the draws."""
import numpy as np
import pytest

import nw_affine_util as AU
import nw_mixed_util as MX
import nw_motion_util as MU
import nw_truth as T
from a_dive_into_ray_tracing_amd import nextweek as nw

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SEED = 4711


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Xoro:
    def __init__(self, seed, pixel, sample):
        key = ((pixel << 24) | sample) & M64
        self.s0 = _mix64(seed ^ ((key * 0x9E3779B97F4A7C15) & M64))
        self.s1 = _mix64((self.s0 + 0x9E3779B97F4A7C15) & M64)

    def next(self):
        a, r = self.s0, (self.s0 + self.s1) & M64
        b = self.s1 ^ a
        self.s0 = (((a << 24) | (a >> 40)) ^ b ^ (b << 16)) & M64
        self.s1 = ((b << 37) | (b >> 27)) & M64
        return r


def time_and_key(cam, W, i, j, s, has_media):
    g = Xoro(SEED, j * W + i, s)
    g.next()  # the pixel jitter (pair)
    g.next()  # the lens (in_disk_direct's pair)
    uni = np.float32((g.next() >> 40) * 2.0 ** -24)
    t0, t1 = np.float32(cam.time0), np.float32(cam.time1)
    # fma(uni, t1 - t0, t0): the product of two floats is exact in float64
    time = np.float32(np.float64(uni) * np.float64(np.float32(t1 - t0)) + np.float64(t0))
    return time, (g.next() if has_media else 0)


def fixed(vals, lo, hi):
    tot = 0
    for v in vals:
        v = float(v)
        v = 0.0 if v != v else min(max(v, lo), hi)
        tot += int(v * 4294967296.0)  # (exact in float64; int() truncates toward zero)
    return tot


def check(r, scene, cam, W, H, fspp):
    """Every pixel: n, z, cov bit for bit; the albedo bit for bit where every
    sample's value is exact (background, dielectric, a solid texture, and any
    texture whose float32 and float64 evaluations agree to the bit), else within
    8 x the float32 deviation of nw_truth.texture_value summed over the pixel's
    samples.  A pixel with a sample at a texture discontinuity (nw_truth's ill
    flag, or its float32 run choosing another checker side or texel) has no
    albedo tolerance under that rule: those are counted, and must stay rare.
    Returns (pixels compared exactly, with a tolerance, left out, medium samples)."""
    F = T.Flat(scene.flat())
    has_media = bool((F.kind == T.KIND_NAMES.index("medium")).any())
    feat = r.features(cam, W, H, fspp=fspp, seed=SEED)
    rays, keys, win, ts = [], [], [], []
    for j in range(H):
        for i in range(W):
            for s in range(fspp):
                seg, ids, tm = r.debug_trace(cam, W, H, i, j, s, seed=SEED, cap=1, with_time=True)
                time, key = time_and_key(cam, W, i, j, s, has_media)
                assert time == tm, (i, j, s, time, tm)
                rays.append(list(seg[0, :6]) + [tm])
                keys.append(key)
                win.append(ids[0, 0])
                ts.append(seg[0, 6])
    rays, win, ts = np.asarray(rays, np.float32), np.asarray(win), np.asarray(ts, np.float32)
    idx, t, rec, mat = r.debug_records(rays, np.asarray(keys, np.uint64))
    assert np.array_equal(idx, win)  # the records are those of the traced hits
    hit = win >= 0
    assert np.array_equal(t[hit], ts[hit])
    medium = np.zeros(len(win), bool)
    if has_media and len(F.kind) > win.max():
        medium[hit] = F.kind[win[hit]] == T.KIND_NAMES.index("medium")
        assert (rec[medium, 3:6] == (1.0, 0.0, 0.0)).all() and (rec[medium, 6:8] == 0).all()
    recs = {"mat": np.where(hit, mat, -1), "u": rec[:, 6], "v": rec[:, 7], "p": rec[:, 0:3]}
    rgb64, br64, ill = T.material_value(F, recs, np.float64)
    rgb32, br32, _ = T.material_value(F, recs, np.float32)
    rgb64[~hit] = rgb32[~hit] = F.bg
    ill = (ill | (br64 != br32)) & hit
    dev = np.abs(rgb32.astype(np.float64) - rgb64)
    counts = [0, 0, 0, int(medium.sum())]
    for j in range(H):
        for i in range(W):
            k = (j * W + i) * fspp
            sel = slice(k, k + fspp)
            h = hit[sel]
            surf = h & ~medium[sel]
            for c in range(3):
                want = np.float32(fixed(rec[sel, 3 + c][surf], -64.0, 64.0) * 2.0 ** -32 / fspp)
                assert feat[j, i, 3 + c] == want, ("n", i, j, c)
            nh = int(h.sum())
            z = np.float32(fixed(ts[sel][h], 0.0, 2.0 ** 20) * 2.0 ** -32 / nh) if nh else np.float32(0)
            assert feat[j, i, 6] == z and feat[j, i, 7] == np.float32(nh / fspp), ("z, cov", i, j)
            if ill[sel].any():
                counts[2] += 1
                continue
            tol = 8.0 * dev[sel].sum(axis=0) / fspp
            if (tol == 0).all():
                counts[0] += 1
                for c in range(3):
                    want = np.float32(fixed(rgb32[sel, c], 0.0, 64.0) * 2.0 ** -32 / fspp)
                    assert feat[j, i, c] == want, ("albedo", i, j, c, feat[j, i, c], want)
            else:
                counts[1] += 1
                want = np.clip(rgb64[sel], 0.0, 64.0).sum(axis=0) / fspp
                # (and the truncation of each sample to 2^-32 and the rounding of the mean to float)
                assert (np.abs(feat[j, i, :3] - want) <= tol + 2.0 ** -30 + 2.0 ** -24 * want).all(), ("albedo", i, j)
    assert counts[2] <= 0.05 * W * H, counts
    return counts


def mixed(kind):
    if kind == "tri":
        return MX.mixed_scene(second_subdiv=1), MX.mixed_camera(24, 16), 1
    if kind == "attr":
        return MX.mixed_scene(attr=True, second_subdiv=1), MX.mixed_camera(24, 16), 2
    if kind == "shared":
        return MX.mixed_scene(shared=True, attr=True), MX.mixed_camera(24, 16), 3
    cam = nw.camera((2.0, 4.5, 15.0), (0.4, 0.4, 1.4), (0, 1, 0), 40, 24 / 16, 0.0, 10.0, 0.2, 0.8)
    if kind == "moving":
        return MU.scene_m("moving"), cam, 4
    return AU.scene_a().scene, cam, 5


@pytest.mark.parametrize("kind", ["tri", "attr", "shared", "moving", "affine"])
def test_features_are_exact_on_every_walk(kind):
    """24 x 16 with fspp = 3: the mixed scene (every object kind, triangles with
    and without attributes, placements) and the scenes with moving and affine
    placements, so that all five walks run; grid and BVH where the scene has a grid.
    (The second icosphere of the unshared mixed scenes is icosphere(1), as in the
    tests of the one-shot grid kernels: the grid then fits a block's LDS.)"""
    scene, cam, tri = mixed(kind)
    r = nw.NwRenderer(scene)
    try:
        assert r.scene_tri() == tri
        accels = ["bvh"] + (["grid"] if any(r.accel_info()["dims"]) else [])
        assert kind not in ("tri", "attr") or "grid" in accels
        for accel in accels:
            r.set_accel(accel)
            assert r.accel_info()["accel"] == accel
            counts = check(r, scene, cam, 24, 16, 3)
            print(kind, accel, "pixels exact / toleranced / left out, medium samples:", counts)
            assert counts[0] > 0
    finally:
        r.close()


def test_features_with_media():
    """cornell_smoke at 16 x 16 x 4: a sample whose winner is a medium contributes
    the medium's colour, a zero normal, t and coverage; all samples are checked."""
    scene, cam = nw.preset("cornell_smoke", aspect=1.0)
    r = nw.NwRenderer(scene)
    try:
        counts = check(r, scene, cam, 16, 16, 4)
        print("cornell_smoke: pixels exact / toleranced / left out, medium samples:", counts)
        assert counts[3] > 0 and counts[0] == 16 * 16  # (solid textures only)
    finally:
        r.close()
