"""The Next-Week denoiser on the GPU: the filter against the float64 model
(tests/nw_denoise_model.py), the feature buffers against rt_nw_debug_trace, and
the driver end to end."""
import numpy as np
import pytest

import nw_denoise_model as M
from a_dive_into_ray_tracing_amd import nextweek as nw
from conftest import record_parity_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def box():
    s, cam = nw.preset(6, aspect=1.0)
    r = nw.NwRenderer(s)
    yield r, cam
    r.close()


def inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros((H, W, 8), np.float32)
    f[..., :3] = rng.random((H, W, 3)) * 0.9
    n = rng.normal(size=(H, W, 3))
    f[..., 3:6] = n / np.linalg.norm(n, axis=-1, keepdims=True) * (0.9 + 0.1 * rng.random((H, W, 1)))
    f[:, : W // 2, 3:6] = (0.0, 0.0, 1.0)
    f[..., 6] = 3.0 + 0.05 * np.arange(W)[None, :] + 0.1 * rng.random((H, W))
    f[..., 7] = rng.random((H, W)) > 0.1
    col = (rng.random((H, W, 3)) * 1.5).astype(np.float32)
    var = (rng.random((H, W)) * 0.02).astype(np.float32)
    return col, var, f


@pytest.mark.parametrize("W,H", [(37, 21), (17, 16), (16, 16), (1, 1)])
@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_filter_equals_the_model(box, W, H, iterations):
    """GPU output against the float64 model, within 8 x the model's own float32
    deviation: with and without the variance, with and without demodulation, a
    +inf-variance pixel, and a NaN colour that passes through and is no tap."""
    r, _ = box
    col, var, f = inputs(H, W, 100 * W + iterations)
    if W > 1:
        var[H // 2, W // 3] = np.inf
        col[H // 3, W // 2] = np.nan
    for v in (var, None):
        for flags in (M.DEMODULATE, 0):
            want, tol = M.tolerance(col, v, f, iterations=iterations, flags=flags)
            got = r.denoise(col, v, f, iterations=iterations, demodulate=bool(flags))
            ok = np.isfinite(want)
            assert np.array_equal(np.isfinite(got), ok)
            err = float(np.abs(got.astype(np.float64) - want)[ok].max(initial=0.0))
            print(f"{W}x{H} it {iterations} var {v is not None} flags {flags}: err {err:.3e} tol {tol:.3e}")
            assert err <= tol
            if W > 1:
                bad = got[H // 3, W // 2]
                assert np.isnan(bad).all()


def test_right_angle_edge_is_exact(box):
    """Changing one side's colours changes no output bit on the other side (no variance: any number of levels)."""
    r, _ = box
    H, W = 21, 37
    col, _, f = inputs(H, W, 7)
    f[:, W // 2:, 3:6] = (1.0, 0.0, 0.0)
    other = col.copy()
    other[:, W // 2:] *= 3.0
    a, b = r.denoise(col, None, f, iterations=5), r.denoise(other, None, f, iterations=5)
    assert np.array_equal(a[:, : W // 2], b[:, : W // 2]) and not np.array_equal(a[:, W // 2:], b[:, W // 2:])
    # with the variance guide: the first level (later ones couple the sides through the 3 x 3 mean of the filtered v')
    var = np.full((H, W), 0.01, np.float32)
    a, b = r.denoise(col, var, f, iterations=1), r.denoise(other, var, f, iterations=1)
    assert np.array_equal(a[:, : W // 2], b[:, : W // 2]) and not np.array_equal(a[:, W // 2:], b[:, W // 2:])


@pytest.mark.parametrize("flags", [M.DEMODULATE, 0])
def test_filtered_variance_equals_the_model(box, flags):
    """var_out (the pass kernel's v'_out, the finish kernel's rescale, the host copy) against the float64 model,
    within 8 x the model's float32 deviation; a +inf variance stays +inf."""
    r, _ = box
    H, W = 21, 37
    col, var, f = inputs(H, W, 11)
    var[5, 7] = np.inf
    for it in (1, 4):
        _, want = M.denoise(col, var, f, np.float64, iterations=it, flags=flags)
        _, v32 = M.denoise(col, var, f, np.float32, iterations=it, flags=flags)
        _, got = r.denoise(col, var, f, var_out=True, iterations=it, demodulate=bool(flags))
        ok = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), ok) and np.isposinf(got[5, 7])
        tol = 8.0 * float(np.abs(v32.astype(np.float64)[ok] - want[ok]).max())
        err = float(np.abs(got.astype(np.float64)[ok] - want[ok]).max())
        print(f"var_out it {it} flags {flags}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)


def test_cli_denoise_and_aov(box, tmp_path):
    """--denoise --aov writes every file at the image's size, the AOVs equal NwRenderer.features, the filtered
    image differs from the noisy one; --out without --denoise equals the Python render's quantisation."""
    import os
    import subprocess

    import a_dive_into_ray_tracing_amd as rt

    exe = os.path.join(os.path.dirname(rt.__file__), "bin", "rtmi_nw_render")
    base = [exe, "--scene", "cornell_box", "--width", "64", "--height", "64", "--spp", "32"]
    pre = str(tmp_path / "aov")
    subprocess.run(base + ["--denoise", "--aov", pre, "--out", str(tmp_path / "dn.ppm"), "--pfm", str(tmp_path / "dn.pfm")],
                   check=True, capture_output=True, timeout=120)
    planes = {k: read_pfm(f"{pre}_{k}.pfm") for k in ("albedo", "normal", "depth", "noisy")}
    dn = read_pfm(tmp_path / "dn.pfm")
    assert all(p.shape == (64, 64, 3) for p in planes.values()) and dn.shape == (64, 64, 3)
    assert open(tmp_path / "dn.ppm", "rb").read().split()[:4] == [b"P3", b"64", b"64", b"255"]
    r, cam = box
    feat = r.features(cam, 64, 64, fspp=16, seed=1984)
    assert np.array_equal(planes["albedo"], feat[..., :3]) and np.array_equal(planes["normal"], feat[..., 3:6])
    assert np.array_equal(planes["depth"], np.repeat(feat[..., 6:7], 3, axis=2))
    sums = r.render(cam, 64, 64, 32)
    assert np.array_equal(planes["noisy"], sums / np.float32(32))  # (threshold 0: the plain render of 32 samples)
    assert not np.array_equal(dn, planes["noisy"]) and np.isfinite(dn).all()
    # without --denoise: the output a build without the feature writes, P3 int(255.99 sqrt(mean)), top row first
    subprocess.run(base + ["--out", str(tmp_path / "plain.ppm")], check=True, capture_output=True, timeout=120)
    tok = open(tmp_path / "plain.ppm", "rb").read().split()
    assert tok[:4] == [b"P3", b"64", b"64", b"255"]
    want = (255.99 * np.sqrt(sums / np.float32(32)).astype(np.float64)).astype(np.int64)[::-1]
    assert np.array_equal(np.array(tok[4:], np.int64).reshape(64, 64, 3), want)


def fixed_sum(vals, lo, hi):
    tot = 0
    for v in vals:
        v = float(v)
        v = 0.0 if v != v else min(max(v, lo), hi)
        tot += int(v * 4294967296.0)  # (exact in float64; int() truncates toward zero)
    return tot


def test_features_equal_the_traced_first_hits(box):
    """n, z and cov of every pixel, bit for bit, from segment 0 of debug_trace of every (i, j, s)."""
    r, cam = box
    W, H, fspp = 12, 10, 3
    feat = r.features(cam, W, H, fspp=fspp, seed=77)
    for j in range(H):
        for i in range(W):
            ns, ts = [], []
            for s in range(fspp):
                seg, ids = r.debug_trace(cam, W, H, i, j, s, seed=77, cap=1)
                if ids[0, 0] >= 0:
                    ns.append(seg[0, 7:10])
                    ts.append(seg[0, 6])
            for c in range(3):
                want = np.float32(fixed_sum([n[c] for n in ns], -64.0, 64.0) * 2.0 ** -32 / fspp)
                assert feat[j, i, 3 + c] == want, (i, j, c)
            z = np.float32(fixed_sum(ts, 0.0, 2.0 ** 20) * 2.0 ** -32 / len(ts)) if ts else np.float32(0)
            assert feat[j, i, 6] == z and feat[j, i, 7] == np.float32(len(ts) / fspp), (i, j)
    assert ((feat[..., :3] >= 0) & (feat[..., :3] <= 64)).all()


def test_denoised_render_is_closer_to_the_reference(box):
    r, cam = box
    W = H = 96
    ref = r.render(cam, W, H, 2048) / 2048
    mean, n, err, filt = r.adaptive(cam, W, H, 16, 64, 16, 0.05, denoise=True)
    m2, n2, e2 = r.adaptive(cam, W, H, 16, 64, 16, 0.05)
    assert np.array_equal(mean, m2) and np.array_equal(n, n2) and np.array_equal(err, e2)
    noisy, clean = M.rmse(mean, ref), M.rmse(filt, ref)
    print(f"rmse noisy {noisy:.5f} filtered {clean:.5f} ratio {clean / noisy:.3f}")
    record_parity_stats("nw_denoise_cornell_96", {"rmse_noisy": noisy, "rmse_filtered": clean, "ratio": clean / noisy})
    assert clean < noisy
