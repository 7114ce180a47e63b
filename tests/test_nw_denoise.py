"""The Next-Week denoiser without a GPU: the float64 model of the filter
(tests/nw_denoise_model.py) on synthetic inputs, the variance guide
(rt_nw_adapt_variance) against the criterion, the parameter checks, and the
host-only code under the sanitizers as a program of its own
(tests/native/nw_denoise_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nw_denoise_model as M
import test_nw_progressive as TP
from a_dive_into_ray_tracing_amd import _abi, nextweek as nw
from a_dive_into_ray_tracing_amd._abi import RTError

EINVAL = -1
ONE = 1 << 32


def features(H, W, rng, normal=(0.0, 0.0, 1.0)):
    f = np.zeros((H, W, 8), np.float32)
    f[..., :3] = rng.random((H, W, 3)) * 0.9 + 0.05
    f[..., 3:6] = normal
    f[..., 6] = 3.0 + 0.01 * np.arange(W)[None, :] + 0.02 * np.arange(H)[:, None]
    f[..., 7] = 1.0
    return f


# ---- the model alone ---------------------------------------------------------------------------
def test_constant_colour_is_kept():
    """A constant colour with arbitrary features comes back within 32 * 2^-24
    relative in the model's float32 evaluation: 25 positive terms and a division."""
    rng = np.random.default_rng(1)
    H, W = 19, 23
    f = features(H, W, rng)
    f[..., 3:6] = rng.normal(size=(H, W, 3))
    f[..., 6] = rng.random((H, W)) * 10
    f[..., 7] = rng.random((H, W)) > 0.2
    col = np.broadcast_to(np.float32([0.3, 0.55, 0.8]), (H, W, 3)).copy()
    var = (rng.random((H, W)) * 0.01).astype(np.float32)
    out, _ = M.denoise(col, var, f, np.float32, flags=0)
    assert np.abs(out / col - 1).max() <= 32 * 2.0 ** -24
    # demodulated: the constant is the demodulated colour, c / A
    a = np.maximum(f[..., :3], np.float32(0.01))
    out, _ = M.denoise(col * a, var, f, np.float32, iterations=3)
    assert np.abs(out / (col * a) - 1).max() <= 34 * 2.0 ** -24  # (and the two roundings of / A and * A)


def b3_blur(img, iterations):
    """The separable B3 a-trous blur computed independently: taps outside skipped, renormalised."""
    out = img.astype(np.float64)
    H, W = out.shape[:2]
    for k in range(iterations):
        step = 1 << k
        acc, wsum = np.zeros_like(out), np.zeros((H, W))
        for y in range(H):
            for x in range(W):
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        yy, xx = y + dy * step, x + dx * step
                        if 0 <= yy < H and 0 <= xx < W:
                            w = M.H5[dy + 2] * M.H5[dx + 2]
                            acc[y, x] += w * out[yy, xx]
                            wsum[y, x] += w
        out = acc / wsum[..., None]
    return out


def test_no_edges_is_the_b3_blur():
    rng = np.random.default_rng(2)
    H, W = 9, 11
    col = rng.random((H, W, 3)).astype(np.float32)
    out, _ = M.denoise(col, None, features(H, W, rng), flags=M.NO_EDGES, iterations=3)
    assert np.abs(out - b3_blur(col, 3)).max() < 1e-13


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_nothing_crosses_a_right_angle_edge(dt):
    """Two half-planes with normals 90 degrees apart: each side's output does not
    depend on the other side's colours — without a variance guide for any number
    of levels, with one for the first level.  From the second level on the guide
    itself couples the sides: vt_p is a 3 x 3 mean of the filtered v', which
    reaches across the edge, and the far side's v' was filtered with weights
    that depend on its colours (measured in float64: 4.8e-3 after two levels)."""
    rng = np.random.default_rng(3)
    H, W = 12, 16
    f = features(H, W, rng)
    f[:, W // 2:, 3:6] = (1.0, 0.0, 0.0)
    col = rng.random((H, W, 3)).astype(np.float32)
    var = np.full((H, W), 0.01, np.float32)
    other = col.copy()
    other[:, W // 2:] = rng.random((H, W - W // 2, 3)) * 5
    for v, it in ((None, 3), (var, 1)):
        a, _ = M.denoise(col, v, f, dt, iterations=it)
        b, _ = M.denoise(other, v, f, dt, iterations=it)
        assert np.array_equal(a[:, :W // 2], b[:, :W // 2])
        assert not np.array_equal(a[:, W // 2:], b[:, W // 2:])


def test_variance_of_a_flat_region():
    """Unit edge weights, one pass, away from the border: var_out = (sum h^4 over the 25 taps) * var."""
    rng = np.random.default_rng(4)
    H, W = 9, 9
    col = rng.random((H, W, 3)).astype(np.float32)
    var = np.full((H, W), 0.25, np.float32)
    _, v = M.denoise(col, var, features(H, W, rng), flags=M.NO_EDGES, iterations=1)
    h4 = sum((a * b) ** 2 for a in M.H5 for b in M.H5)
    assert abs(v[4, 4] / 0.25 - h4) < 1e-14


def test_infinite_variance_and_nan_colour():
    rng = np.random.default_rng(5)
    H, W = 9, 9
    f = features(H, W, rng)
    col = rng.random((H, W, 3)).astype(np.float32)
    var = np.full((H, W), 1e-4, np.float32)
    var[4, 4] = np.inf
    col[2, 6] = np.nan
    out, v = M.denoise(col, var, f, iterations=2, flags=0)
    assert np.isnan(out[2, 6]).all() and np.isfinite(np.delete(out.reshape(-1, 3), 2 * W + 6, axis=0)).all()
    assert np.isinf(v[4, 4]) and np.isfinite(out[4, 4]).all()
    # the pixel without a variance is filtered by the features alone: as with no variance anywhere
    free, _ = M.denoise(col, None, f, iterations=1, flags=0)
    one, _ = M.denoise(col, var, f, iterations=1, flags=0)
    assert np.array_equal(one[4, 4], free[4, 4]) and not np.array_equal(one[4, 5], free[4, 5])
    assert np.isfinite(one).sum() == one.size - 3


# ---- rt_nw_adapt_variance ---------------------------------------------------------------------------
def moments(rng, H, W, nmax=40):
    n = rng.integers(2, nmax, (H, W)).astype(np.int32)
    s = (rng.random((H, W, 3)) * n[..., None] * ONE).astype(np.int64)
    mean = s.sum(-1) / ONE / n
    m2 = ((mean ** 2 * (1 + rng.random((H, W)))) * n * 2.0 ** 28).astype(np.uint64)
    return s, m2, n


def test_variance_against_the_criterion():
    rng = np.random.default_rng(6)
    s, m2, n = moments(rng, 7, 13)
    floor = 0.03
    _, err, _ = nw.adapt_criterion(s, m2, n, 2, 64, 0.1, floor)
    mean = s.sum(-1).astype(np.float64) * 2.0 ** -32 / n
    want = (err * np.maximum(mean, floor)) ** 2
    got = nw.adapt_variance(s, m2, n)
    assert got.dtype == np.float32 and got.shape == n.shape
    assert np.abs(got - want).max() <= np.abs(want).max() * 2.0 ** -22  # float rounding of the result and of err^2


def test_variance_edges():
    s = np.zeros((1, 4, 3), np.int64)
    m2 = np.zeros((1, 4), np.uint64)
    n = np.int32([[0, 1, 2, 1 << 20]])
    s[0, 2:] = ONE
    m2[0, 2:] = np.iinfo(np.uint64).max
    v = nw.adapt_variance(s, m2, n)
    assert np.isposinf(v[0, :2]).all() and np.isfinite(v[0, 2:]).all() and (v[0, 2:] > 0).all()
    ex2 = float(np.iinfo(np.uint64).max) * 2.0 ** -28 / 2
    assert v[0, 2] == np.float32(max(0.0, ex2 - 1.5 ** 2) / 1.0)
    n[0, 0] = -1
    with pytest.raises(RTError) as e:
        nw.adapt_variance(s, m2, n)
    assert e.value.code == EINVAL


def test_params_are_checked():
    p = nw.denoise_params()
    assert (p.iterations, p.sigma_l, p.sigma_n, p.sigma_z, p.flags) == (5, 4.0, 128.0, 1.0, 1)
    assert nw.denoise_params(demodulate=False, no_edges=True).flags == 2
    for bad in (dict(iterations=0), dict(iterations=9), dict(sigma_l=0.0), dict(sigma_n=-1.0), dict(sigma_z=float("inf")),
                dict(sigma_l=float("nan"))):
        with pytest.raises(RTError) as e:
            nw.denoise_params(**bad)
        assert e.value.code == EINVAL, bad
    L = _abi.load()
    assert L.rt_nw_denoise_params_check(None) == EINVAL
    z = np.zeros(24, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert L.rt_nw_denoise_host(None, 1, 1, z, None, z, None, z, None) == EINVAL
    assert L.rt_nw_denoise(None, 1, 1, None, None, None, None, None, None, None) == EINVAL
    assert L.rt_nw_render_features(None, None, 1, 1, 1, 1, None, None, None) == EINVAL


def test_host_code_under_asan_ubsan(tmp_path):
    """`make asan-denoise`: tests/native/nw_denoise_sanitize.cpp (its own main; nothing is preloaded)."""
    if not os.path.exists(TP.CLANG) or not TP._sanitizer_runtime_present(tmp_path):
        pytest.skip("the compiler lacks the sanitizer runtime")
    san_dir = tmp_path / "asan"
    subprocess.run(["make", "-C", TP.CSRC, "asan-denoise", f"SAN_DIR={san_dir}"], check=True, capture_output=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS="suppressions=" + os.path.join(TP.REPO, "tests", "native", "lsan.supp"),
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(san_dir / "nw_denoise_sanitize")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "all checks passed" in p.stdout


# ---- quality of the model on real noise ---------------------------------------------------------
def test_model_reduces_the_error_of_an_oracle_render():
    """Preset 6 (the Cornell box) from the oracle alone, 96 x 96: 16 samples per
    pixel (their per-sample values, as differences of the renders of 1 .. 16
    samples, give the mean and the variance of its channel sum), a 1024-spp
    reference, and features from the oracle's own trace (or_nw_trace, segment 0
    of sample 0; the scene's textures are solid, so the albedo is the winner's
    colour).  The float64 model's output must be closer to the reference than its
    input, on the PPM's clamped square-root transfer: a filter that cannot do that
    is broken.  Seen: RMSE 0.1812 noisy, 0.0657 filtered, ratio 0.363 (the print below)."""
    import nw_truth as T
    import oracle_py as O

    W = H = 96
    spp = 16
    s, cam = nw.preset(6, aspect=1.0)
    flat = s.flat()
    F = T.Flat(flat)
    assert (F.tex_kind == T.SOLID).all()
    ref = O.nw_render(flat, cam, W, H, 1024, 50, 1984)[0].astype(np.float64) / 1024
    cum = [np.zeros((H, W, 3))] + [O.nw_render(flat, cam, W, H, k, 50, 1984)[0].astype(np.float64) for k in range(1, spp + 1)]
    samples = np.stack([cum[k] - cum[k - 1] for k in range(1, spp + 1)])
    mean = samples.mean(axis=0)
    var = samples.sum(axis=-1).var(axis=0, ddof=1) / spp
    feat = np.zeros((H, W, 8), np.float32)
    for j in range(H):
        for i in range(W):
            seg, ids = O.nw_trace(flat, cam, W, H, 50, 1984, i, j, 0, cap=1)
            k = ids[0, 0]
            if k < 0:
                feat[j, i, :3] = F.bg
                continue
            m = F.mat_of[k]
            feat[j, i, :3] = 1.0 if F.mat_kind[m] == T.DIELECTRIC else F.tex_rgb[F.mat_tex[m]]
            feat[j, i, 3:6], feat[j, i, 6], feat[j, i, 7] = seg[0, 7:10], seg[0, 6], 1.0
    out, _ = M.denoise(mean.astype(np.float32), var.astype(np.float32), feat)
    noisy, clean = M.rmse(mean, ref), M.rmse(out, ref)
    print(f"oracle preset 6 96x96x16: rmse noisy {noisy:.4f} filtered {clean:.4f} ratio {clean / noisy:.3f}")
    assert clean < noisy
