"""Adaptive sampling of the Next-Week renderer, the host half (no device):
rt_nw_adapt_criterion against a numpy float64 restatement of the formula in
include/rtmi_nw.h, the argument checks that need no device, and
rt_nw_adapt_info on hand-written files, and that host code under ASan + UBSan in
a program of its own (tests/native/nw_adaptive_sanitize.cpp)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import test_nw_progressive as TP
from a_dive_into_ray_tracing_amd import _abi, nextweek as nw
from a_dive_into_ray_tracing_amd._abi import RTError

EINVAL, EIO = -1, -7  # include/rtmi.h
ONE = 1 << 32  # 1.0 as a 2^-32 fixed-point colour value
MAX_SPP = 1 << 20


def criterion_ref(s, m2, n, min_spp, max_spp, threshold, floor, dilate):
    """The header's formula, per pixel in float64 and in its order, then the dilation: (mask, err, count)."""
    n64 = n.astype(np.float64)
    S = s[..., 0] + s[..., 1] + s[..., 2]  # int64: exact
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = S.astype(np.float64) * 2.0 ** -32 / n64
        ex2 = m2.astype(np.float64) * 2.0 ** -28 / n64
        var = np.maximum(0.0, ex2 - mean * mean) * n64 / (n64 - 1.0)
        err = np.sqrt(var / n64) / np.maximum(mean, floor)
    err = np.where(n < 2, np.inf, err)
    raw = (n < max(min_spp, 2)) | (((err > threshold) | (threshold == 0)) & (n < max_spp))  # (0 cannot be met)
    H, W = n.shape
    out = np.zeros_like(raw)
    for y in range(H):
        for x in range(W):
            out[y, x] = raw[max(0, y - dilate):y + dilate + 1, max(0, x - dilate):x + dilate + 1].any()
    out &= n < max_spp
    return out.astype(np.uint8), err, int(out.sum())


def synthetic():
    """9 x 7 pixels: random noisy pixels plus every special case the criterion has to get right."""
    g = np.random.default_rng(5)
    H, W = 7, 9
    n = g.integers(40, 200, (H, W)).astype(np.int32)
    mean_ch = g.uniform(0.05, 2.0, (H, W))  # per channel
    s = np.zeros((H, W, 3), np.int64)
    m2 = np.zeros((H, W), np.uint64)
    for y in range(H):
        for x in range(W):
            k = int(n[y, x])
            f = int(mean_ch[y, x] * ONE)
            s[y, x] = [k * f, k * f, k * f]
            spread = float(g.uniform(1.0, 1.5))  # E[l^2] = spread * E[l]^2
            m2[y, x] = int(k * ((3 * f) >> 18) ** 2 * spread)
    n[0, 0] = 0  # no sample at all
    s[0, 0], m2[0, 0] = 0, 0
    n[0, 1] = 1  # one sample: no variance estimate
    s[0, 1], m2[0, 1] = ONE // 2, ((3 * (ONE // 2)) >> 18) ** 2
    n[0, 2] = 10  # below min_spp (16), tiny error otherwise
    s[0, 2], m2[0, 2] = 10 * ONE, 10 * ((3 * ONE) >> 18) ** 2
    n[3, 4] = 64  # zero variance: 64 equal samples
    s[3, 4], m2[3, 4] = 64 * ONE, 64 * ((3 * ONE) >> 18) ** 2
    n[3, 5] = 64  # under the floor: channel sum 0.003 with a large relative spread
    s[3, 5], m2[3, 5] = 64 * (ONE // 1000), int(64 * ((3 * (ONE // 1000)) >> 18) ** 2 * 10)
    n[6, 8] = 256  # at max_spp in the corner, still noisy
    s[6, 8], m2[6, 8] = 256 * ONE, 256 * ((3 * ONE) >> 18) ** 2 * 9
    n[5, 7] = 64  # ... and next to it a clean pixel, then a noisy one: dilation must skip the pixel at the maximum
    s[5, 7], m2[5, 7] = 64 * ONE, 64 * ((3 * ONE) >> 18) ** 2
    n[6, 7] = 64
    s[6, 7], m2[6, 7] = 64 * ONE, 64 * ((3 * ONE) >> 18) ** 2 * 30
    n[2, 0] = MAX_SPP  # the accumulator's limit, every sample at the brightest value: m2 near 2^63
    s[2, 0] = MAX_SPP * 64 * ONE
    m2[2, 0] = MAX_SPP * ((3 * 64 * ONE) >> 18) ** 2
    assert 1 << 62 < int(m2[2, 0]) < 1 << 64
    return s, m2, n


@pytest.mark.parametrize("dilate", [0, 1, 2, 50])
@pytest.mark.parametrize("threshold", [0.0, 0.02, 0.05, 0.2])
def test_criterion_equals_the_float64_restatement(threshold, dilate):
    s, m2, n = synthetic()
    for max_spp in (256, MAX_SPP):
        want_mask, want_err, want_count = criterion_ref(s, m2, n, 16, max_spp, threshold, 0.03, dilate)
        mask, err, count = nw.adapt_criterion(s, m2, n, 16, max_spp, threshold, 0.03, dilate)
        assert np.array_equal(mask, want_mask)
        assert np.array_equal(err, want_err)  # inf where n < 2, bit for bit elsewhere
        assert count == want_count == int(mask.sum())


def test_criterion_special_cases():
    s, m2, n = synthetic()
    raw, err, _ = nw.adapt_criterion(s, m2, n, 16, 256, 0.05, 0.03, 0)
    assert raw[0, 0] and raw[0, 1] and np.isinf(err[0, 0]) and np.isinf(err[0, 1])  # n = 0, n = 1
    assert raw[0, 2] and err[0, 2] == 0.0  # below min_spp although clean
    assert not raw[3, 4] and err[3, 4] == 0.0  # zero variance
    rel = err[3, 5] * 0.03 / 0.003  # the pixel under the floor: relative to its own mean the error is large ...
    assert 0.3 < rel < 0.45 and 0 < err[3, 5] < 0.05 and not raw[3, 5]  # ... but it is judged against the floor
    assert err[6, 8] > 0.05 and not raw[6, 8]  # noisy, but at max_spp
    assert not raw[5, 7] and raw[6, 7]
    assert not raw[2, 0] and np.isfinite(err[2, 0]) and err[2, 0] < 1e-3  # m2 near 2^63, read as unsigned
    dil, _, count = nw.adapt_criterion(s, m2, n, 16, 256, 0.05, 0.03, 1)
    assert dil[5, 7] and dil[6, 7] and not dil[6, 8]  # spread onto the clean neighbour, never onto the pixel at the maximum
    assert dil[1, 0] and dil[1, 1] and dil[0, 0] and count == dil.sum() > raw.sum()  # ... and it stops at the border
    assert (dil >= raw).all()
    # with the accumulator's own limit as max_spp the noisy corner is active again
    assert nw.adapt_criterion(s, m2, n, 16, MAX_SPP, 0.05, 0.03, 0)[0][6, 8]
    # a threshold of 0 cannot be met, not even by the pixels without variance: everything below the maximum
    zero, err0, _ = nw.adapt_criterion(s, m2, n, 0, 256, 0.0, 0.03, 0)
    assert np.array_equal(zero != 0, n < 256) and zero[3, 4] and err0[3, 4] == 0.0
    tiny = nw.adapt_criterion(s, m2, n, 0, 256, 1e-300, 0.03, 0)[0]
    assert np.array_equal(tiny != 0, (n < 256) & ((n < 2) | (err0 > 0))) and not tiny[3, 4]


def test_criterion_argument_checks():
    s, m2, n = synthetic()

    def refused(*a):
        with pytest.raises(RTError) as e:
            nw.adapt_criterion(s, m2, n, *a)
        assert e.value.code == EINVAL

    refused(-1, 256, 0.05)
    refused(300, 256, 0.05)  # min_spp above max_spp
    refused(0, 1, 0.05)  # a variance needs two samples
    refused(16, MAX_SPP + 1, 0.05)
    refused(16, 256, -0.1)
    refused(16, 256, float("nan"))
    refused(16, 256, 0.05, 0.0)  # floor
    refused(16, 256, 0.05, float("inf"))
    refused(16, 256, 0.05, 0.03, -1)  # dilate
    bad = n.copy()
    bad[4, 4] = -3
    with pytest.raises(RTError):
        nw.adapt_criterion(s, m2, bad, 16, 256, 0.05)
    L = _abi.load()
    act = np.zeros(n.shape, np.uint8)
    a8 = act.ctypes.data_as(C.POINTER(C.c_uint8))
    ptrs = (s.ctypes.data_as(C.POINTER(C.c_int64)), m2.ctypes.data_as(C.POINTER(C.c_uint64)), n.ctypes.data_as(C.POINTER(C.c_int32)))
    assert L.rt_nw_adapt_criterion(None, ptrs[1], ptrs[2], 9, 7, 16, 256, 0.05, 0.03, 1, a8, None, None) == EINVAL
    assert L.rt_nw_adapt_criterion(ptrs[0], None, ptrs[2], 9, 7, 16, 256, 0.05, 0.03, 1, a8, None, None) == EINVAL
    assert L.rt_nw_adapt_criterion(ptrs[0], ptrs[1], None, 9, 7, 16, 256, 0.05, 0.03, 1, a8, None, None) == EINVAL
    assert L.rt_nw_adapt_criterion(*ptrs, 9, 7, 16, 256, 0.05, 0.03, 1, None, None, None) == EINVAL
    assert L.rt_nw_adapt_criterion(*ptrs, 0, 7, 16, 256, 0.05, 0.03, 1, a8, None, None) == EINVAL
    assert L.rt_nw_adapt_criterion(*ptrs, 9, 7, 16, 256, 0.05, 0.03, 1, a8, None, None) == 0  # err and the count are optional


def test_null_arguments_of_the_device_entry_points():
    L = _abi.load()
    cam = nw.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40, 1.0, 0.0, 5.0)
    assert L.rt_nw_adapt_reset(None, 8, 8) == EINVAL
    assert L.rt_nw_adapt_pass(None, C.byref(cam), 8, 8, 1, 50, 1, 0, 1, 8, None, None) == EINVAL
    assert L.rt_nw_adapt_export(None, None, None, None, 0) == EINVAL
    assert L.rt_nw_adapt_import(None, None, None, None, 0) == EINVAL
    assert L.rt_nw_adapt_resolve(None, None, None, None) == EINVAL
    assert L.rt_nw_adapt_save(None, b"x", None, C.byref(cam), 8, 0, 1, 50, 1) == EINVAL
    assert L.rt_nw_adapt_load(None, b"x", None, C.byref(cam), 8, 8, 0, 1, 8, 50, 1) == EINVAL
    assert L.rt_nw_render_adaptive(None, None, C.byref(cam), 8, 8, 4, 8, 4, 0.05, 0.03, 1, 50, 1, None, -1.0, None, None, None,
                                   None, _abi.NW_ADAPT_ON_PASS(), None) == EINVAL
    assert L.rt_nw_adapt_info(None, None, None) == EINVAL


# ---- checkpoint files ---------------------------------------------------------------------
def header(magic, W=3, H=2, nrows=2, spp_done=5):
    return magic + struct.pack("<8i3Q", W, H, 0, 1, nrows, spp_done, 50, 0, 1984, 0x1122334455667788, 0x99AABBCCDDEEFF00)


def body(npix):
    return (np.arange(npix * 3, dtype="<i8").tobytes() + np.arange(npix, dtype="<u8").tobytes()
            + np.full(npix, 5, "<i4").tobytes())


def test_adapt_info_on_hand_written_files(tmp_path):
    good = tmp_path / "good.ckpt"
    good.write_bytes(header(b"RTMINWD1") + body(6))
    info = nw.adapt_info(good)
    assert (info["W"], info["H"], info["row0"], info["row_step"], info["nrows"], info["spp_done"], info["max_depth"]) == (3, 2, 0, 1, 2, 5, 50)
    assert (info["seed"], info["scene_hash"], info["camera_hash"]) == (1984, 0x1122334455667788, 0x99AABBCCDDEEFF00)
    with pytest.raises(RTError) as e:  # an adaptive checkpoint is no progressive one
        nw.accum_info(good)
    assert e.value.code == EIO

    def refused(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(RTError) as e:
            nw.adapt_info(p)
        assert e.value.code == EIO, name

    whole = header(b"RTMINWD1") + body(6)
    refused("short_header.ckpt", whole[:40])
    refused("truncated.ckpt", whole[:-4])
    refused("header_only.ckpt", whole[:64])
    refused("overlong.ckpt", whole + b"\0")
    refused("foreign.ckpt", header(b"NOTACKPT") + body(6))
    refused("one_weekend.ckpt", header(b"RTMIACC1") + body(6))
    prog = tmp_path / "progressive.ckpt"  # a progressive checkpoint, valid as such
    prog.write_bytes(header(b"RTMINWA1") + np.arange(18, dtype="<i8").tobytes())
    assert nw.accum_info(prog)["spp_done"] == 5
    with pytest.raises(RTError, match="adaptive checkpoint") as e:
        nw.adapt_info(prog)
    assert e.value.code == EIO
    with pytest.raises(RTError) as e:
        nw.adapt_info(tmp_path / "missing.ckpt")
    assert e.value.code == EIO


# ---- the sanitizer program -----------------------------------------------------------------------
def test_criterion_and_checkpoint_code_under_asan_ubsan(tmp_path):
    """`make asan-adaptive`: tests/native/nw_adaptive_sanitize.cpp (its own main;
    nothing is preloaded) with the host sources under -fsanitize=address,undefined
    — the criterion on strips from 1 x 1 up with every dilation, checkpoint files
    written, read back, cut short, lengthened, mislabelled and with a lying header."""
    if not os.path.exists(TP.CLANG) or not TP._sanitizer_runtime_present(tmp_path):
        pytest.skip("the compiler lacks the sanitizer runtime")
    san_dir = tmp_path / "asan"
    subprocess.run(["make", "-C", TP.CSRC, "asan-adaptive", f"SAN_DIR={san_dir}"], check=True, capture_output=True, timeout=900)
    work = tmp_path / "files"
    work.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS="suppressions=" + os.path.join(TP.REPO, "tests", "native", "lsan.supp"),
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(san_dir / "nw_adaptive_sanitize"), str(work)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "all checks passed" in p.stdout
    assert os.listdir(work) == []
