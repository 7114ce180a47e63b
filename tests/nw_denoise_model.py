"""Float64 restatement of the Next-Week denoiser (include/rtmi_nw.h "Denoising";
DESIGN.md §9 "Denoising"): the yardstick of tests/test_nw_denoise*.py.

Plain numpy over whole images, one shifted copy per tap; `dt` selects the
precision every formula runs in.  With dt=np.float32 the same formulas run in
single precision, which is how the tests form their tolerances (8 x the largest
float32 deviation of the model from itself, the rule of tests/nw_truth.py).
"""
import numpy as np

DEMODULATE, NO_EDGES = 1, 2
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, flags=DEMODULATE)


def _shift(a, ox, oy, fill=0):
    """b[y, x] = a[y + oy, x + ox] where that lies in the image, and the mask of those places."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ok = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        ok[y0:y1, x0:x1] = True
    return b, ok


def albedo(feat, flags, dt):
    a = np.fmax(feat[..., :3].astype(dt), dt(0.01)) if flags & DEMODULATE else np.ones(feat.shape[:2] + (3,), dt)
    return a, ((a[..., 0] + a[..., 1]) + a[..., 2]) / dt(3)


def depth_slope(feat, dt):
    z, cov = feat[..., 6].astype(dt), feat[..., 7]
    g = []
    for ox, oy in ((1, 0), (0, 1)):
        zl, okl = _shift(z, -ox, -oy)
        zh, okh = _shift(z, ox, oy)
        okl &= _shift(cov, -ox, -oy)[0] > 0
        okh &= _shift(cov, ox, oy)[0] > 0
        g.append(np.where(okl & okh, (zh - zl) * dt(0.5), np.where(okh, zh - z, np.where(okl, z - zl, dt(0)))))
    return np.maximum(np.abs(g[0]), np.abs(g[1]))


def one_pass(c, v, n, z, gz, step, have_var, p, dt):
    """One a-trous level: (c', v') -> (c'_out, v'_out)."""
    H, W = z.shape
    edges = not (p["flags"] & NO_EDGES)
    with np.errstate(all="ignore"):
        c_ok = np.isfinite(c).all(axis=-1)
        v_ok = np.isfinite(v)
        lum = edges and have_var
        inv_sd = None
        if lum:
            sv, sk = np.zeros((H, W), dt), np.zeros((H, W), dt)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, ok = _shift(v, dx, dy)
                    ok &= np.isfinite(vq)
                    k = dt((0.25 if dx else 0.5) * (0.25 if dy else 0.5))
                    sv += np.where(ok, k * np.where(ok, vq, 0), 0)
                    sk += np.where(ok, k, 0)
            vt = np.maximum(sv / np.where(sk > 0, sk, 1), 0)
            inv_sd = dt(1) / (dt(p["sigma_l"]) * np.sqrt(vt) + dt(1e-6))
        lsum = (c[..., 0] + c[..., 1]) + c[..., 2]
        wc = dt(9 / 64)
        sw = np.full((H, W), wc, dt)
        sc = wc * np.where(c_ok[..., None], c, 0)
        s2 = np.where(v_ok, wc * wc * np.where(v_ok, v, 0), 0)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                cq, ok = _shift(c, dx * step, dy * step)
                vq, _ = _shift(v, dx * step, dy * step)
                ok &= np.isfinite(cq).all(axis=-1) & np.isfinite(vq)
                w = np.full((H, W), dt(H5[dx + 2] * H5[dy + 2]), dt)
                if edges:
                    nq, _ = _shift(n, dx * step, dy * step)
                    zq, _ = _shift(z, dx * step, dy * step)
                    dn = n - nq
                    arg = dt(p["sigma_n"] / 2) * ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2])
                    arg = arg + np.abs(z - zq) / (dt(p["sigma_z"]) * gz * dt(step) * dt(max(abs(dx), abs(dy)))
                                                  + dt(1e-3) * np.abs(z) + dt(1e-12))
                    if lum:
                        lq = (cq[..., 0] + cq[..., 1]) + cq[..., 2]
                        arg = arg + np.where(v_ok, np.abs(lsum - lq) * inv_sd, 0)
                    w = w * np.exp(-arg)
                    ok &= np.isfinite(w)
                w = np.where(ok, w, 0).astype(dt)
                sw += w
                sc += w[..., None] * np.where(ok[..., None], cq, 0)
                s2 += w * w * np.where(ok, vq, 0)
        c_out = np.where(c_ok[..., None], sc / sw[..., None], c)
        v_out = np.where(c_ok, np.where(v_ok, s2 / (sw * sw), v), v)
    return c_out.astype(dt), v_out.astype(dt)


def denoise(color, var, feat, dt=np.float64, **params):
    """(out [H, W, 3], var_out [H, W]) in precision dt; var may be None."""
    p = dict(DEFAULTS, **params)
    color, feat = np.asarray(color), np.asarray(feat)
    with np.errstate(all="ignore"):
        a, abar = albedo(feat, p["flags"], dt)
        c = color.astype(dt) / a
        v = np.zeros(color.shape[:2], dt) if var is None else np.asarray(var).astype(dt) / (abar * abar)
        n, z = feat[..., 3:6].astype(dt), feat[..., 6].astype(dt)
        gz = depth_slope(feat, dt)
        for k in range(p["iterations"]):
            c, v = one_pass(c, v, n, z, gz, 1 << k, var is not None, p, dt)
        return c * a, v * (abar * abar)


def tolerance(color, var, feat, **params):
    """(float64 result, 8 x the largest deviation of the float32 evaluation from it), over the finite outputs."""
    want, _ = denoise(color, var, feat, np.float64, **params)
    got, _ = denoise(color, var, feat, np.float32, **params)
    ok = np.isfinite(want)
    return want, 8.0 * float(np.abs(got.astype(np.float64) - want)[ok].max(initial=0.0))


def transfer(img):
    """The PPM's clamped square-root transfer."""
    return np.sqrt(np.clip(np.asarray(img, np.float64), 0.0, 1.0))


def rmse(a, b):
    return float(np.sqrt(np.mean((transfer(a) - transfer(b)) ** 2)))
