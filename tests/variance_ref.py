"""Host statements of the second moment the render paths fold into colors[].w (option "moments") and of the variance read-out
(pt_read_variance), in float32 with an exactly rounded fmaf -- include/pt_api.h pins both."""
import ctypes as C
import ctypes.util

import numpy as np

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


def fmaf(a, b, c):
    """Element-wise fmaf (one rounding) over float32 arrays of one shape, through libm."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    out = np.empty(a.shape, np.float32)
    fa, fb, fc, fo = a.ravel(), b.ravel(), c.ravel(), out.reshape(-1)
    f = _libm.fmaf
    for i in range(fo.size):
        fo[i] = f(float(fa[i]), float(fb[i]), float(fc[i]))
    return out


def luminance(rgb):
    """l(c) = fmaf(0.0722f, c.b, fmaf(0.7152f, c.g, 0.2126f * c.r)) per row of an (n, >=3) float32 array."""
    rgb = np.asarray(rgb, np.float32)
    return fmaf(np.float32(0.0722), rgb[:, 2], fmaf(np.float32(0.7152), rgb[:, 1], np.float32(0.2126) * rgb[:, 0]))


def fold_moment(m2, x, s):
    """m2 = fmaf(m2, (float)s, q) / (float)(s + 1), q = l(x) * l(x): sample s of the running second moment."""
    l = luminance(x)
    return fmaf(m2, np.float32(s), l * l) / np.float32(s + 1)


def variance(colors, n):
    """v = fmaxf(fmaf(-mu, mu, m2), 0) / (float)(n - 1), mu = l(colors.xyz), +inf where n < 2."""
    colors = np.asarray(colors, np.float32)
    n = np.broadcast_to(np.asarray(n, np.int64), (colors.shape[0],))
    mu = luminance(colors)
    d = np.maximum(fmaf(-mu, mu, colors[:, 3]), np.float32(0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = d / np.maximum(n - 1, 1).astype(np.float32)
    return np.where(n < 2, np.float32(np.inf), v).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- the filter
def _lum64(x):
    return 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]


def variance_atrous_model(colors, variance, albedo_rgbm, normal_depth, W, H, iterations=2, sigma_luminance=4.0, sigma_normal=8.0,
                          sigma_depth=0.05, demodulate=0):
    """pt_denoise_variance (include/pt_api.h) in float64: (W*H, 4) float64, .xyz the filtered colour, .w the filtered variance."""
    from denoise_ref import KERNEL, _shift
    c = np.asarray(colors, dtype=np.float64)[:, :3].reshape(H, W, 3)
    v = np.asarray(variance, dtype=np.float64).reshape(H, W).copy()
    a = np.maximum(np.asarray(albedo_rgbm, dtype=np.float64)[:, :3].reshape(H, W, 3), 1e-3)
    la = np.maximum(_lum64(np.asarray(albedo_rgbm, dtype=np.float64)[:, :3].reshape(H, W, 3)), 1e-3)
    nd = np.asarray(normal_depth, dtype=np.float64).reshape(H, W, 4)
    n, z = nd[..., :3], nd[..., 3]
    miss = z < 0
    zero_n = np.all(n == 0, axis=-1)
    x = c / a if demodulate else c.copy()
    if demodulate:
        v = v / (la * la)
    gk = (0.25, 0.5, 0.25)
    for i in range(iterations):
        s = 1 << i
        gs = np.zeros((H, W))
        gw = np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, inside = _shift(v, dy, dx, 0.0)
                k = gk[dx + 1] * gk[dy + 1]
                gs += np.where(inside, k * vq, 0.0)
                gw += np.where(inside, k, 0.0)
        g = gs / gw
        lp = _lum64(x)
        num = np.zeros_like(x)
        vnum = np.zeros((H, W))
        den = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                xq, inside = _shift(x, s * dy, s * dx, 0.0)
                vq, _ = _shift(v, s * dy, s * dx, 0.0)
                if dx == 0 and dy == 0:
                    w = np.full((H, W), 9.0 / 64.0)
                else:
                    w = np.where(inside, KERNEL[dx + 2] * KERNEL[dy + 2], 0.0)
                    if np.isfinite(sigma_luminance):
                        dl = np.abs(lp - _lum64(xq))
                        with np.errstate(all="ignore"):
                            wl = np.exp(-dl / (float(sigma_luminance) * np.sqrt(g) + 1e-6))
                        w = w * np.where((dl == 0) | np.isinf(g), 1.0, wl)
                    if np.isfinite(sigma_normal) and sigma_normal > 0:
                        nq, _ = _shift(n, s * dy, s * dx, 0.0)
                        zq_n, _ = _shift(zero_n, s * dy, s * dx, True)
                        wn = np.maximum(np.sum(n * nq, axis=-1), 0.0) ** float(sigma_normal)
                        w = w * np.where(zero_n | zq_n, 1.0, wn)
                    zq, _ = _shift(z, s * dy, s * dx, -1.0)
                    mq = zq < 0
                    wz = np.where(miss != mq, 0.0, 1.0)
                    if np.isfinite(sigma_depth):
                        both_hit = ~miss & ~mq
                        dz = np.abs(z - zq)
                        with np.errstate(all="ignore"):
                            e = np.where(dz == 0, 1.0, np.exp(-dz / (float(sigma_depth) * s * max(abs(dx), abs(dy)) * z)))
                        wz = np.where(both_hit, e, wz)
                    w = w * wz
                num += w[..., None] * xq
                with np.errstate(invalid="ignore"):
                    vnum += np.where(w > 0, w * w * vq, 0.0)
                den += w
        x = num / den[..., None]
        v = vnum / (den * den)
    if demodulate:
        x = x * a
        v = v * la * la
    out = np.empty((H * W, 4))
    out[:, :3] = x.reshape(-1, 3)
    out[:, 3] = v.reshape(-1)
    return out
