"""CPU replay of the guide buffers (pt_render_aovs) and a float64 model of the a-trous filter (pt_denoise), both pinned in
include/pt_api.h.

The AOV replay runs in numpy float32 on the oracle's own camera, closest-hit and specular / refractive ray constructors, so
that the GPU's buffers can be compared bit for bit.  A refraction is forced by handing orc_new_ray_refractive a draw > 1 (the
reflection probability is at most 1): it then refracts exactly when disc > 0, as the AOV pass does."""
import ctypes as C

import numpy as np

F32 = np.float32


def _fma32(a, b, c):
    # the product of two float32 is exact in float64; one rounding of the sum, then to float32 (this double rounding differs from
    # a true fma only when the float64 sum lands exactly halfway between two float32 -- it decides no more than a sign here)
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def dot3(a, b):
    """pt_device.hpp dot3: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return _fma32(a[2], b[2], _fma32(a[1], b[1], F32(F32(a[0]) * F32(b[0]))))


def subpixel_offsets(n):
    """The (rnd1, rnd2) of every sub-pixel in raster order (j outer, i inner), rounded as the device computes them."""
    out = []
    for j in range(n):
        for i in range(n):
            out.append((F32(F32(i) + F32(0.5)) / F32(n), F32(F32(j) + F32(0.5)) / F32(n)))
    return out


def _trace_chain(oracle, osc, ray, specular_depth):
    """One sub-pixel ray: (t of the primary hit or None, albedo (3,) f32, normal (3,) f32, material or -1)."""
    L = oracle.lib()
    zero = np.zeros(3, dtype=F32)
    hit = osc.closest_hit(ray)[0]
    if not hit["t"] > 0:
        return None, zero, zero, -1
    t0 = F32(hit["t"])
    tint = np.ones(3, dtype=F32)
    inside = C.c_int(0)
    d = 0
    while True:
        D = ray["D"][0, :3].astype(F32)
        N = hit["N"][:3].astype(F32).copy()
        if dot3(D, N) > 0:
            N = -N
        mat = hit["mat"]
        mtype = int(mat["type"])
        if mtype in (1, 2) and d < specular_depth:
            P4 = np.zeros(4, dtype=F32)
            P4[:3] = hit["P"][:3]
            N4 = np.zeros(4, dtype=F32)
            N4[:3] = N
            new = np.zeros(1, dtype=oracle.RAY)
            if mtype == 1:
                tint = (tint * mat["F0"][:3].astype(F32)).astype(F32)
                L.orc_new_ray_specular(new.ctypes.data_as(C.c_void_p), P4.ctypes.data_as(C.c_void_p), N4.ctypes.data_as(C.c_void_p),
                                       ray.ctypes.data_as(C.c_void_p))
            else:
                F04 = mat["F0"].astype(F32).copy()
                L.orc_new_ray_refractive(new.ctypes.data_as(C.c_void_p), P4.ctypes.data_as(C.c_void_p), N4.ctypes.data_as(C.c_void_p),
                                         F04.ctypes.data_as(C.c_void_p), float(mat["n"]), ray.ctypes.data_as(C.c_void_p),
                                         C.byref(inside), 2.0)
            ray = new
            d += 1
            hit = osc.closest_hit(ray)[0]
            if not hit["t"] > 0:
                return t0, zero, zero, -1
            continue
        if mtype == 1:
            a = mat["F0"][:3].astype(F32)
        elif mtype == 2:
            a = np.ones(3, dtype=F32)
        else:
            a = (mat["kd"][:3].astype(F32) + mat["emission"][:3].astype(F32)).astype(F32)
        return t0, (tint * a).astype(F32), N, int(hit["mati"])


def aov_replay(oracle, osc, cam, pixel_ids, subpixels, specular_depth):
    """albedo_rgbm, normal_depth ((len(pixel_ids), 4) float32) as pt_render_aovs must leave them for those global pixel ids."""
    L = oracle.lib()
    npix = len(pixel_ids)
    sa = np.zeros((npix, 3), dtype=F32)
    sn = np.zeros((npix, 3), dtype=F32)
    st = np.zeros(npix, dtype=F32)
    hits = np.zeros(npix, dtype=np.int64)
    mat0 = np.full(npix, -1.0, dtype=F32)
    offs = subpixel_offsets(subpixels)
    for k, (r1, r2) in enumerate(offs):
        for p, gid in enumerate(pixel_ids):
            ray = np.zeros(1, dtype=oracle.RAY)
            L.orc_camera_get_ray(ray.ctypes.data_as(C.c_void_p), int(gid), cam.ctypes.data_as(C.c_void_p), float(r1), float(r2))
            t, alb, nrm, mat = _trace_chain(oracle, osc, ray, specular_depth)
            if t is not None:
                st[p] = F32(st[p] + t)
                hits[p] += 1
            if k == 0:
                mat0[p] = F32(mat)
            sa[p] = (sa[p] + alb).astype(F32)
            sn[p] = (sn[p] + nrm).astype(F32)
    albedo = np.empty((npix, 4), dtype=F32)
    albedo[:, :3] = sa / F32(subpixels * subpixels)
    albedo[:, 3] = mat0
    nd = np.zeros((npix, 4), dtype=F32)
    l2 = (sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1]) + sn[:, 2] * sn[:, 2]
    nz = np.any(sn != 0, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F32(1.0) / np.sqrt(l2)
    nd[nz, :3] = sn[nz] * inv[nz, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        nd[:, 3] = np.where(hits > 0, st / hits.astype(F32), F32(-1.0))
    return albedo, nd


# ---------------------------------------------------------------------------------------------------------- the filter
KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float64)


def _shift(a, sy, sx, fill):
    """b[y, x] = a[y + sy, x + sx] where that is inside the frame, else fill; plus the inside mask."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    m = np.zeros((H, W), dtype=bool)
    y0, y1 = max(0, -sy), min(H, H - sy)
    x0, x1 = max(0, -sx), min(W, W - sx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
        m[y0:y1, x0:x1] = True
    return b, m


def atrous_model(colors, albedo_rgbm, normal_depth, W, H, iterations=5, sigma_color=np.inf, sigma_normal=0.0, sigma_depth=np.inf,
                 demodulate=0):
    """The filter of include/pt_api.h in float64; (W*H, 4) float64 with .w = 1 (rows of colors' layout)."""
    c = np.asarray(colors, dtype=np.float64)[:, :3].reshape(H, W, 3)
    a = np.maximum(np.asarray(albedo_rgbm, dtype=np.float64)[:, :3].reshape(H, W, 3), 1e-3)
    nd = np.asarray(normal_depth, dtype=np.float64).reshape(H, W, 4)
    n, z = nd[..., :3], nd[..., 3]
    miss = z < 0
    zero_n = np.all(n == 0, axis=-1)
    x = c / a if demodulate else c.copy()
    for i in range(iterations):
        s = 1 << i
        num = np.zeros_like(x)
        den = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                xq, inside = _shift(x, s * dy, s * dx, 0.0)
                if dx == 0 and dy == 0:
                    w = np.full((H, W), 9.0 / 64.0)
                else:
                    w = np.where(inside, KERNEL[dx + 2] * KERNEL[dy + 2], 0.0)
                    if np.isfinite(sigma_color):
                        d2 = np.sum((x - xq) ** 2, axis=-1)
                        with np.errstate(divide="ignore", invalid="ignore"):
                            wc = np.where(d2 == 0, 1.0, np.exp(-(d2 * 4.0 ** i) / (float(sigma_color) ** 2)))
                        w = w * wc
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
                den += w
        x = num / den[..., None]
    if demodulate:
        x = x * a
    out = np.ones((H * W, 4))
    out[:, :3] = x.reshape(-1, 3)
    return out


def b3_blur(colors, W, H, iterations):
    """Plain B3-spline a-trous (no edge stopping; taps outside the frame skipped and the rest renormalised)."""
    x = np.asarray(colors, dtype=np.float64)[:, :3].reshape(H, W, 3)
    for i in range(iterations):
        s = 1 << i
        num = np.zeros_like(x)
        den = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                xq, inside = _shift(x, s * dy, s * dx, 0.0)
                w = np.where(inside, KERNEL[dx + 2] * KERNEL[dy + 2], 0.0)
                num += w[..., None] * xq
                den += w
        x = num / den[..., None]
    return x.reshape(-1, 3)
