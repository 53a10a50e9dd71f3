"""float64 model of pt_temporal_accumulate (include/pt_api.h pins it): the reprojection, the bilinear footprint with its validity tests
and the blend.  Next to the result it reports every pixel's margin to each decision the float32 device makes (the snap of a bilinear
weight, which also covers the floor -- its boundary lies inside the snap band --, the sign of a, the normal and depth tests of every tap
that is read, the W threshold), so that a test can leave out the pixels where float32 rounding may decide differently."""
import numpy as np

SNAP = 2.0 ** -10
MIN_WEIGHT = 0.01
# a pixel is left out when a decision is this close to going the other way: 1e-4 in the decision's own unit (pixels for the snap, the
# value of a, of the cosine, of W), 1e-5 of depth_q for the depth test (|dist - depth_q| is a difference of ~1,000-unit floats whose
# float32 error is ~1e-7 of them; at 1e-4, grazing walls alone leave out ~1.5 % of a 96x64 Cornell frame)
EPS, EPS_DEPTH = 1e-4, 1e-5


def _cam(c):
    c = np.asarray(c).reshape(-1)[0]
    f = lambda k: np.asarray(c[k][:3], np.float64)      # noqa: E731
    return f("eye"), f("lookat"), f("up"), f("right"), float(c["XM"]), float(c["YM"])


def _lum64(x):
    return 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]


def ray_dir(cam, px, py):
    """The direction camera_get_ray(gid, cam, 0.5f, 0.5f) gives, as the device rounds it (float32; dot3's fmaf through libm): the
    reprojection pins D to it, and its float32 rounding moves a point by ~1e-4 px at 128 px, as much as the whole budget."""
    from variance_ref import fmaf
    c = np.asarray(cam).reshape(-1)[0]
    f = lambda k: np.asarray(c[k][:3], np.float32)      # noqa: E731
    X, Y = np.float32(int(c["XM"])), np.float32(int(c["YM"]))
    sx = (np.float32(2.0) * (np.asarray(px).astype(np.float32) + np.float32(0.5))) / X - np.float32(1.0)
    sy = (np.float32(2.0) * (np.asarray(py).astype(np.float32) + np.float32(0.5))) / Y - np.float32(1.0)
    d = ((f("lookat") + f("right") * sx[:, None]) + f("up") * sy[:, None]) - f("eye")
    dd = fmaf(d[:, 2], d[:, 2], fmaf(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
    return d * (np.float32(1.0) / np.sqrt(dd))[:, None]


def reproject(cur, prev, px, py, depth):
    """Pixel centres (px, py) of cur (arrays) followed to depth, in prev's view: (x', y', |X - eye_prev|, a); float64 after ray_dir."""
    eye, lookat, up, right, XM, YM = _cam(cur)
    peye, plookat, pup, pright, pXM, pYM = _cam(prev)
    depth = np.asarray(depth, np.float64)
    D = ray_dir(cur, np.atleast_1d(px), np.atleast_1d(py)).astype(np.float64)
    v = eye + depth[..., None] * D - peye
    ahead = plookat - peye
    ru = np.cross(pright, pup)
    det = np.dot(ahead, ru)
    a = (v @ ru) / det
    b = np.einsum("j,...j->...", ahead, np.cross(v, pup)) / det
    c = np.einsum("j,...j->...", ahead, np.cross(pright, v)) / det
    with np.errstate(divide="ignore", invalid="ignore"):
        xp = (b / a + 1.0) * pXM / 2.0 - 0.5
        yp = (c / a + 1.0) * pYM / 2.0 - 0.5
    return xp, yp, np.linalg.norm(v, axis=-1), a


class History:
    """The model's history set: colour (npix, 3), m2, n, and the guides it was made with (normal_depth (npix, 4), material)."""

    def __init__(self, c, m2, n, nd, mat, cam, bad, tol_c, tol_m2):
        self.c, self.m2, self.n, self.nd, self.mat, self.cam, self.bad = c, m2, n, nd, mat, cam, bad
        self.tol_c, self.tol_m2 = tol_c, tol_m2     # how far the device's colour (any channel) and m2 may be from c and m2


def accumulate(prev, cam, colors, k, albedo_rgbm, normal_depth, W, H, max_history=64, normal_cos=0.9, depth_tolerance=0.02):
    """One pt_temporal_accumulate.  prev: a History or None (no history).  Returns (History of the result, dict with "v" the variance
    of the mean, "margin" the smallest margin to a decision per pixel (the depth test's scaled so that EPS stands for EPS_DEPTH of
    depth_q), "no_tap" the pixels that found no history although their primary ray hit, "tainted" the pixels whose footprint read a
    pixel of prev that was itself left out, "tol_v" how far the device's variance may be from "v").  The result's `bad` = margin < EPS or tainted: where the device may differ, and what the next frame's
    footprint must not read."""
    colors = np.asarray(colors, np.float32)
    npix = W * H
    k = np.broadcast_to(np.asarray(k, np.float64).reshape(-1), (npix,))
    nd = np.asarray(normal_depth, np.float32)
    mat = np.asarray(albedo_rgbm, np.float32)[:, 3]
    fc = colors[:, :3].astype(np.float64)
    fm2 = colors[:, 3].astype(np.float64)
    hc = np.zeros((npix, 3))
    hm2 = np.zeros(npix)
    hn = np.zeros(npix)
    margin = np.full(npix, np.inf)
    scale = np.abs(fc).max(axis=1)
    scale_m2 = np.abs(fm2)
    inh_c = np.zeros(npix)          # the largest tolerance among the history pixels read
    inh_m2 = np.zeros(npix)
    tainted = np.zeros(npix, bool)
    found = np.zeros(npix, bool)
    hit = nd[:, 3] >= 0
    if prev is not None and max_history > 0:
        idx = np.nonzero(hit)[0]
        py, px = np.divmod(idx, W)
        xp, yp, dist, a = reproject(cam, prev.cam, px, py, nd[idx, 3])
        margin[idx] = np.minimum(margin[idx], np.abs(a))
        front = (a > 0) & np.isfinite(xp) & np.isfinite(yp) & (xp > -2) & (xp < W + 1) & (yp > -2) & (yp < H + 1)
        np_ = nd[idx, :3].astype(np.float64)
        zero_np = np.all(nd[idx, :3] == 0, axis=1)
        for t, p in enumerate(idx):
            if not front[t]:
                continue
            ws = []
            for f in (xp[t], yp[t]):
                f0 = np.floor(f)
                fr = f - f0
                margin[p] = min(margin[p], abs(fr - SNAP), abs(fr - (1.0 - SNAP)))
                if fr < SNAP:
                    fr = 0.0
                elif fr > 1.0 - SNAP:
                    fr, f0 = 0.0, f0 + 1.0
                ws.append((int(f0), fr))
            (x0, fx), (y0, fy) = ws
            sw, sc, sm2, sn = 0.0, np.zeros(3), 0.0, 0.0
            for j in (0, 1):
                for i in (0, 1):
                    w = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
                    if w == 0.0:
                        continue
                    qx, qy = x0 + i, y0 + j
                    if not (0 <= qx < W and 0 <= qy < H):
                        continue
                    q = qy * W + qx
                    gq = prev.nd[q]
                    if not (gq[3] > 0) or prev.mat[q] != mat[p]:
                        continue
                    zero_nq = bool(np.all(gq[:3] == 0))
                    if zero_np[t] != zero_nq:
                        continue
                    if not zero_np[t]:
                        dn = float(np.dot(np_[t], gq[:3].astype(np.float64)))
                        margin[p] = min(margin[p], abs(dn - normal_cos))
                        if not dn >= normal_cos:
                            continue
                    dq = float(gq[3])
                    dd = abs(dist[t] - dq) - depth_tolerance * dq
                    margin[p] = min(margin[p], abs(dd) / dq * (EPS / EPS_DEPTH))
                    if not dd <= 0:
                        continue
                    tainted[p] |= prev.bad[q]
                    scale[p] = max(scale[p], float(np.abs(prev.c[q]).max()))
                    scale_m2[p] = max(scale_m2[p], abs(float(prev.m2[q])))
                    inh_c[p] = max(inh_c[p], float(prev.tol_c[q]))
                    inh_m2[p] = max(inh_m2[p], float(prev.tol_m2[q]))
                    sw += w
                    sc += w * prev.c[q]
                    sm2 += w * prev.m2[q]
                    sn += w * prev.n[q]
            margin[p] = min(margin[p], abs(sw - MIN_WEIGHT))
            if sw >= MIN_WEIGHT:
                found[p] = True
                hc[p], hm2[p], hn[p] = sc / sw, sm2 / sw, sn / sw
    nh = np.minimum(hn, float(max_history))
    n = nh + k
    use = nh > 0
    c = np.where(use[:, None], (nh[:, None] * hc + k[:, None] * fc) / n[:, None], fc)
    m2 = np.where(use, (nh * hm2 + k * fm2) / n, fm2)
    n = np.where(use, n, k)
    mu = _lum64(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(n < 2, np.inf, np.maximum(m2 - mu * mu, 0.0) / (n - 1.0))
    bad = (margin < EPS) | tainted
    # tolerances: float32 rounding relative to the result and to the largest input (the bilinear weights come from an x' that is
    # ~1e-5 px off the float64 one: the result moves by that times the spread of the taps), plus the history's own share of what
    # its pixels were allowed
    share = np.where(use, nh / n, 0.0)
    tol_c = 1e-6 + 1e-4 * np.abs(c).max(axis=1) + 1e-4 * scale + share * inh_c
    tol_m2 = 1e-12 + 1e-4 * np.abs(m2) + 2e-4 * scale_m2 + share * inh_m2
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_v = 1e-4 * np.abs(v) + (tol_m2 + 2.0 * np.abs(mu) * tol_c) / np.maximum(n - 1.0, 1.0) + 1e-12
    res = History(c, m2, n, nd.copy(), mat.copy(), np.array(cam, copy=True), bad, tol_c, tol_m2)
    return res, {"v": v, "tol_v": tol_v, "margin": margin, "no_tap": hit & ~found, "tainted": tainted}
