"""Float64 model of pt_display (include/pt_api.h) on float32 inputs, its error bound, and the authored frames the host and GPU tests share.

The histogram is exact: the luminance is the device's float32 fmaf chain bit for bit (fma32 below), the bin comes from its bits.
Everything after the histogram is float64; `tol` bounds what the float32 device may differ by.  The bound counts roundings (u = 2^-24
of the magnitude of the terms, carried through the pyramid next to the values) on the longest dependency chain:

    h = E c                                  1, plus the relative error of E
    bright pass  (h (lh - t)) / lh           lh 3, the subtraction 1, product and quotient 2; the cancellation in lh - t is carried as
                                             an absolute error of lh, times |h| t / lh^2
    one level down                           8: per axis one product and three additions
    one level up, U_k = D_k + up(U_(k+1))    5: per axis one product and one addition, and the addition of D_k
    final  h + (intensity / levels) up(U_1)  7: the upsample 4, the gain's quotient 1, its product 1, the sum 1
    curve                                    Reinhard 9, ACES 8, relative (every term is >= 0)
    encoding                                 sRGB: powf (measured), the rounded exponent 1 / 2.4f (|ln v| u), one product, one difference

so 2 + 6 + 8 levels + 5 (levels - 1) + 7 roundings reach `out`: 88 at six levels.  The error of `out` goes through curve and encoding by
differences of the float64 model itself (each channel moved by its bound in both directions), so the bound follows the slope of the
curve where the pixel sits.  E's error: the fmaf chain of S (u |S_b| at every bin with k_b > 0), the quotient, the difference ev - M,
exp2f and log2f (EPS: relative error of exp2f and of powf on [0.0031308, 1]^(1 / 2.4), error of log2f over max(|log2 x|, 1); the
defaults are twice the 1 ulp the HIP math documentation states, the GPU test measures them and passes twice the measured values)."""
import numpy as np

U = 2.0 ** -24
EPS_DOC = {"exp2": 2.0 * 2.0 ** -23, "log2": 2.0 * 2.0 ** -23, "pow": 2.0 * 2.0 ** -23}
LUM = tuple(np.float32(k) for k in (0.2126, 0.7152, 0.0722))
T = np.float32(np.log2(1.0 + (np.arange(8) + 0.5) / 8.0))
FRAME, DENOISED, TEMPORAL, DESPECKLED = range(4)
MANUAL, AUTO = 0, 1
LINEAR, REINHARD, ACES = range(3)
SRGB, ENC_LINEAR = 0, 1
DEFAULTS = dict(source=FRAME, metering=AUTO, ev=0.0, key=float(np.float32(0.18)), low_permille=100, high_permille=950, min_ev=-16.0, max_ev=16.0, adapt=1.0,
                bloom_levels=4, bloom_threshold=1.0, bloom_intensity=0.0, curve=ACES, white=float("inf"), encoding=SRGB)
KNEE = float(np.float32(0.0031308))


def fma32(a, b, c):
    """float32 fmaf(a, b, c), correctly rounded: the float64 sum is rounded to odd before the cast (53 >= 2 * 24 + 2)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                            # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                      # TwoSum
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def lum32(rgb):
    """The pinned luminance of float32 rgb (..., 3), bit for bit."""
    rgb = np.asarray(rgb, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return fma32(LUM[2], rgb[..., 2], fma32(LUM[1], rgb[..., 1], LUM[0] * rgb[..., 0]))


def lum64(rgb):
    return float(LUM[0]) * rgb[..., 0] + float(LUM[1]) * rgb[..., 1] + float(LUM[2]) * rgb[..., 2]


def live_of(frame):
    f = np.asarray(frame, dtype=np.float32)
    l = lum32(f[..., :3])
    return np.isfinite(f[..., :3]).all(axis=-1) & np.isfinite(l), l


def bins_of(l):
    """bin of float32 luminances >= 2^-16 from their bits"""
    return np.minimum((np.asarray(l, dtype=np.float32).view(np.uint32) >> 20).astype(np.int64) - 888, 255)


def meter(frame, p, prev_exposure=None, eps=EPS_DOC):
    """dict(hist, n_dark, n_nonfinite, K, M, E, E_rtol, M_atol) of step 1."""
    live, l = live_of(frame)
    dark = live & ~(l >= np.float32(2.0 ** -16))
    lit = live & ~dark
    hist = np.bincount(bins_of(l[lit]).ravel(), minlength=256).astype(np.uint32)
    N = int(hist.sum())
    lo, hi = N * int(p["low_permille"]) // 1000, N * int(p["high_permille"]) // 1000
    cum = np.concatenate([[0], np.cumsum(hist.astype(np.int64))])
    k = np.maximum(np.minimum(cum[1:], hi) - np.maximum(cum[:-1], lo), 0)
    K = int(k.sum())
    lam = (((np.arange(256) >> 3) - 16).astype(np.float32) + T[np.arange(256) & 7]).astype(np.float64)
    partial = np.cumsum(k * lam)
    M = float(partial[-1] / K) if K else 0.0
    M_atol = (float(np.abs(partial[k > 0]).sum()) * U / K + U * abs(M)) if K else 0.0
    ev, key = float(np.float32(p["ev"])), float(np.float32(p["key"]))
    E, rtol = 2.0 ** ev, eps["exp2"]
    if p["metering"] == AUTO:
        if K:
            E = key * 2.0 ** (ev - M)
            rtol = np.log(2.0) * (M_atol + U * abs(ev - M)) + eps["exp2"] + U
            e_lo, e_hi = 2.0 ** float(np.float32(p["min_ev"])), 2.0 ** float(np.float32(p["max_ev"]))
            if E < e_lo * (1 + rtol) or E > e_hi * (1 - rtol):             # (at the clamp either side may win: both errors)
                rtol += eps["exp2"]
            E = min(max(E, e_lo), e_hi)
        a = float(np.float32(p["adapt"]))
        if prev_exposure is not None and a < 1.0:
            pe = float(np.float32(prev_exposure))
            x0, x1 = np.log2(pe), np.log2(E)
            d = (1 - a) * eps["log2"] * max(abs(x0), 1.0) + a * (eps["log2"] * max(abs(x1), 1.0) + rtol / np.log(2.0)) + 4 * U * (abs(x0) + abs(x1))
            E = 2.0 ** ((1 - a) * x0 + a * x1)
            rtol = np.log(2.0) * d + eps["exp2"]
    return dict(hist=hist, n_dark=int(dark.sum()), n_nonfinite=int((~live).sum()), K=K, M=M, M_atol=M_atol, E=float(E), E_rtol=float(rtol), live=live)


def level_sizes(W, H, levels):
    out = [(W, H)]
    for _ in range(levels):
        W, H = (W + 1) // 2, (H + 1) // 2
        out.append((W, H))
    return out


def down(D):
    """one level down of (H, W, 3): 4 x 4 taps {1, 3, 3, 1} / 8 per axis at 2x - 1 + i, clamped"""
    a = np.array([1.0, 3.0, 3.0, 1.0]) / 8.0
    H, W = D.shape[:2]
    xs, ys = np.arange((W + 1) // 2), np.arange((H + 1) // 2)
    r = sum(a[i] * D[:, np.clip(2 * xs - 1 + i, 0, W - 1)] for i in range(4))
    return sum(a[j] * r[np.clip(2 * ys - 1 + j, 0, H - 1)] for j in range(4))


def up(S, W, H):
    """the separable upsample of (sh, sw, 3) to (H, W, 3): 3/4 of x >> 1, 1/4 of its neighbour on x's side, clamped"""
    sh, sw = S.shape[:2]
    xs, ys = np.arange(W), np.arange(H)
    qx = np.clip((xs >> 1) + np.where(xs & 1, 1, -1), 0, sw - 1)
    qy = np.clip((ys >> 1) + np.where(ys & 1, 1, -1), 0, sh - 1)
    t = 0.75 * S[:, xs >> 1] + 0.25 * S[:, qx]
    return 0.75 * t[ys >> 1] + 0.25 * t[qy]


def _border(a):
    return bool(np.any(a[0] != 0) or np.any(a[-1] != 0) or np.any(a[:, 0] != 0) or np.any(a[:, -1] != 0))


def bloom(h, habs_err, p, levels):
    """step 2 on h (H, W, 3) with the absolute error bound habs_err of h: dict(B, up (= up(U_1)), up_err, touches_border)."""
    H, W = h.shape[:2]
    thr = float(np.float32(p["bloom_threshold"]))
    lh, lhabs = lum64(h), lum64(np.abs(h))
    with np.errstate(divide="ignore", invalid="ignore"):
        on = lh > thr
        B = np.where(on[..., None], h * ((lh - thr) / lh)[..., None], 0.0)
        dlh = 3 * U * lhabs + lum64(habs_err)
        near = lh + dlh > thr
        Berr = np.abs(B) * (habs_err / np.maximum(np.abs(h), 1e-300) + 3 * U) + np.where(near[..., None], np.abs(h) * (thr * dlh / np.maximum(lh, 1e-300) ** 2)[..., None], 0.0)
    D, Dm, De = [B], [np.abs(B)], [Berr]
    touches = False
    for _ in range(levels):
        touches = touches or _border(Dm[-1])
        De.append(down(De[-1]) + 8 * U * down(Dm[-1]))
        D.append(down(D[-1]))
        Dm.append(down(Dm[-1]))
    Uv, Um, Ue = D[levels], Dm[levels], De[levels]
    for k in range(levels - 1, 0, -1):
        touches = touches or _border(Um)
        hk, wk = D[k].shape[:2]
        um = Dm[k] + up(Um, wk, hk)
        Ue = De[k] + up(Ue, wk, hk) + 5 * U * um
        Uv, Um = D[k] + up(Uv, wk, hk), um
    touches = touches or _border(Um)
    return dict(B=B, up=up(Uv, W, H), up_mag=up(Um, W, H), up_err=up(Ue, W, H), touches_border=touches)


def curve(x, p):
    c = p["curve"]
    if c == LINEAR:
        return x
    if c == REINHARD:
        w = float(np.float32(p["white"]))
        L = lum64(x)[..., None]
        with np.errstate(over="ignore"):
            return x * ((1.0 + L / (w * w)) / (1.0 + L))
    return (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)


def encode(t, p):
    v = np.clip(t, 0.0, 1.0)
    if p["encoding"] == SRGB:
        v = np.where(v < KNEE, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
    return v


def tone(out, p):
    """step 3 of out (..., 3)"""
    return encode(curve(np.where(out > 0, out, 0.0), p), p)


CURVE_ROUNDINGS = {LINEAR: 0, REINHARD: 9, ACES: 8}


def display(frame, prev_exposure=None, eps=EPS_DOC, **params):
    """The whole stage on frame (H, W, >= 3) float32.  dict(hist, n_dark, n_nonfinite, K, M, E, E_rtol, live, h, out (before the curve), v
    (H, W, 3), tol (H, W, 3), rgba (H, W, 4), rgb8 (H, W, 3) top row first, decidable (H, W, 3) in rgb8's order, levels, B, bloom,
    touches_border)."""
    p = dict(DEFAULTS)
    p.update(params)
    f = np.asarray(frame, dtype=np.float32)
    r = meter(f, p, prev_exposure, eps)
    live, E = r["live"], r["E"]
    c = np.where(live[..., None], f[..., :3].astype(np.float64), 0.0)
    h = E * c
    herr = np.abs(h) * (r["E_rtol"] + U)
    inten = float(np.float32(p["bloom_intensity"]))
    levels = int(p["bloom_levels"]) if inten > 0 else 0
    out, oerr = h, herr
    if levels:
        b = bloom(h, herr, p, levels)
        g = inten / levels
        out = h + g * b["up"]
        oerr = herr + g * (b["up_err"] + 6 * U * b["up_mag"]) + U * (np.abs(h) + g * b["up_mag"])
        r.update(B=b["B"], bloom=b["up"], touches_border=b["touches_border"])
    v = tone(out, p)
    # the error of out through curve and encoding: each channel moved by its bound, both ways
    tol = np.zeros_like(v)
    for ch in range(3):
        d = np.zeros_like(out)
        d[..., ch] = oerr[..., ch]
        tol += np.maximum(np.abs(tone(out + d, p) - v), np.abs(tone(out - d, p) - v))
    t = curve(np.where(out > 0, out, 0.0), p)
    dt = (CURVE_ROUNDINGS[p["curve"]] + 1) * U * np.abs(t)
    tol += np.maximum(np.abs(encode(t + dt, p) - v), np.abs(encode(t - dt, p) - v))
    if p["encoding"] == SRGB:
        tc = np.clip(t, 0.0, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            tol += np.where(tc >= KNEE, (eps["pow"] + U * np.abs(np.log(np.maximum(tc, 1e-300))) + 3 * U) * (v + 0.055), 2 * U * v)
            # within reach of the knee either branch may be taken
            reach = np.abs(tc - KNEE) <= dt + 2 * U * KNEE + tol / 12.92
            tol += np.where(reach, np.abs(12.92 * tc - (1.055 * np.power(tc, 1.0 / 2.4) - 0.055)), 0.0)
    v = np.where(live[..., None], v, 0.0)
    tol = np.where(live[..., None], tol, 0.0)
    y = 255.0 * v
    rgb8 = np.floor(y + 0.5).astype(np.uint8)
    edge = np.abs(y - (np.floor(y) + 0.5))
    decidable = edge > 255.0 * tol + 512.0 * U
    r.update(h=h, out=out, v=v, tol=tol, rgba=np.concatenate([v, np.ones(v.shape[:2] + (1,))], axis=-1), rgb8=rgb8[::-1], decidable=decidable[::-1],
             levels=levels)
    return r


# ------------------------------------------------------------------------------------------------------------- authored frames
def _rgba(rgb):
    rgb = np.asarray(rgb, dtype=np.float32)
    return np.concatenate([rgb, np.zeros(rgb.shape[:2] + (1,), dtype=np.float32)], axis=-1)


def ramp(w, h, lo=-20.0, hi=20.0):
    """log-uniform over 2^lo .. 2^hi in raster order, a slight tint per channel"""
    e = lo + (hi - lo) * np.arange(w * h, dtype=np.float64) / max(w * h - 1, 1)
    g = 2.0 ** e.reshape(h, w)
    return _rgba(np.stack([g, 0.9 * g, 1.1 * g], axis=-1))


def edges(w=17, h=9):
    """greys around bin edges 2^e (1 + j / 8): the edge itself and two ulps on either side, from dark over every range to bin 255"""
    vals = []
    for e in (-17, -16, -15, -1, 0, 1, 15, 16, 17):
        for j in (0, 3):
            t = np.float32(2.0 ** e * (1 + j / 8.0))
            x = t
            for _ in range(2):
                x = np.nextafter(x, np.float32(0))
            for _ in range(5):
                vals.append(x)
                x = np.nextafter(x, np.float32(np.inf))
    f = np.zeros((h, w, 3), dtype=np.float32)
    f.reshape(-1, 3)[:len(vals)] = np.asarray(vals, dtype=np.float32)[:, None]
    f.reshape(-1, 3)[len(vals):len(vals) + 4] = [[-1.0, 2.0, 0.5], [0.5, -0.25, 0.0], [-1.0, -1.0, -1.0], [0.0, 1e-6, 0.0]]
    assert len(vals) + 4 <= w * h
    return _rgba(f)


def blobs(w, h, seed=7, peak=24.0):
    """a smooth scene-like frame: mid-grey gradient plus a few bright blobs"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = 0.05 + 0.4 * x / max(w - 1, 1) + 0.2 * y / max(h - 1, 1)
    f = np.stack([g, 0.8 * g, 0.6 * g], axis=-1)
    for _ in range(5):
        cx, cy, s = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h, rng.uniform(0.8, 2.0)
        f += (peak * rng.uniform(0.3, 1.0) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)))[..., None] * rng.uniform(0.5, 1.0, 3)
    return _rgba(f)


def impulse(w, h, x, y, value=100.0):
    f = np.zeros((h, w, 3), dtype=np.float32)
    f[y, x] = (value, 0.5 * value, 0.25 * value)
    return _rgba(f)


def with_nonfinite(frame):
    """NaN, +inf and -inf pixels alone, a channel alone, a block over the corner (32, 8) of the pyramid's tiles and one over the row 16
    of the final kernel's"""
    f = frame.copy()
    h, w = f.shape[:2]
    f[7 % h, 5 % w, :3] = np.nan
    f[3 % h, 40 % w, 1] = np.inf
    f[50 % h, 20 % w, :3] = -np.inf
    f[12 % h, 9 % w, 2] = np.nan
    if w >= 34 and h >= 18:
        f[6:10, 30:34, :3] = np.nan
        f[14:18, w - 2:, 0] = np.inf
    f[h - 1, w - 1, :3] = np.inf
    return f


def authored():
    """[(name, frame (h, w, 4) float32)]"""
    out = [("1x1 grey", _rgba(np.full((1, 1, 3), 0.37, dtype=np.float32))),
           ("1x1 bright", _rgba(np.full((1, 1, 3), 40.0, dtype=np.float32))),
           ("3x2 zero and negative channels", _rgba(np.array([[[0, 0, 0], [-1, 2, 0.5], [0.5, -0.25, 0]], [[-1, -1, -1], [3, 0, 0], [0, 1e-6, 0]]], dtype=np.float32))),
           ("3x2 all non-finite", _rgba(np.array([[[np.nan] * 3, [np.inf, 0, 0], [0, -np.inf, 0]], [[np.nan, 1, 1], [np.inf] * 3, [1, 1, -np.inf]]], dtype=np.float32))),
           ("17x9 all black", np.zeros((9, 17, 4), dtype=np.float32)),
           ("17x9 bin edges", edges()),
           ("17x9 ramp", ramp(17, 9)),
           ("33x31 blobs", blobs(33, 31)),
           ("33x31 impulse in a corner", impulse(33, 31, 0, 0) + impulse(33, 31, 32, 30, 60.0)),
           ("33x31 ramp with non-finite", with_nonfinite(ramp(33, 31))),
           ("64x64 ramp", ramp(64, 64)),
           ("64x64 blobs with non-finite", with_nonfinite(blobs(64, 64, seed=3))),
           ("64x64 interior impulse", impulse(64, 64, 32, 32))]
    return out


IMPULSE = "64x64 interior impulse"
BLOOM = dict(bloom_threshold=1.0, bloom_intensity=0.5)


def configs():
    """[(name, params)]: manual and auto metering x three curves x two encodings x (no bloom, levels 1, 2, 6)"""
    out = []
    for mname, m in (("manual", dict(metering=MANUAL, ev=-1.0)), ("auto", dict(metering=AUTO))):
        for cname, c in (("linear", LINEAR), ("reinhard", REINHARD), ("aces", ACES)):
            for ename, e in (("srgb", SRGB), ("lin", ENC_LINEAR)):
                for levels in (0, 1, 2, 6):
                    p = dict(m, curve=c, encoding=e)
                    if c == REINHARD and e == SRGB:
                        p["white"] = 4.0
                    if levels:
                        p.update(BLOOM, bloom_levels=levels)
                    out.append(("%s %s %s L%d" % (mname, cname, ename, levels), p))
    return out
