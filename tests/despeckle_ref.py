"""Float64 model of pt_despeckle (include/pt_api.h) on float32-rounded inputs, and the authored frames the host and GPU tests share.

despeckle(rgbv, ...) follows the definition step by step and returns, next to colour, variance and flags, the relative margin of
each decision: |l - T| / max(|l|, |T|) for the limit and |v - g| / max(v, g), g = (min_rel_sigma l)^2, for the gate.  The device
decides in float32, so a pixel whose margin is within rounding may legitimately come out the other way; the tests only compare
flags where the margin is clear.  A 0 / 0 margin (l = T = 0: a black pixel among black ones) counts as clear: every product with an
exact zero is exact in float32 too.  `margin` is the one that matters for the pixel: the limit's where l <= T (the gate is not
asked), else the smaller of the two.

replay(rgbv, flags, ...) runs steps 4-6 for GIVEN flags (the device's), so values can be compared where a decision was within
rounding.  Both return `scale`: per pixel and output column the largest magnitude among the terms of the sum that makes it, fully
written out -- c'(q), and c(p) / n(p) and c'(p) / n(p) for every flagged p of the window (the share is their difference, and a
difference is only as exact as its operands); for the variance v'(q) and (l(c(p)) / n(p))^2.  The device's float32 sum of at most
49 such terms is held to 1e-5 of that scale.
"""
import numpy as np

LUM = tuple(float(np.float32(k)) for k in (0.2126, 0.7152, 0.0722))
DEFAULTS = dict(radius=2, rank=2, threshold=4.0, floor=0.0, min_rel_sigma=0.5, spread=1)
INF = float("inf")


def _lum(c):
    with np.errstate(all="ignore"):
        return LUM[0] * c[..., 0] + LUM[1] * c[..., 1] + LUM[2] * c[..., 2]


def _windows(a, R, fill):
    """(2R+1)^2 shifted copies of the (H, W) array a in raster order (dy outer from -R, dx inner): out[k][y, x] = a[y + dy, x + dx]."""
    H, W = a.shape
    p = np.full((H + 2 * R, W + 2 * R), fill, dtype=a.dtype)
    p[R:R + H, R:R + W] = a
    return np.stack([p[R + dy:R + dy + H, R + dx:R + dx + W] for dy in range(-R, R + 1) for dx in range(-R, R + 1)])


def _rel(a, b):
    """|a - b| / max(|a|, |b|); inf where both are 0 or either is not finite."""
    with np.errstate(all="ignore"):
        m = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    return np.where(np.isfinite(m), m, INF)


def _limit(rgbv, radius, rank, threshold, floor):
    x = np.asarray(rgbv, dtype=np.float32).astype(np.float64)
    c, v = x[..., :3], x[..., 3]
    l = _lum(c)
    live = np.isfinite(l) & (np.abs(l) <= float(np.finfo(np.float32).max))
    win = _windows(np.where(live, l, np.nan), radius, np.nan)
    centre = win.shape[0] // 2
    nb = np.delete(win, centre, axis=0)
    valid = ~np.isnan(nb)
    K = valid.sum(axis=0)
    desc = -np.sort(-np.where(valid, nb, -INF), axis=0)
    idx = np.clip(np.minimum(rank, K) - 1, 0, None)
    m = np.take_along_axis(desc, idx[None], axis=0)[0]
    with np.errstate(all="ignore"):
        T = float(np.float32(threshold)) * m + float(np.float32(floor))
    T = np.where(K > 0, T, 0.0)
    n = K + 1
    return c, v, l, live, K, n, T


def _finish(c, v, l, live, n, T, flagged, radius, spread):
    """Steps 4-6 for the boolean map `flagged`."""
    H, W = l.shape
    with np.errstate(all="ignore"):
        s = np.where(flagged, T / l, 1.0)
    s3 = s[..., None]
    cp = np.where(flagged[..., None], c * s3, c)
    with np.errstate(all="ignore"):
        vp = np.where(flagged, np.where(np.isinf(v), INF, v * s * s), v)
    out_c, out_v = cp.copy(), vp.copy()
    scale = np.concatenate([np.abs(cp), np.abs(np.where(np.isfinite(vp), vp, 0.0))[..., None]], axis=-1)
    if spread:
        nf = n.astype(np.float64)[..., None]
        with np.errstate(invalid="ignore"):
            share = np.where(flagged[..., None], (c - cp) / nf, 0.0)
        ls = _lum(share)
        big_c = np.where(flagged[..., None], np.maximum(np.abs(c), np.abs(cp)) / nf, 0.0)
        big_v = np.where(flagged, (np.abs(np.where(flagged, l, 0.0)) / nf[..., 0]) ** 2, 0.0)
        acc_c = np.zeros_like(cp)
        for k in range(3):
            acc_c[..., k] = _windows(share[..., k], radius, 0.0).sum(axis=0)
            scale[..., k] = np.maximum(scale[..., k], _windows(big_c[..., k], radius, 0.0).max(axis=0))
        acc_v = _windows(ls * ls, radius, 0.0).sum(axis=0)
        scale[..., 3] = np.maximum(scale[..., 3], _windows(big_v, radius, 0.0).max(axis=0))
        out_c = np.where(live[..., None], cp + acc_c, c)
        out_v = np.where(live, vp + acc_v, v)
    return out_c, out_v, scale


def despeckle(rgbv, radius=2, rank=2, threshold=4.0, floor=0.0, min_rel_sigma=0.5, spread=1, **_):
    """rgbv (H, W, 4) -> dict(c (H, W, 3), v (H, W), flags (H, W) int32, above (l > T: the gate was asked), margin_T, margin_gate, margin, scale (H, W, 4)), float64."""
    c, v, l, live, K, n, T = _limit(rgbv, radius, rank, threshold, floor)
    mrs = float(np.float32(min_rel_sigma))
    above = live & (K > 0) & (l > T)
    g = (mrs * l) * (mrs * l)
    asked = (mrs != 0.0) & ~np.isinf(v)                 # the gate compares v with g only then
    with np.errstate(invalid="ignore"):
        gate = ~asked | (v >= g)
    flagged = above & gate
    margin_T = np.where(live & (K > 0), _rel(l, T), INF)
    margin_gate = np.where(asked, _rel(v, g), INF)
    margin = np.where(above, np.minimum(margin_T, margin_gate), margin_T)
    out_c, out_v, scale = _finish(c, v, l, live, n, T, flagged, radius, spread)
    flags = np.where(live, flagged.astype(np.int32), 2).astype(np.int32)
    return dict(c=out_c, v=out_v, live=live, flags=flags, above=above, margin_T=margin_T, margin_gate=margin_gate, margin=margin, scale=scale)


def replay(rgbv, flags, radius=2, rank=2, threshold=4.0, floor=0.0, min_rel_sigma=0.5, spread=1, **_):
    """Steps 4-6 with the given flags (H, W) instead of the model's own decisions; dict(c, v, scale)."""
    c, v, l, live, K, n, T = _limit(rgbv, radius, rank, threshold, floor)
    out_c, out_v, scale = _finish(c, v, l, live, n, T, np.asarray(flags) == 1, radius, spread)
    return dict(c=out_c, v=out_v, live=live, scale=scale)


def check_values(got_rgbv, want, rtol=1e-5):
    """The device's (H, W, 4) float32 against a model dict: within rtol of `scale`; +inf variances must match exactly, pixels that are
    not live are left to the caller (bit for bit against the input).  Returns the worst error / tolerance ratio (<= 1 passes) and where."""
    got = np.asarray(got_rgbv, dtype=np.float64)
    model = np.concatenate([want["c"], want["v"][..., None]], axis=-1)
    both_inf = np.isinf(got) & np.isinf(model) & (np.sign(got) == np.sign(model))
    with np.errstate(invalid="ignore"):
        err = np.where(both_inf, 0.0, np.abs(got - model))
    tol = rtol * want["scale"]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / tol)
    ratio = np.where(want["live"][..., None], np.where(np.isnan(ratio), INF, ratio), 0.0)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), at


# ------------------------------------------------------------------------------------------------------ authored frames
def _base(h, w, seed):
    """A smooth, strictly positive background (luminance within a factor 1.3 over the frame) with a converged variance."""
    rng = np.random.default_rng(seed)
    f = np.empty((h, w, 4), np.float32)
    f[..., :3] = (0.5 + 0.1 * rng.random((h, w, 1)) + 0.02 * rng.random((h, w, 3))).astype(np.float32)
    l = _lum(f[..., :3].astype(np.float64))
    f[..., 3] = ((0.05 * l) ** 2).astype(np.float32)              # relative sigma 0.05: the gate refuses it at 0.5
    return f


def _firefly(f, y, x, gain=40.0, rel_sigma=1.0):
    f[y, x, :3] = (f[y, x, :3].astype(np.float64) * gain * np.array([1.0, 0.9, 1.1])).astype(np.float32)
    l = float(_lum(f[y, x, :3].astype(np.float64)))
    f[y, x, 3] = np.float32(INF if rel_sigma is None else (rel_sigma * l) ** 2)


def authored():
    """[(name, rgbv (H, W, 4) float32, params)]: the table of test_gpu_despeckle.py; test_despeckle_host.py checks that no decision
    of it has a margin under 1e-3."""
    cases = []

    def add(name, f, **kw):
        cases.append((name, f, dict(DEFAULTS, **kw)))

    add("1x1: K = 0", _base(1, 1, 1) * np.float32(50.0), radius=1, rank=1)
    f = _base(3, 2, 2)
    _firefly(f, 1, 0)
    for spread in (0, 1):
        add("2x3 at radius 3, spread %d" % spread, f.copy(), radius=3, rank=1, spread=spread)
    # one tile exactly: the four corners and every edge
    f = _base(16, 16, 3)
    for y, x in ((0, 0), (0, 15), (15, 0), (15, 15), (0, 7), (15, 8), (6, 0), (9, 15), (8, 8)):
        _firefly(f, y, x)
    for radius in (1, 2, 3):
        for spread in (0, 1):
            add("16x16 corners and edges, radius %d spread %d" % (radius, spread), f.copy(), radius=radius, rank=1, spread=spread)
    # partial tiles in both axes; an outlier on each side of the tile boundaries (columns 15 | 16, rows 15 | 16); shares that overlap
    f = _base(19, 17, 4)
    for y, x in ((3, 15), (7, 16), (15, 5), (16, 9), (18, 16), (12, 12), (12, 14)):
        _firefly(f, y, x)
    for radius in (1, 2, 3):
        add("17x19 tile boundaries, radius %d" % radius, f.copy(), radius=radius, rank=3)
    f = _base(5, 33, 5)
    for y, x in ((0, 0), (4, 32), (2, 15), (2, 16), (0, 31), (4, 17)):
        _firefly(f, y, x, rel_sigma=None)                             # v = +inf passes the gate
    for radius in (1, 2, 3):
        add("33x5 v = +inf, radius %d" % radius, f.copy(), radius=radius, rank=2 if radius == 1 else 3)
    # two and three adjacent outliers under rank 1, 2 and 3: rank 1 misses the pair, rank 2 catches it, rank 3 the triple
    f = _base(20, 24, 6)
    _firefly(f, 4, 4)
    _firefly(f, 4, 5, gain=41.0)
    _firefly(f, 12, 10)
    _firefly(f, 12, 11, gain=43.0)
    _firefly(f, 13, 10, gain=39.0)
    _firefly(f, 17, 20)
    for rank in (1, 2, 3):
        for spread in (0, 1):
            add("24x20 pair and triple, rank %d spread %d" % (rank, spread), f.copy(), radius=2, rank=rank, spread=spread)
    # ties in luminance among the top three neighbours (a flat background with equal bright neighbours)
    f = np.empty((9, 9, 4), np.float32)
    f[..., :3] = np.float32(0.25)
    f[..., 3] = np.float32(1e-6)
    for y, x in ((3, 3), (3, 5), (5, 4)):
        f[y, x, :3] = np.float32(2.0)
        f[y, x, 3] = np.float32(9.0)
    f[4, 4, :3] = np.float32(64.0)
    f[4, 4, 3] = np.float32(4096.0)
    for rank in (1, 2, 3):
        add("9x9 ties, rank %d" % rank, f.copy(), radius=1, rank=rank, threshold=2.0)
    # an all-black neighbourhood with floor 0: s = 0, v finite and +inf
    f = np.zeros((8, 12, 4), np.float32)
    f[2, 3] = (3.0, 2.0, 1.0, 5.0)
    f[5, 9] = (1.0, 2.0, 3.0, INF)
    for spread in (0, 1):
        add("12x8 black, spread %d" % spread, f.copy(), radius=2, rank=1, spread=spread)
    add("12x8 black with a floor", f.copy(), radius=2, rank=2, floor=0.5)
    # the gate: a bright pixel of small variance is kept, the same pixel goes with min_rel_sigma = 0 or v = +inf
    f = _base(10, 10, 7)
    _firefly(f, 4, 4, rel_sigma=0.1)
    _firefly(f, 7, 2, rel_sigma=0.1)
    f[7, 2, 3] = np.float32(INF)
    add("10x10 gate refuses", f.copy(), radius=2, rank=1)
    add("10x10 gate off", f.copy(), radius=2, rank=1, min_rel_sigma=0.0)
    add("10x10 gate at 0.05", f.copy(), radius=2, rank=1, min_rel_sigma=0.05, spread=0)
    # pixels that are not live next to an outlier
    f = _base(12, 14, 8)
    _firefly(f, 5, 5)
    f[5, 6, 0] = np.float32(np.nan)
    f[4, 5, 1] = np.float32(INF)
    f[6, 4] = (np.float32(INF), np.float32(-INF), 1.0, 2.0)      # l = NaN from inf - inf
    _firefly(f, 0, 13)
    f[1, 13, 2] = np.float32(np.nan)
    for radius in (1, 3):
        for spread in (0, 1):
            add("14x12 not live, radius %d spread %d" % (radius, spread), f.copy(), radius=radius, rank=1, spread=spread)
    # several tiles at radius 3
    f = _base(40, 48, 9)
    rng = np.random.default_rng(10)
    for _ in range(40):
        _firefly(f, int(rng.integers(0, 40)), int(rng.integers(0, 48)), gain=float(rng.uniform(30.0, 60.0)),
                 rel_sigma=None if rng.random() < 0.2 else 1.0)
    for y, x in ((15, 15), (16, 16), (15, 31), (16, 32), (31, 16), (32, 15), (39, 47), (0, 47), (39, 0)):
        _firefly(f, y, x)
    for spread in (0, 1):
        add("48x40 at radius 3, spread %d" % spread, f.copy(), radius=3, rank=3, spread=spread)
    add("48x40 at radius 2, rank 2", f.copy(), radius=2, rank=2)
    return cases


LARGEST = "48x40 at radius 3, spread 1"
