"""Authored frames for tests/test_gpu_tonemap.py (k_resolve_reinhard, k_filt_im and the 8-bit writer against the oracle) and the guards
that say the frames hold what they are built for (tests/test_tonemap_host.py asserts them without a device).  Plain numpy, deterministic."""
import numpy as np

import spec_inputs as S

SIZES = ((1, 1), (2, 2), (3, 3), (31, 7), (32, 8), (33, 9), (65, 17))      # no interior; one interior pixel; both sides of the 32 x 8 block edge
KNEE = np.float32(0.00304)
F = np.float32


def f1(b):
    """the float32 with bit pattern b"""
    return S.fl(np.array([b], dtype=np.uint32))[0]


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays whose exact a b + c fits float64 (a 48-bit product and an addend within 2^5 of it): one rounding"""
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def reinhard_scale(c):
    """per channel the value the Reinhard map hands to the sRGB curve, c L2 / L (prog.cl:264-267), in float32 as the kernels compute it"""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        L = fma32(F(0.0722), c[:, 2], fma32(F(0.7152), c[:, 1], F(0.2126) * c[:, 0]))
        L2 = L / (F(1.0) + L)
        return (c * L2[:, None]) / L[:, None], L


def zero_luminance_pixels():
    """non-zero channels whose luminance is exactly +-0: y = 0 and z = -2^k make the fma's product 0.0722f 2^k exact, so L is 0 when
    0.2126f x rounds to exactly that; found by searching the floats next to the quotient"""
    found = []
    for k in (0, 3, -5):
        target = F(0.0722) * F(2.0 ** k)
        x0 = int(S.bits(F(target / F(0.2126)))[0])
        for d in range(-4, 5):
            x = f1(x0 + d)
            if F(0.2126) * x == target:
                found += [(float(x), 0.0, -(2.0 ** k)), (-float(x), 0.0, 2.0 ** k)]
                break
    return np.array(found, dtype=F)


def reinhard_pool():
    """(pixels (n, 3), category of each): every value class the map has to get right"""
    nz = f1(0x80000000)
    rows, cat = [], []

    def add(name, px):
        px = np.asarray(px, dtype=F).reshape(-1, 3)
        rows.append(px)
        cat.extend([name] * px.shape[0])

    add("zero", [(0, 0, 0), (nz, nz, nz), (0, nz, 0)])
    add("denormal", [(1e-40, 2e-41, 1e-45), (1e-39, 0, 0), (f1(0x007fffff),) * 3])
    add("negative", [(-0.5, -0.2, -1.0), (-0.5, 0.3, 0.1), (0.5, -0.01, 0.2)])
    g0 = int(S.bits(F(0.00304 / (1 - 0.00304)))[0])                                  # a grey g maps to about g / (1 + g)
    add("knee", [(f1(g0 + d),) * 3 for d in range(-24, 25)])
    add("knee", [(f1(g0 + d), 0.004, 0.002) for d in range(-8, 9)])
    add("huge", [(1e30, 1e30, 1e30), (1e30, 1.0, 0.0), (np.inf, 1.0, 1.0), (np.inf, np.inf, np.inf), (1.0, np.inf, 0.5)])
    add("nan", [(np.nan, 1.0, 1.0), (0.5, np.nan, 0.25), (np.nan, np.nan, np.nan)])
    add("zero_luminance", zero_luminance_pixels())
    add("ordinary", S.unit24(S.hashed(96, 0x70e)).reshape(-1, 3) * F(4.0))
    return np.concatenate(rows), np.array(cat)


def reinhard_frame(w, h):
    """(w h, 4) colours: the pool's pixels in turn, starting where the size says, .w hashed (the maps do not read it)"""
    pool, _ = reinhard_pool()
    idx = (np.arange(w * h) + 7 * w + h) % pool.shape[0]
    return np.concatenate([pool[idx], S.unit24(S.hashed(w * h, 0xa1fa))[:, None]], axis=1).astype(F)


# ---- the median: colours of equal mean grey, so that which one the selection leaves in the middle shows
SAME_GREY = np.array([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.25, 0.25), (0.25, 0.5, 0.25), (0.25, 0.25, 0.5), (0.125, 0.375, 0.5),
                      (0.75, 0.125, 0.125), (0.375, 0.375, 0.25)], dtype=F)          # every sum is exactly 1
E004 = int(S.bits(F(0.004))[0])
AROUND_004 = np.array([(f1(E004 + d), f1(E004 - d), 0.004) for d in range(-3, 4)], dtype=F)
OTHERS = np.array([(0.1, 0.1, 0.1), (2.0, 1.0, 0.5), (0.0, 0.0, 0.0), (0.6, 0.9, 0.3), (np.nan, 0.5, 0.5), (0.2, np.nan, 0.1), (np.inf, 0.0, 0.0),
                   (-1.0, 0.5, 0.25), (0.004, 0.004, 0.004)], dtype=F)


def median_frame(w, h):
    """(w h, 4) colours: hashed picks from a palette in which nine colours share one grey and seven sit around the filmic threshold
    0.004 (these seven share a grey too, up to rounding), with NaN greys among the rest; rows 0..2 x columns 0..2 hold the nine
    equal-grey colours (all nine tie) wherever the frame has them"""
    pal = np.concatenate([SAME_GREY, SAME_GREY[:4], AROUND_004, OTHERS])
    pick = (S.hashed(w * h, 0x3ed1 + 131 * w + h) % np.uint64(pal.shape[0])).astype(np.int64)
    c = pal[pick].reshape(h, w, 3)
    for y in range(min(h, 3)):
        for x in range(min(w, 3)):
            c[y, x] = SAME_GREY[3 * y + x]
    return np.concatenate([c.reshape(-1, 3), np.ones((w * h, 1), dtype=F)], axis=1).astype(F)


def grey(c):
    with np.errstate(invalid="ignore"):
        return ((c[..., 0] + c[..., 1]) + c[..., 2]) / F(3.0)


def neighbourhoods(frame, w, h):
    """(interior pixels, 9, 3): each interior pixel's 3 x 3 neighbourhood in the kernels' order"""
    c = frame[:, :3].reshape(h, w, 3)
    return np.stack([c[y - 1 + i, x - 1 + j] for y in range(1, h - 1) for x in range(1, w - 1) for i in range(3) for j in range(3)]).reshape(-1, 9, 3)


def median_by_selection(nb):
    """prog.cl:405-420 restated: eight rounds of moving the first maximum of the unsorted part to its end; the middle is what is left at 4"""
    nb = nb.copy()
    g = grey(nb)
    for n in range(nb.shape[0]):
        for jn in range(9, 1, -1):
            maxi = 0
            for i in range(1, jn):
                if g[n, i] > g[n, maxi]:
                    maxi = i
            g[n, [jn - 1, maxi]] = g[n, [maxi, jn - 1]]
            nb[n, [jn - 1, maxi]] = nb[n, [maxi, jn - 1]]
    return nb[:, 4]


def median_by_stable_sort(nb):
    """another selection order with the same greys: a stable ascending sort (NaN greys last), element 4"""
    order = np.argsort(grey(nb), axis=1, kind="stable")
    return nb[np.arange(nb.shape[0]), order[:, 4]]


def quantise(rgba, w, h):
    """pt_image_write_ppm's bytes: rows top to bottom (buffer row 0 is the bottom), per channel NaN and negatives to 0, above 1 to 1,
    then lrintf(v * 255.0f): a float32 product rounded to the nearest integer, ties to even"""
    v = np.asarray(rgba, F).reshape(h, w, 4)[::-1, :, :3]
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, F(0.0))
        v = np.where(v > 1, F(1.0), v)
    return np.rint(v.astype(F) * F(255.0)).astype(np.uint8).tobytes()
