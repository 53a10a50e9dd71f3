"""Input builders of tests/test_gpu_spec_math.py (pt_debug_spec against the oracle's unit-level functions) and the guards that say an
input list reaches the classes it is meant to reach.  Plain numpy and deterministic (a hash of the index, no random state), so the
lists can be built, counted and fed to the oracle without a device (tests/test_spec_host.py).

Floats travel as float32 arrays; `bits` / `fl` move between a float32 array and its uint32 bit patterns."""
import numpy as np

M32 = np.uint64(0xffffffff)
ONE = 0x3f800000              # 1.0f
LCG_M = 2147483647            # the modulus 2^31 - 1 of prog.cl:72-77
LCG_ONE = LCG_M - 1           # the state whose float is (float)(2^31 - 2) / 2^31 = 1.0f


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fl(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def hashed(n, salt):
    """n well-mixed 32-bit values (uint64 array holding them), a different stream per salt"""
    k = np.arange(n, dtype=np.uint64)
    return lowbias32(lowbias32(k ^ np.uint64(salt)) + np.uint64(0x9e3779b9) * (np.uint64(salt & 0xffff) + np.uint64(1)))


def unit24(h, closed=False):
    """hashed 32-bit values -> float32 k / 2^24 (exact): k in [1, 2^24 - 1], so in (0, 1); closed: k in [0, 2^24], so in [0, 1]"""
    top = h >> np.uint64(8)
    k = top % np.uint64((1 << 24) + 1) if closed else top % np.uint64((1 << 24) - 1) + np.uint64(1)
    return (k.astype(np.float64) / float(1 << 24)).astype(np.float32)


def lcg_float(n):
    """the float lcg_rand returns for new state n: (float)n / 2147483648.0f"""
    return np.asarray(n, dtype=np.int64).astype(np.float32) / np.float32(2147483648.0)


def lcg_states(n, salt, below_one=False):
    """n hashed LCG states in [1, 2^31 - 2]; below_one: in [1, 2^31 - 65], the states whose float is < 1.0f (2^31 - 64 and above round
    up to 2^31)"""
    top = LCG_M - 65 if below_one else LCG_M - 1
    return (hashed(n, salt) % np.uint64(top) + np.uint64(1)).astype(np.int64)


def lcg_step(seed):
    """prog.cl:72-77 on int32 seeds (a negative one sign-extends to 64 bits and wraps): the new states, int64 in [0, 2^31 - 2]"""
    w = np.asarray(seed, dtype=np.int32).astype(np.int64).astype(np.uint64)
    return ((w * np.uint64(48271)) % np.uint64(LCG_M)).astype(np.int64)


def theta_of(rnd):
    """the angle lobe_direction forms from rnd2: (float)(6.283185307179586 * (double)rnd)"""
    return (6.283185307179586 * np.asarray(rnd, dtype=np.float32).astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ sine and cosine
def sincos_inputs():
    """float32 angles in the oracle's domain [0, 8]"""
    grid = np.arange(0, 0x41000000 + 1, 256, dtype=np.int64)                         # every 256th float of [0, 8]
    near = []
    for k in range(11):                                                              # +-128 ulp around the float nearest k pi / 4
        c = int(bits(np.float32(k * np.pi / 4))[0])
        near.append(np.arange(max(c - 128, 0), c + 129, dtype=np.int64))
    edge = np.array([0, 1, 0x00800000, 0x41000000], dtype=np.int64)                  # +0, smallest denormal, 2^-126, 8
    n = np.concatenate([np.array([1, 2, 3, LCG_ONE], dtype=np.int64), lcg_states(1 << 20, 0x51c05)])
    th = bits(theta_of(lcg_float(n))).astype(np.int64)
    return fl(np.concatenate([grid] + near + [edge, th]).astype(np.uint32))


def sincos_quadrants(theta):
    """q & 3 of spec_sincos for every angle, the way the routine forms q (without its fma: this is for counting)"""
    q = np.floor(np.asarray(theta, dtype=np.float32).astype(np.float64) * 0.63661977236758138 + 0.5).astype(np.int64)
    return q & 3


# ------------------------------------------------------------------------------------------------ pow
POW_MANTISSAS = [0x000000, 0x000001, 0x000002, 0x0ccccd, 0x100000, 0x200000, 0x2aaaab, 0x3504f3, 0x3504f4, 0x400000, 0x555555, 0x600000,
                 0x6db6db, 0x7f0000, 0x7ffffe, 0x7fffff]
SQRT2_MANTISSA = 0x3504f3        # 0x3fb504f3 is the float just below sqrt 2, 0x3fb504f4 the one just above
POW_Y = fl(np.array([0x00000000, 0x80000000, 0x00000001], dtype=np.uint32)).tolist() + [0.4167, 1.0, 2.0, 5.0, 50.0, 200.0, 1e4, 1e30, -1.0, -50.0,
                                                                                      np.inf, -np.inf, np.nan]


def pow_x_list():
    expo = np.arange(1, 255, dtype=np.int64) << 23                                   # binary exponents -126 .. 127
    parts = [np.array([0x00000000, 0x80000000, 0x00000001, 0x00800000], dtype=np.int64),            # +0, -0, denormal, 2^-126
             (expo[:, None] | np.array(POW_MANTISSAS, dtype=np.int64)[None, :]).reshape(-1),
             (expo[:, None] | (SQRT2_MANTISSA + np.arange(-8, 9, dtype=np.int64))[None, :]).reshape(-1),
             np.array([ONE - 1, ONE, ONE + 1], dtype=np.int64),                      # 1 - 2^-24, 1, 1 + 2^-23
             np.array([0x40000000], dtype=np.int64), bits(np.float32(1e30)).astype(np.int64),       # 2, 1e30
             np.array([0x7f800000, 0x7fc00000, 0xbf800000, 0xff800000], dtype=np.int64)]            # +inf, NaN, -1, -inf
    x = fl(np.concatenate(parts).astype(np.uint32))
    return np.concatenate([x, unit24(hashed(1 << 16, 0x90f1), closed=False), np.array([1.0], dtype=np.float32)])       # hashed floats in (0, 1]


def pow_threshold_pairs():
    """for 4,096 hashed x in (0, 1): y with y log2(x) at -126 and at 128 as nearly as float32 allows, and 1 .. 4 ulps to either side"""
    x = unit24(hashed(4096, 0x7e57), closed=False)
    lg = np.log2(x.astype(np.float64))
    xs, ys = [], []
    for target in (-126.0, 128.0):
        y0 = bits((target / lg).astype(np.float32)).astype(np.int64)
        for d in range(-4, 5):
            xs.append(x)
            ys.append(fl((y0 + d).astype(np.uint32)))
    return np.concatenate(xs), np.concatenate(ys)


def pow_inputs():
    """(x, y) float32 arrays: the cross product of the two lists, then the threshold pairs"""
    xl, yl = pow_x_list(), np.array(POW_Y, dtype=np.float32)
    tx, ty = pow_threshold_pairs()
    return np.concatenate([np.repeat(xl, yl.size), tx]), np.concatenate([np.tile(yl, xl.size), ty])


def pow_guards(x, y, out):
    """how many pairs reach each branch of spec_pow past its special cases, counted from the inputs and the ORACLE's results"""
    x, y, out = (np.asarray(a, dtype=np.float32) for a in (x, y, out))
    with np.errstate(invalid="ignore"):
        general = (x > 0) & np.isfinite(x) & (y != 0) & ~np.isnan(y)                  # neither returned early
        m = 2.0 * np.frexp(x.astype(np.float64))[0]                                   # the mantissa in [1, 2)
        tiny = general & (out > 0) & (out < np.float32(2.0 ** -120))
    ob = bits(out)
    return {"underflow_zero": int((general & (ob == 0)).sum()), "overflow_inf": int((general & (ob == 0x7f800000)).sum()),
            "finite_below_2^-120": int(tiny.sum()), "above_sqrt2": int((general & (m > 1.4142135623730951)).sum()),
            "below_sqrt2": int((general & ~(m > 1.4142135623730951)).sum())}


POW_GUARD_MIN = {"underflow_zero": 1000, "overflow_inf": 1000, "finite_below_2^-120": 1000, "above_sqrt2": 100, "below_sqrt2": 100}


# ------------------------------------------------------------------------------------------------ pow5 and fresnel
def pow5_inputs():
    special = fl(np.array([0x00000000, ONE, 0x00000001, 0x007fffff, 0x7fc00000, 0x7f800000, 0x80000000, 0xff800000], dtype=np.uint32))
    return np.concatenate([unit24(hashed(1 << 20, 0x9055), closed=True), special])


def unit_vectors(n, salt):
    """n hashed unit vectors: normalised in float64, rounded to float32"""
    v = np.stack([hashed(n, salt + k).astype(np.float64) / 2147483648.0 - 1.0 for k in range(3)], axis=1)
    v[(v * v).sum(axis=1) < 1e-3] = (0.6, 0.0, 0.8)
    return (v / np.sqrt((v * v).sum(axis=1))[:, None]).astype(np.float32)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)


def fresnel_inputs():
    """65,536 items (n, 9) {F0, N, D} and masks of the rows built for a class:
    'perp': N . D = 0 exactly (every product is an exact zero); 'par': D = +-N, so |N . D| is 1 up to rounding -- exactly 1 on the axes,
    a last bit below or above it elsewhere.  Rows of both classes have F0.x = 0, so that the result's x is (1 - |N . D|)^5 itself."""
    n = 65536
    F0 = np.stack([unit24(hashed(n, 0xf0 + k), closed=True) for k in range(3)], axis=1)
    F0[::8] = 1.0                                                                     # what N = K = 0 materials get
    N, D = unit_vectors(n, 0x4e00), unit_vectors(n, 0xd100)
    perp, par = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    # axis pairs: 36 combinations, perpendicular or (anti)parallel
    a, b = np.repeat(np.arange(6), 6), np.tile(np.arange(6), 6)
    r = np.arange(1024, 1024 + 36 * 8)
    N[r], D[r] = AXES[np.tile(a, 8)], AXES[np.tile(b, 8)]
    same_axis = np.tile(a // 2 == b // 2, 8)
    perp[r], par[r] = ~same_axis, same_axis
    # N in a coordinate plane, D along the third axis
    r = np.arange(2048, 2048 + 1536)
    third = (np.arange(r.size) % 3)
    sign = np.where(np.arange(r.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    Nn = N[r].astype(np.float64)
    Nn[np.arange(r.size), third] = 0.0
    N[r] = (Nn / np.sqrt((Nn * Nn).sum(axis=1))[:, None]).astype(np.float32)
    D[r] = 0.0
    D[r, third] = sign
    perp[r] = True
    # D = N and D = -N for hashed N
    r = np.arange(8192, 8192 + 8192)
    D[r] = N[r] * np.where(np.arange(r.size) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None]
    par[r] = True
    F0[perp | par, 0] = 0.0
    return np.concatenate([F0, N, D], axis=1), {"perp": perp, "par": par}


def fresnel_guards(items, masks, out):
    """counted from the ORACLE's results: with F0.x = 0 the result's x is (1 - |N . D|)^5 -- 1 where the dot product is 0, +0 where it
    is exactly 1, negative where rounding put it above 1"""
    x = np.asarray(out, dtype=np.float32)[:, 0]
    return {"dot_zero": int((masks["perp"] & (bits(x) == ONE)).sum()), "dot_exactly_one": int((masks["par"] & (bits(x) == 0)).sum()),
            "dot_above_one": int((masks["par"] & (x < 0)).sum()), "F0_one_rows": int((bits(items[:, :3]) == ONE).all(axis=1).sum())}


FRESNEL_GUARD_MIN = {"dot_zero": 100, "dot_exactly_one": 100, "dot_above_one": 100, "F0_one_rows": 1000}


# ------------------------------------------------------------------------------------------------ LCG
LCG_TO_ONE = pow(48271, -1, LCG_M) * LCG_ONE % LCG_M      # the seed whose successor is 2^31 - 2 (its float is 1.0f)


def lcg_inputs():
    """int32 seeds: hashed over all 32 bits, the edges, and for 4,096 seeds the first 64 iterates, each fed back as a seed"""
    h = hashed(1 << 20, 0x1c6).astype(np.uint32).view(np.int32)
    edge = np.array([0, 1, 2, LCG_ONE, LCG_M, -1, -2, -(1 << 31), -(1 << 31) + 1, LCG_TO_ONE], dtype=np.int64).astype(np.int32)
    s = hashed(4096, 0xc4a1).astype(np.uint32).view(np.int32)
    chain = []
    for _ in range(64):
        chain.append(s)
        s = lcg_step(s).astype(np.int32)
    return np.concatenate([h, edge] + chain)


# ------------------------------------------------------------------------------------------------ cosine-lobe direction
def cornell_normals():
    """the distinct geometric normals of the Cornell box's triangles, as the triangle constructor computes them, in both orientations"""
    from opencl_path_tracer_amd import api, scenes
    spec = scenes.cornell_box()
    N = np.concatenate([api.triangles_from_vertices(v, m)["N"][:, :3] for v, m in spec.objects])
    N = fl(np.unique(bits(N), axis=0))
    return np.concatenate([N, -N])


def diffuse_normals(extra):
    e = int(bits(np.float32(0.001))[0])
    thr = fl(np.array([e - 1, e, e + 1], dtype=np.uint32))                            # 0.001f, one ulp below and above
    rows = [AXES, np.array([[0, 1, 0], [0, -1, 0]], dtype=np.float32)]
    sg = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float32)
    for ax in thr:                                                                    # both small components at the threshold
        for az in thr:
            y = np.sqrt(np.float32(1.0) - ax * ax - az * az, dtype=np.float32)
            rows.append(sg * np.array([ax, y, az], dtype=np.float32))
    for t in thr:                                                                     # one at the threshold, the other far from it
        y = np.sqrt(np.float32(0.75) - t * t, dtype=np.float32)
        rows.append(sg * np.array([t, y, 0.5], dtype=np.float32))
        rows.append(sg * np.array([0.5, y, t], dtype=np.float32))
    rows += [unit_vectors(4096, 0xd1f0), np.asarray(extra, dtype=np.float32).reshape(-1, 3)]
    return np.concatenate(rows)


DIFFUSE_MIXED = (1, 2, 32, 63)        # lanes with rnd1 == 1.0f in a mixed wave


def diffuse_inputs(extra_normals):
    """items (n, 8) float32 {P, N, rnd1, rnd2}, laid out wave by wave (item i is lane i % 64 of wave i / 64):
    first waves whose 64 lanes all have rnd1 < 1 (inside the window of the square-root cores), then waves whose lanes all have rnd1 ==
    1.0f, then mixed waves with 1, 2, 32 and 63 lanes at 1.0f -- at lane 0, at lane 63, at both and at hashed lanes -- and a last wave
    that the items do not fill."""
    normals = diffuse_normals(extra_normals)

    def items(idx, salt, n1=None):
        k = idx.size
        mag = np.array([0.0, 500.0, 1e4], dtype=np.float32)[np.arange(k) % 3]
        P = (unit_vectors(k, salt) * mag[:, None]).astype(np.float32)
        n1 = lcg_states(k, salt + 7, below_one=True) if n1 is None else n1
        n2 = lcg_states(k, salt + 11)
        n2[::97] = LCG_ONE                                                            # rnd2 = 1.0f: theta just past 2 pi
        n2[1::97] = 1
        return np.concatenate([P, normals[idx], lcg_float(n1)[:, None], lcg_float(n2)[:, None]], axis=1).astype(np.float32)

    def pad64(a):
        return np.concatenate([a, a[:(-a.shape[0]) % 64]])

    every = np.tile(np.arange(normals.shape[0]), 4)
    inside = items(every, 0x1000)
    inside[::61, 6] = lcg_float(1)                                                    # the smallest output, 2^-31
    outside = items(np.arange(normals.shape[0]), 0x2000, n1=np.full(normals.shape[0], LCG_ONE, dtype=np.int64))
    waves = [pad64(inside), pad64(outside)]
    w = 0
    for k in DIFFUSE_MIXED:
        for place in ("lane0", "lane63", "both") + ("hashed",) * 6:
            order = np.argsort(hashed(64, 0x3000 + w), kind="stable")                 # a hashed permutation of the lanes
            first = {"lane0": [0], "lane63": [63], "both": [0, 63], "hashed": []}[place][:k]
            if k == 63 and place != "hashed":                                         # here the ONE in-window lane sits at 63 / 0 / hashed
                lanes = [x for x in range(64) if x != {"lane0": 63, "lane63": 0, "both": int(order[0])}[place]]
            else:
                lanes = (first + [int(x) for x in order if int(x) not in first])[:k]
            wave = items(hashed(64, 0x4000 + w).astype(np.int64) % normals.shape[0], 0x5000 + w)
            wave[lanes, 6] = 1.0
            waves.append(wave)
            w += 1
    tail = items(np.arange(37), 0x6000)
    tail[[0, 5, 36], 6] = 1.0
    waves.append(tail)
    return np.concatenate(waves)


def diffuse_wave_kinds(items):
    """per wave: how many of its lanes have rnd1 == 1.0f, and whether lane 0 / lane 63 is one of them (full waves only)"""
    out = bits(items[:, 6]) == ONE
    full = out[:out.size // 64 * 64].reshape(-1, 64)
    return full.sum(axis=1), full[:, 0], full[:, 63]


def diffuse_in_window(items):
    """per item, the vote diffuse_direction's lane casts for the IEEE cores: rsqrt_window(l2) of the frame's l2 and 2^-96 <= rnd1 < 1.
    (l2 in float64: for these normals it is nowhere near 2^-96 or inf, where its last bit would matter)"""
    N, rnd1 = items[:, 3:6].astype(np.float64), items[:, 6]
    yaxis = (np.abs(items[:, 3]) <= np.float32(0.001)) & (np.abs(items[:, 5]) <= np.float32(0.001))
    other = np.where(yaxis, N[:, 1], N[:, 0])
    l2 = N[:, 2] * N[:, 2] + other * other
    lo = 2.0 ** -96
    return (l2 >= 2 * lo) & (l2 < 1e30) & (rnd1 >= np.float32(lo)) & (rnd1 < np.float32(1.0))
