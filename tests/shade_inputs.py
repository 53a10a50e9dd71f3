"""The scene and the item lists of tests/test_gpu_shade_vertex.py (pt_debug_shade, the real shade_hit, against the oracle's iteration
body orc_shade_step_n) and the guards that say each list reaches the branch it is meant to reach.  Plain numpy plus the CPU oracle,
deterministic (hashes of the index, no random state), so everything is built and counted without a device (tests/test_shade_host.py).

An item is one row of 25 32-bit words {P, D, t, triangle, seed, inside, L, B, S, R, colour} (include/pt_api.h, oracle/pt_oracle.h); the
triangle is an index into triangles() (add order) here and the packed index on the device, t is filled in from the oracle's result.
Item i of a list runs on lane i % 64 of wave i / 64; every list is a whole number of waves."""
import functools

import numpy as np

import spec_inputs as S
from oracle import oracle_py as O

W = H = 8
VIEW = (60.0, 0.0, 0.0, (-500.0, -500.0, 1149.037842))        # fov, yaw, pitch, shift: the eye at (0, 0, -150)
SQRT_WINDOW_LO = 2.0 ** -96                                   # kSqrtWindowLo of pt_device.hpp (tests/test_shade_host.py reads it there)
ONE3, ZERO3 = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


def camera():
    return O.make_camera(VIEW[0], VIEW[1], VIEW[2], VIEW[3], W, H)


# ------------------------------------------------------------------------------------------------ scene
def _mat(kd=ZERO3, ks=ZERO3, em=ZERO3, F0=ZERO3, n=0.0, sh=0.0, t=0):
    m = np.zeros(1, dtype=O.MATERIAL)
    m["kd"][0, :3], m["ks"][0, :3], m["emission"][0, :3], m["F0"][0, :3] = kd, ks, em, F0
    m["n"], m["shininess"], m["type"] = n, sh, t
    return m


KD, KS = (0.75, 0.6, 0.45), (0.3, 0.25, 0.5)
M_PLAIN, M_SH0, M_SH1, M_SHF, M_SH200, M_CHROME, M_MIRROR0, M_MIRROR1, M_GLASS, M_GLASS1, M_GLASSLT1, M_GLASSF0, M_EMIT, M_OTHER = range(14)
GLASS = (M_GLASS, M_GLASS1, M_GLASSLT1, M_GLASSF0)


def materials():
    """records authored directly (add_Material takes a record), so that F0 and n are free of the constructor's formula"""
    chrome = O.make_material(ZERO3, ZERO3, ZERO3, (3.1, 3.1, 2.0), (3.3, 3.3, 2.9), 0.0, 1)       # F0 through the reference's formula
    return np.concatenate([
        _mat(kd=KD, sh=10.0),                                   # diffuse, ks = 0: the _pad / `plain` shortcut
        _mat(kd=KD, ks=KS, sh=0.0), _mat(kd=KD, ks=KS, sh=1.0), _mat(kd=KD, ks=KS, sh=2.5), _mat(kd=KD, ks=KS, sh=200.0),
        chrome, _mat(F0=ZERO3, t=1), _mat(F0=ONE3, t=1),
        _mat(F0=(0.04, 0.04, 0.04), n=1.5, t=2), _mat(F0=(0.04, 0.05, 0.06), n=1.0, t=2), _mat(F0=(0.02, 0.02, 0.02), n=0.75, t=2),
        _mat(F0=ZERO3, n=1.5, t=2),                             # prob = 0 at normal incidence: 1 / prob is inf, factor_R becomes NaN
        _mat(kd=(0.1, 0.1, 0.1), em=(12.0, 10.0, 8.0), t=3),
        _mat(kd=KD, ks=KS, em=(1.0, 2.0, 3.0), F0=(0.5, 0.5, 0.5), n=1.5, sh=5.0, t=7)])      # a type the plain path leaves unchanged


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum())


def _orientation(c, n):
    n = _unit(n)
    u = _unit(np.cross(n, (0.0, 1.0, 0.0)) if abs(n[1]) < 0.9 else np.cross(n, (1.0, 0.0, 0.0)))
    return np.asarray(c, dtype=np.float64), u, np.cross(n, u)


# centre, u, v: the triangle is {c - 300 u - 200 v, c + 300 u - 200 v, c + 400 v}; the first three are axis planes (normals with exact
# +-0 components), the last has |N.x|, |N.z| <= 0.001 (the y-axis branch of the tangent frame)
ORIENT = [(np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 1.0, 0])),
          (np.array([100.0, -50, 200]), np.array([1.0, 0, 0]), np.array([0, 0, 1.0])),
          (np.array([-300.0, 0, 100]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])),
          _orientation((200, 100, 300), (1, 2, 3)), _orientation((-100, 250, -50), (-2, 1, -0.5)), _orientation((50, 300, 50), (0.0005, 1, -0.0003))]
Z0_MATS = (M_PLAIN, M_SH0, M_SH1, M_SHF, M_SH200, M_CHROME, M_GLASS, M_GLASS1, M_GLASSLT1, M_GLASSF0, M_EMIT)


@functools.lru_cache(maxsize=None)
def scene():
    """(TRIANGLE records in add order, per triangle its orientation index): one triangle per material in varied orientations and
    windings, then for Z0_MATS one triangle in the plane z = 0 through the origin in each winding (N = (+-0, +-0, +-1))"""
    tris, orient = [], []

    def add(o, mati, flip):
        c, u, v = ORIENT[o]
        r = [c - 300 * u - 200 * v, c + 300 * u - 200 * v, c + 400 * v]
        if flip:
            r = r[::-1]                                         # (on an axis plane this order gives the normal a -0 component)
        tris.append(O.make_triangle(*[x.astype(np.float32) for x in r], mati))
        orient.append(o)

    for m in range(14):
        add(m % 6 if m % 6 else 3 + m % 3, m, m % 2 == 1)       # (the z = 0 plane is left to the second group)
    for m in Z0_MATS:
        add(0, m, False)
        add(0, m, True)
    return np.concatenate(tris), np.array(orient)


def triangles():
    return scene()[0]


def z0(mati, flipped=False):
    """index of the z = 0 triangle of material mati"""
    return 14 + 2 * Z0_MATS.index(mati) + int(flipped)


def tri_type():
    return materials()["type"][triangles()["mati"]]


# ------------------------------------------------------------------------------------------------ items
def seeds(n, salt):
    return S.lcg_states(n, salt).astype(np.int32)


def items(tri, D, a=0.0, b=0.0, s=100.0, seed=None, inside=0, L=ONE3, B=ONE3, Sf=ONE3, R=ONE3, C=ZERO3, salt=1):
    """n items: the ray from P = Q - s D along D, Q = c + a u + b v a point well inside triangle `tri` (|a|, |b| <= 100)"""
    D = np.asarray(D, dtype=np.float32).reshape(-1, 3)
    n = D.shape[0]
    tri = np.broadcast_to(np.asarray(tri, dtype=np.int64), (n,))
    o = scene()[1][tri]
    c, u, v = (np.stack([ORIENT[k][j] for k in o]) for j in range(3))
    Q = c + np.broadcast_to(a, (n,))[:, None] * u + np.broadcast_to(b, (n,))[:, None] * v
    P = (Q - np.broadcast_to(np.asarray(s, dtype=np.float64), (n,))[:, None] * D.astype(np.float64)).astype(np.float32)
    it = np.zeros((n, 25), dtype=np.uint32)
    it[:, 0:3], it[:, 3:6] = S.bits(P), S.bits(D)
    it[:, 7] = tri.astype(np.uint32)
    it[:, 8] = (seeds(n, salt) if seed is None else np.broadcast_to(np.asarray(seed, dtype=np.int32), (n,))).view(np.uint32)
    it[:, 9] = np.broadcast_to(np.asarray(inside, dtype=np.uint32), (n,))
    for k, f in enumerate((L, B, Sf, R, C)):
        it[:, 10 + 3 * k:13 + 3 * k] = S.bits(np.broadcast_to(np.asarray(f, dtype=np.float32), (n, 3)))
    return it


def pad64(a):
    """a whole number of waves: the list's first items again"""
    return np.concatenate([a, a[:(-a.shape[0]) % 64]])


def run_oracle(it, iterations=8):
    return O.shade_step_n(it, triangles(), materials(), camera(), iterations)


def device_items(it, out, packed_of):
    """the device's items: the oracle's t of each hit and the packed index of each triangle (packed_of[add-order index])"""
    d = it.copy()
    d[:, 6] = out[:, 0]
    d[:, 7] = np.asarray(packed_of, dtype=np.uint32)[it[:, 7]]
    return d


def kinds(it, out):
    """per item what the oracle's step did: 0 diffuse, 1 mirror, 2 glass reflected, 3 glass refracted, 4 emitter, 5 any other type,
    -1 the oracle's triangle_intersect reports a miss"""
    t = tri_type()[it[:, 7]]
    k = np.where(t == 0, 0, np.where(t == 1, 1, np.where(t == 2, 2, np.where(t == 3, 4, 5))))
    k = np.where((t == 2) & (out[:, 8] != it[:, 9]), 3, k)
    return np.where(S.fl(out[:, 0]) > 0, k, -1)


def normals(tri):
    return triangles()["N"][np.asarray(tri), :3]


def camera_dirs(n):
    """n directions out of the oracle's own normalize (camera_get_ray)"""
    cam, out = camera(), np.zeros(n, dtype=O.RAY)
    for i in range(n):
        O.lib().orc_camera_get_ray(out[i:i + 1].ctypes.data_as(O.C.c_void_p), i % (W * H), cam.ctypes.data_as(O.C.c_void_p), float(S.lcg_float(1 + 7919 * i)),
                                   float(S.lcg_float(3 + 104729 * i)))
    return out["D"][:, :3].copy()


# ---- incidence
def incidence_list():
    """every triangle from both faces: normal incidence (D = -+N, the record's bits), hashed directions, directions out of the oracle's
    normalize, directions with exact zero and with denormal components; every glass item with `inside` off and on"""
    N, parts = triangles()["N"][:, :3], []
    cd = camera_dirs(4)
    for t in range(N.shape[0]):
        k = int(np.argmax(np.abs(N[t])))
        ax = np.zeros(3, dtype=np.float32)
        ax[k] = 1.0
        den = ax.copy()
        den[(k + 1) % 3], den[(k + 2) % 3] = S.fl(np.array([1, 0x80000003], dtype=np.uint32))          # a denormal of either sign
        D = np.concatenate([N[t:t + 1], S.unit_vectors(6, 0x100 + t), cd, ax[None], den[None], (ax * np.float32(0.6) + np.roll(ax, 1) * np.float32(0.8))[None]])
        dn = D.astype(np.float64) @ N[t].astype(np.float64)
        D[np.abs(dn) < 0.05] = N[t]                                                  # too flat for a hit point well inside: normal incidence
        dn = D.astype(np.float64) @ N[t].astype(np.float64)
        for face in (1.0, -1.0):                                                     # face > 0: the ray meets the side N points to
            Df = D * np.where(dn * face > 0, -1.0, 1.0).astype(np.float32)[:, None]
            for inside in ((0, 1) if tri_type()[t] == 2 else (0,)):
                parts.append(items(t, Df, a=37.0, b=-21.0, inside=inside, salt=0x200 + 4 * t + int(face > 0) + 2 * inside))
    # normal incidence on the F0 = 0 glass with the LCG stuck at 0 (draw 0.0f): prob = 0, the lane reflects, 1 / prob is inf and factor_R NaN
    for flipped in (False, True):
        t = z0(M_GLASSF0, flipped)
        for inside in (0, 1):
            parts.append(items(t, np.concatenate([N[t:t + 1], -N[t:t + 1]]), a=5.0, b=5.0, seed=0, inside=inside))
    return pad64(np.concatenate(parts))


# ---- grazing: dot(D, N) a few ulps (denormals) either side of 0, and exactly 0
GRAZE_K = (1, 2, 3, -1, -2, -3)


def grazing_list():
    """On the z = 0 triangles N = (+-0, +-0, +-1), so dot(D, N) is +-D.z exactly.  D = (cos a, sin a, k d) and P.z = -100 k d for d
    the smallest denormal, 2^-126 and 1e-30: triangle_intersect's t is 100 exactly and the hit point has z = 0; k > 0 meets the face
    N does not point to.  Then D.z = +-0 with P.z = 0: dot(D, N) is exactly 0, the reference divides by it and reports no hit."""
    parts, ang = [], np.arange(8) * 0.7 + 0.1
    xy = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    for m in Z0_MATS:
        for flipped in (False, True):
            for d in (2.0 ** -149, 2.0 ** -126, 1e-30):
                for k in GRAZE_K:
                    D = np.concatenate([xy, np.full((8, 1), k * d)], axis=1).astype(np.float32)
                    it = items(z0(m, flipped), D, a=10.0, b=5.0, inside=int(k > 0) if m in GLASS else 0, salt=0x900 + m + k)
                    it[:, 2] = S.bits((-100.0 * D[:, 2].astype(np.float64)).astype(np.float32))
                    parts.append(it)
            for z in (0.0, -0.0):
                D = np.concatenate([xy, np.full((8, 1), z)], axis=1).astype(np.float32)
                it = items(z0(m, flipped), D, a=10.0, b=5.0, salt=0x990 + m)
                it[:, 2] = 0
                parts.append(it)
    return pad64(np.concatenate(parts))


# ---- total internal reflection
def disc_of(cosa, n):
    """new_ray_refractive's disc (prog.cl:231-232) in float32: 1 - (fma(-cosa, cosa, 1) / n) / n.  The fma is exact here: cosa^2 has 48
    bits, so 1 - cosa^2 is exact in float64 and one rounding takes it to float32."""
    cosa = np.asarray(cosa, dtype=np.float32)
    s2 = (1.0 - cosa.astype(np.float64) ** 2).astype(np.float32)
    return np.float32(1.0) - (s2 / np.float32(n)) / np.float32(n)


TIR_CASES = ((M_GLASS, 1), (M_GLASSLT1, 0))      # (material, inside): n = 1 / 1.5 inside the n = 1.5 glass, n = 0.75 entering the n < 1 one


def tir_list():
    """On a z = 0 glass triangle cosa = dot(-D, N) is -+D.z exactly, so D = (sqrt(1 - c^2), 0, -c) puts cosa = c: c runs ulp by ulp, 96
    either side of the float nearest the critical cosine sqrt(1 - n^2); the seed's next draw is above prob (0.99), so the lane refracts
    exactly where disc > 0.  Returns (items, disc per item)."""
    seed_hi = S.LCG_ONE * pow(48271, -1, S.LCG_M) % S.LCG_M - 0      # the seed whose draw is (2^31 - 2) / 2^31 = 1.0f
    parts, disc = [], []
    for m, inside in TIR_CASES:
        n = float(materials()["n"][m])
        nr = np.float32(1.0) / np.float32(n) if inside else np.float32(n)
        c0 = int(S.bits(np.float32(np.sqrt(1.0 - float(nr) ** 2)))[0])
        c = S.fl(np.arange(c0 - 96, c0 + 96, dtype=np.uint32))
        D = np.stack([np.sqrt(1.0 - c.astype(np.float64) ** 2), np.zeros(c.size), -c.astype(np.float64)], axis=1).astype(np.float32)
        parts.append(items(z0(m), D, a=-20.0, b=30.0, inside=inside, seed=seed_hi))
        disc.append(disc_of(c, nr))
    return np.concatenate(parts), np.concatenate(disc)


# ---- the reflect / refract coin
LCG_INV = pow(48271, -1, S.LCG_M)


def prob_of(it):
    """the oracle's prob of a glass item: its fresnel() on the item's F0, N, D, then ((F.x + F.y) + F.z) / 3.0f"""
    F0 = materials()["F0"][triangles()["mati"][it[:, 7]], :3]
    F = O.fresnel_n(np.concatenate([F0, normals(it[:, 7]), S.fl(it[:, 3:6])], axis=1))
    return ((F[:, 0] + F[:, 1]) + F[:, 2]) / np.float32(3.0)


def coin_list():
    """Glass items at hashed incidence (disc > 0 for all of them: outside the glass, or inside at under 30 degrees), each three times:
    the seed whose next draw is the float just below prob, prob itself, just above.  The LCG is x' = 48271 x mod 2^31 - 1 and the draw
    x' / 2^31, so the seed is x' 48271^-1 for x' = prob 2^31 (an integer: prob > 2^-7 has at most 24 significant bits).
    Returns (items, relation per item: -1 / 0 / 1)."""
    base = []
    for m in (M_GLASS, M_GLASS1, M_GLASSLT1):
        for inside in (0, 1):
            for flipped in (False, True):
                th = (S.unit24(S.hashed(16, 0xc01 + m)).astype(np.float64)) * (0.5 if inside or m == M_GLASSLT1 else 1.4)
                ph = S.unit24(S.hashed(16, 0xc02 + m)).astype(np.float64) * 6.28
                D = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * (-1 if inside else 1)], axis=1)
                base.append(items(z0(m, flipped), D.astype(np.float32), a=15.0, b=-40.0, inside=inside))
    base = np.concatenate(base)
    prob = prob_of(base)
    assert (prob > 2.0 ** -7).all() and (prob < 0.5).all()
    pb = S.bits(prob).astype(np.int64)
    parts, rel = [], []
    for d in (-1, 0, 1):
        target = S.fl((pb + d).astype(np.uint32)).astype(np.float64) * 2147483648.0
        x = target.astype(np.int64)
        assert (x == target).all() and (x >= 1).all() and (x < S.LCG_M).all()
        it = base.copy()
        it[:, 8] = np.array([int(v) * LCG_INV % S.LCG_M for v in x], dtype=np.int64).astype(np.uint32)
        parts.append(it)
        rel.append(np.full(base.shape[0], d))
    order = np.arange(3 * base.shape[0]).reshape(3, -1).T.reshape(-1)                # below, equal, above of one item on neighbouring lanes
    return np.concatenate(parts)[order], np.concatenate(rel)[order]


# ---- state
STATE_VALUES = (1.0, 1e-30, 1e30, 0.0, -0.0, np.inf, -2.5)


def state_list():
    """every kind of hit with each factor in turn at 1, small, large, zero, negative zero, infinite and negative (the other factors hashed
    in (0, 1)) and a non-zero colour; glass with `inside` off and on and a draw below and above prob"""
    parts = []
    lo, hi = 1 * LCG_INV % S.LCG_M, S.LCG_ONE * LCG_INV % S.LCG_M                    # the draw 2^-31 (reflects) and 1.0f (refracts if it may)
    for t, sd in ((M_PLAIN, None), (M_SH200, None), (M_CHROME, None), (M_MIRROR1, None), (M_GLASS, lo), (M_GLASS, hi), (M_GLASSF0, hi), (M_EMIT, None),
                  (M_OTHER, None)):
        for which in range(4):
            for val in STATE_VALUES:
                for inside in ((0, 1) if t in GLASS else (0,)):
                    f = [S.unit24(S.hashed(3, 0x57a + 16 * which + k)) for k in range(4)]
                    f[which] = np.array([val, 1.0, val], dtype=np.float32)
                    D = S.unit_vectors(1, 0xd00 + t + which)
                    N = normals(t)
                    D = (D * np.float32(-1.0 if float(D[0].astype(np.float64) @ N.astype(np.float64)) > 0 else 1.0)) if abs(float(D[0].astype(np.float64) @ N.astype(np.float64))) > 0.05 else -N[None]
                    parts.append(items(t, D, a=-60.0, b=45.0, seed=sd, inside=inside, L=f[0], B=f[1], Sf=f[2], R=f[3], C=(0.25, 3.0, 1e-3), salt=0xe00 + t))
    return pad64(np.concatenate(parts))


# ---- diffuse with a lobe: the halfway vector
def lobe_list():
    """Lobe materials on their z = 0 triangles, the hit point placed so that view = normalize(eye - hp) is a chosen function of the NEW
    direction rD (which depends on N and the seed only: a first pass of the oracle gives it):
      'opposite'  view = -rD            the halfway vector is the rounding noise of the sum, or exactly 0 (then NaN, and max0 gives 0)
      'zero'      view = rD - 2 (N.rD) N     view + rD is tangential: N.H = 0 up to rounding
      'one'       view = 2 (N.rD) N - rD     view + rD is along N: N.H = 1 or just below it
    The hit point is where the line from the eye along -view meets the plane z = 0; seeds whose point falls outside the triangle's core
    are passed over.  The ray arrives from the side that makes rD's hemisphere the right one (the far side of the eye for the first two).
    Returns (items, class per item: 0 / 1 / 2)."""
    eye = camera()["eye"][0, :3].astype(np.float64)
    parts, cls = [], []
    for m in (M_SH0, M_SH1, M_SHF, M_SH200):
        t = z0(m)
        for c, far in ((0, True), (1, True), (2, False)):
            # the eye is at z < 0; far: the ray travels towards -z (it meets the z > 0 face), so the flipped normal is (0, 0, 1)
            Nf = np.array([0.0, 0.0, 1.0 if far else -1.0])
            D = np.tile(np.array([[0.3, -0.2, -1.0 if far else 1.0]]), (256, 1))
            D = (D / np.sqrt((D * D).sum(axis=1))[:, None]).astype(np.float32)
            sd = seeds(256, 0x10be + 8 * m + c)
            probe = run_oracle(items(t, D, seed=sd))
            rD = S.fl(probe[:, 4:7]).astype(np.float64)
            nd = rD @ Nf
            view = -rD if c == 0 else (rD - 2 * nd[:, None] * Nf) if c == 1 else (2 * nd[:, None] * Nf - rD)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = eye[2] / view[:, 2]                                              # eye - r view has z = 0
            Q = eye - r[:, None] * view
            ok = (r > 0) & (np.abs(Q[:, 0]) <= 100) & (np.abs(Q[:, 1]) <= 100) & (nd > 0.05)
            k = np.flatnonzero(ok)[:32]
            parts.append(items(t, D[k], a=Q[k, 0], b=Q[k, 1], seed=sd[k]))
            cls.append(np.full(k.size, c))
    return np.concatenate(parts), np.concatenate(cls)


def halfway_dot(it, out):
    """float64: N.H of a lobe item from the oracle's new ray (hp = new P - 0.001 N)"""
    eye = camera()["eye"][0, :3].astype(np.float64)
    Pn, rD = S.fl(out[:, 1:4]).astype(np.float64), S.fl(out[:, 4:7]).astype(np.float64)
    Nf = np.sign(-S.fl(it[:, 5]).astype(np.float64))[:, None] * np.array([0.0, 0.0, 1.0])       # z = 0 triangles: against the ray
    hp = Pn - 0.001 * Nf
    view = eye - hp
    view /= np.sqrt((view * view).sum(axis=1))[:, None]
    h = view + rD
    return (h * Nf).sum(axis=1) / np.sqrt((h * h).sum(axis=1)), np.sqrt((h * h).sum(axis=1))


# ---- wave composition
KIND_NAMES = ("diffuse", "mirror", "glass-reflect", "glass-refract", "emitter")


def wave_lists(pool_items, pool_kinds):
    """From a pool of items whose kind the oracle has decided: waves of one kind, every pair of kinds on alternating lanes, one straggler
    lane of one kind (at a hashed lane) among 63 of another.  Returns (items, per wave a (kind a, kind b, lanes of b) triple)."""
    pools = [pool_items[pool_kinds == k] for k in range(5)]
    assert all(p.shape[0] >= 64 for p in pools), [p.shape[0] for p in pools]
    waves, what = [], []
    for a in range(5):
        waves.append(pools[a][:64])
        what.append((a, a, 0))
    for a in range(5):
        for b in range(a + 1, 5):
            w = pools[a][:64].copy()
            w[1::2] = pools[b][1:64:2]
            waves.append(w)
            what.append((a, b, 32))
    for a in range(5):
        for b in range(5):
            if a != b:
                w = pools[a][64 - 64:64].copy()
                w[int(S.hashed(1, 0x5a0 + 5 * a + b)[0] % 64)] = pools[b][7]
                waves.append(w)
                what.append((a, b, 1))
    return np.concatenate(waves), what


def window_lists(pool_items, pool_kinds):
    """Waves by where their lanes' operands lie against the window of the IEEE cores (x >= kSqrtWindowLo = 2^-96, finite):
    the shared tail's rsqrt_rn takes dot(dnew, dnew) -- inside for every unit D; outside for a mirror item whose D and distance are scaled
    by 2^-60 and 2^60 (|dnew|^2 = 2^-120; the same hit point, the same new direction after normalisation); diffuse_direction's cores
    take rnd1 -- outside when the draw is 1.0f (seed LCG_TO_ONE).  Waves: all lanes inside, all outside (mirror; diffuse), mixed at
    lanes 0 / 63 / every other lane / one straggler.  Returns (items, per item True where the lane's operand is outside)."""
    mir, dif = pool_items[pool_kinds == 1][:64], pool_items[pool_kinds == 0][:64]
    out_m = mir.copy()
    D, P = S.fl(mir[:, 3:6]).astype(np.float64), S.fl(mir[:, 0:3]).astype(np.float64)
    Q = P + 100.0 * D
    out_m[:, 3:6] = S.bits((D * 2.0 ** -60).astype(np.float32))
    out_m[:, 0:3] = S.bits((Q - (100.0 * 2.0 ** 60) * (D * 2.0 ** -60).astype(np.float32).astype(np.float64)).astype(np.float32))
    out_d = dif.copy()
    out_d[:, 8] = S.LCG_TO_ONE
    waves, flags = [mir, dif, out_m, out_d], [np.zeros(64, bool), np.zeros(64, bool), np.ones(64, bool), np.ones(64, bool)]
    for inside, outside in ((mir, out_m), (dif, out_d), (dif, out_m), (mir, out_d)):
        for lanes in ([0], [63], list(range(0, 64, 2)), [int(S.hashed(1, 0x3d)[0] % 62) + 1], [k for k in range(64) if k != 17]):
            w, f = inside.copy(), np.zeros(64, bool)
            w[lanes], f[lanes] = outside[lanes], True
            waves.append(w)
            flags.append(f)
    return np.concatenate(waves), np.concatenate(flags)


def tail_l2(it):
    """dot(D, D) of an item in float64 (a mirror's |dnew|^2 is |D|^2 up to rounding)"""
    D = S.fl(it[:, 3:6]).astype(np.float64)
    return (D * D).sum(axis=1)


# ------------------------------------------------------------------------------------------------ all lists
@functools.lru_cache(maxsize=None)
def build_all():
    """{name: items} in whole waves, the oracle's result per list and pass ({name: (out at 8 iterations, out in preview mode)}) and the
    side tables of the guards"""
    L, meta = {}, {}
    L["incidence"] = incidence_list()
    L["grazing"] = grazing_list()
    L["tir"], meta["tir_disc"] = tir_list()
    L["coin"], meta["coin_rel"] = coin_list()
    L["state"] = state_list()
    L["lobe"], meta["lobe_class"] = lobe_list()
    for k in ("tir", "coin", "lobe"):
        meta[k + "_n"] = L[k].shape[0]
        L[k] = pad64(L[k])
    pool = np.concatenate([L["incidence"], L["coin"]])
    pk = kinds(pool, run_oracle(pool))
    L["waves"], meta["waves_what"] = wave_lists(pool, pk)
    L["window"], meta["window_outside"] = window_lists(pool, pk)
    assert all(v.shape[0] % 64 == 0 for v in L.values())
    out = {k: (run_oracle(v, 8), run_oracle(v, 1)) for k, v in L.items()}
    return L, out, meta


# ------------------------------------------------------------------------------------------------ guards
def draws(seed, k=1):
    """the k-th draw (1-based) of lcg_rand from each seed, as the float it returns"""
    s = np.asarray(seed, dtype=np.uint32).view(np.int32)
    for _ in range(k):
        s = S.lcg_step(s).astype(np.int32)
    return S.lcg_float(s)


def guards():
    """counts, from the inputs and the ORACLE's results, that say each list reaches what it is built for (GUARD_MIN holds the least
    each must reach; tests/test_shade_host.py asserts them without a device, tests/test_gpu_shade_vertex.py again before it compares)"""
    L, out, meta = build_all()
    g = {}
    N64 = lambda it: normals(it[:, 7]).astype(np.float64)
    D64 = lambda it: S.fl(it[:, 3:6]).astype(np.float64)
    # incidence
    it, o = L["incidence"], out["incidence"][0]
    k = kinds(it, o)
    for i, name in enumerate(KIND_NAMES + ("other",)):
        g["incidence_" + name] = int((k == i).sum())
    g["incidence_misses"] = int((k < 0).sum())
    dn = (D64(it) * N64(it)).sum(axis=1)
    g["incidence_front"], g["incidence_back"] = int((dn < 0).sum()), int((dn > 0).sum())
    Nb, Db = S.bits(normals(it[:, 7])), it[:, 3:6]
    g["incidence_normal"] = int(((Db == Nb).all(axis=1) | (Db == (Nb ^ 0x80000000)).all(axis=1)).sum())
    g["incidence_zero_component"] = int(((Db & 0x7fffffff) == 0).any(axis=1).sum())
    g["incidence_denormal_component"] = int((((Db & 0x7f800000) == 0) & ((Db & 0x7fffff) != 0)).any(axis=1).sum())
    g["incidence_glass_inside"] = int(((tri_type()[it[:, 7]] == 2) & (it[:, 9] == 1)).sum())
    g["incidence_glass_outside"] = int(((tri_type()[it[:, 7]] == 2) & (it[:, 9] == 0)).sum())
    g["prob_zero_nan_factor"] = int(((triangles()["mati"][it[:, 7]] == M_GLASSF0) & np.isnan(S.fl(o[:, 18:21])).any(axis=1)).sum())
    Nall = S.bits(triangles()["N"][:, :3])
    g["normals_negative_zero"], g["normals_positive_zero"] = int((Nall == 0x80000000).sum()), int((Nall == 0).sum())
    # grazing: the exact zeros are misses and nothing else is; every hit has t = 100 (exactly for the denormals)
    it, o = L["grazing"], out["grazing"][0]
    dz, t = S.fl(it[:, 5]), S.fl(o[:, 0])
    g["grazing_exact_zero_misses"] = int(((dz == 0) & (t == -1.0)).sum())
    g["grazing_wrong"] = int(((dz == 0) != (t == -1.0)).sum() + ((dz != 0) & (np.abs(t - 100.0) > 1e-3)).sum())
    g["grazing_flip"], g["grazing_no_flip"] = int(((dz * S.fl(Nb_z(it))) > 0).sum()), int(((dz * S.fl(Nb_z(it))) < 0).sum())
    g["grazing_denormal_dot"] = int(((dz != 0) & (np.abs(dz) < 2.0 ** -126)).sum())
    # total internal reflection
    n, disc = meta["tir_n"], meta["tir_disc"]
    refr = kinds(L["tir"][:n], out["tir"][0][:n]) == 3
    g["tir_disc_positive_small"] = int(((disc > 0) & (disc < 1e-6)).sum())
    g["tir_disc_negative_small"] = int(((disc < 0) & (disc > -1e-6)).sum())
    g["tir_disc_zero"] = int((disc == 0).sum())
    g["tir_wrong"] = int((refr != (disc > 0)).sum())
    # coin
    n, rel = meta["coin_n"], meta["coin_rel"]
    it = L["coin"][:n]
    rnd, prob = draws(it[:, 8]), prob_of(it)
    refr = kinds(it, out["coin"][0][:n]) == 3
    g["coin_below"], g["coin_equal"], g["coin_above"] = int((rnd < prob).sum()), int((rnd == prob).sum()), int((rnd > prob).sum())
    g["coin_wrong"] = int((np.sign(rnd.astype(np.float64) - prob) != rel).sum() + (refr != (rnd > prob)).sum())
    g["coin_inside"], g["coin_outside"] = int((it[:, 9] == 1).sum()), int((it[:, 9] == 0).sum())
    # state
    it, o = L["state"], out["state"][0]
    for v in STATE_VALUES:
        g["state_%r" % v] = int((it[:, 10:22] == S.bits(np.float32(v))[0]).any(axis=1).sum())
    g["state_nonzero_colour"] = int((it[:, 22:25] != 0).all(axis=1).sum())
    g["state_nan_results"] = int(np.isnan(S.fl(o[:, 9:24])).any(axis=1).sum())
    for i, name in enumerate(KIND_NAMES + ("other",)):
        g["state_" + name] = int((kinds(it, o) == i).sum())
    # lobe
    n, cls = meta["lobe_n"], meta["lobe_class"]
    nh, hl = halfway_dot(L["lobe"][:n], out["lobe"][0][:n])
    g["lobe_opposite"] = int(((cls == 0) & (hl < 1e-5)).sum())
    g["lobe_nh_zero"] = int(((cls == 1) & (np.abs(nh) < 1e-5)).sum())
    g["lobe_nh_one"] = int(((cls == 2) & (nh > 1 - 1e-6)).sum())
    g["lobe_wrong"] = n - g["lobe_opposite"] - g["lobe_nh_zero"] - g["lobe_nh_one"]
    g["lobe_shininess_values"] = int(np.unique(triangles()["mati"][L["lobe"][:n, 7]]).size)
    # waves: each wave holds the kinds it is labelled with, by the oracle's decision
    k = kinds(L["waves"], out["waves"][0]).reshape(-1, 64)
    g["waves_one_kind"] = g["waves_pairs"] = g["waves_straggler"] = g["waves_wrong"] = 0
    for row, (a, b, nb) in zip(k, meta["waves_what"]):
        ok = int((row == b).sum()) == (64 if a == b else nb) and int((row == a).sum()) == 64 - (0 if a == b else nb)
        g["waves_wrong"] += not ok
        g["waves_one_kind" if a == b else "waves_pairs" if nb == 32 else "waves_straggler"] += ok
    # window: the lanes flagged as outside are the ones whose operand is outside, and every kind of wave is there
    it, flag = L["window"], meta["window_outside"]
    mirror = tri_type()[it[:, 7]] == 1
    outside = np.where(mirror, tail_l2(it) < SQRT_WINDOW_LO, S.bits(draws(it[:, 8])) == S.ONE)
    g["window_wrong"] = int((outside != flag).sum() + (kinds(it, out["window"][0]) != np.where(mirror, 1, 0)).sum())
    per = flag.reshape(-1, 64).sum(axis=1)
    g["window_waves_inside"], g["window_waves_outside"] = int((per == 0).sum()), int((per == 64).sum())
    g["window_waves_mixed"] = int(((per > 0) & (per < 64)).sum())
    g["window_waves_one_lane"] = int(((per == 1) | (per == 63)).sum())
    return g


def Nb_z(it):
    return S.bits(normals(it[:, 7])[:, 2])


GUARD_MIN = {"incidence_diffuse": 300, "incidence_mirror": 100, "incidence_glass-reflect": 50, "incidence_glass-refract": 200, "incidence_emitter": 50,
             "incidence_other": 20, "incidence_front": 500, "incidence_back": 500, "incidence_normal": 72, "incidence_zero_component": 72,
             "incidence_denormal_component": 36, "incidence_glass_inside": 200, "incidence_glass_outside": 200, "prob_zero_nan_factor": 1,
             "normals_negative_zero": 4, "normals_positive_zero": 4, "grazing_exact_zero_misses": 352, "grazing_flip": 1000, "grazing_no_flip": 1000,
             "grazing_denormal_dot": 1000, "tir_disc_positive_small": 8, "tir_disc_negative_small": 8, "coin_below": 32, "coin_equal": 32,
             "coin_above": 32, "coin_inside": 100, "coin_outside": 100, "state_nonzero_colour": 300, "state_nan_results": 4, "state_diffuse": 50,
             "state_mirror": 50, "state_glass-reflect": 50, "state_glass-refract": 50, "state_emitter": 20, "state_other": 20, "lobe_opposite": 64,
             "lobe_nh_zero": 64, "lobe_nh_one": 64, "lobe_shininess_values": 4, "waves_one_kind": 5, "waves_pairs": 10, "waves_straggler": 20,
             "window_waves_inside": 2, "window_waves_outside": 2, "window_waves_mixed": 20, "window_waves_one_lane": 8}
GUARD_MIN.update({"state_%r" % v: 30 for v in STATE_VALUES})
GUARD_ZERO = ("incidence_misses", "grazing_wrong", "tir_wrong", "coin_wrong", "lobe_wrong", "waves_wrong", "window_wrong")


def check_guards(g):
    for k, least in GUARD_MIN.items():
        assert g[k] >= least, (k, g[k], least)
    for k in GUARD_ZERO:
        assert g[k] == 0, (k, g[k])


def load_scene(api, device):
    """the scene on a context: (Scene, packed index of every add-order triangle)"""
    sc = api.Scene(W, H, device=device)
    for m in materials():
        sc.add_Material(m.reshape(1))
    for k in range(0, triangles().shape[0], 4):      # four triangles an object: the z = 0 triangles share one centroid, which the
        sc.add_Triangles(triangles()[k:k + 4])         # reference's tree builder cannot split once an object has more than six
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    sc.set_view(*VIEW)
    orig = sc.debug_bvh()[3]
    packed_of = np.empty(orig.size, dtype=np.int64)
    packed_of[orig] = np.arange(orig.size)
    return sc, packed_of
