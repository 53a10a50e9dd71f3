"""Float64 numpy statement of the thin-lens ray of Scene.set_lens (include/pt_api.h pins it), which tests/path_ref.py's PathModel takes as
its camera ray after set_lens, and a float32 restatement of the pinned sequence that the tests measure their tolerance with.  It shares no code with the
library."""
import numpy as np

import nee_ref as R

TWO_PI = 6.283185307179586


def lcg_pair(S):
    """(rnd1, rnd2) float32 of the two LCG draws from non-negative states S (prog.cl:72-77)"""
    s = np.asarray(S, dtype=np.int64)
    assert (s >= 0).all()
    n1 = (s * 48271) % R.M31
    n2 = (n1 * 48271) % R.M31
    k = np.float32(2147483648.0)
    return n1.astype(np.float32) / k, n2.astype(np.float32) / k


def lens_units(S):
    """(u1, u2) float32: the hash values of segment -1, dimensions 0 and 1, of the complemented key"""
    key = (~np.asarray(S, dtype=np.int64)) & 0xFFFFFFFF
    scale = np.float32(2.0 ** -24)
    u1 = (R.nee_rand(key, -1, 0) >> np.uint32(8)).astype(np.float32) * scale
    u2 = (R.nee_rand(key, -1, 1) >> np.uint32(8)).astype(np.float32) * scale
    return u1, u2


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def lens_rays(cam, aperture, focus, gid, S, dtype=np.float64, rnd=None):
    """The lens rays of n samples: pixel gid (n,), LCG state S (n,) at the start of the sample (rnd: the two draws, default those of S).
    Every input is first rounded to float32 (the values the device gets) and then evaluated in `dtype`.  Returns P, D, Q (n, 3)."""
    t = dtype
    gid = np.asarray(gid, dtype=np.int64)
    rnd1, rnd2 = lcg_pair(S) if rnd is None else (np.asarray(rnd[0], dtype=np.float32), np.asarray(rnd[1], dtype=np.float32))
    u1, u2 = lens_units(S)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(t)
    eye, lookat, up, right = (f32(cam[k][:3]) for k in ("eye", "lookat", "up", "right"))
    X, Y = int(cam["XM"]), int(cam["YM"])
    x = (gid % X).astype(np.float32).astype(t) + rnd1.astype(t)
    y = (gid // X).astype(np.float32).astype(t) + rnd2.astype(t)
    sx = (t(2.0) * x) / t(X) - t(1.0)
    sy = (t(2.0) * y) / t(Y) - t(1.0)
    pp = (lookat + right * sx[:, None]) + up * sy[:, None]
    d = pp - eye
    f, Rh, Uh = _unit(lookat - eye), _unit(right), _unit(up)
    a, F = t(np.float32(aperture)), t(np.float32(focus))
    Q = d * (F / (d @ f))[:, None] + eye
    r = np.sqrt(u1.astype(t))
    theta = (TWO_PI * u2.astype(np.float64)).astype(np.float32).astype(np.float64)
    sn, cs = np.sin(theta).astype(t), np.cos(theta).astype(t)
    O = Uh * (a * (r * sn))[:, None] + (Rh * (a * (r * cs))[:, None] + eye)
    return O, _unit(Q - O), Q


def ray_errors(got, want_P, want_D):
    """per item, the errors of P and D as vectors, relative to the length of the wanted vector: (n, 2)"""
    got = np.asarray(got, dtype=np.float64)
    eP = np.linalg.norm(got[:, :3] - want_P, axis=1) / np.linalg.norm(want_P, axis=1)
    eD = np.linalg.norm(got[:, 3:6] - want_D, axis=1) / np.linalg.norm(want_D, axis=1)
    return np.stack([eP, eD], 1)


def distance_to_ray(Q, P, D):
    """the distance of the points Q from the lines P + t D"""
    D = D / np.linalg.norm(D, axis=1, keepdims=True)
    v = Q - P
    return np.linalg.norm(v - D * (v * D).sum(axis=1, keepdims=True), axis=1)


class LensMixin:
    """class LensModel(LensMixin, SomeModel): kept for the tests that name it.  The lens is a setting of tests/path_ref.py's PathModel:
    set_lens(aperture > 0, focus) turns every model's camera ray into lens_rays' of the seed sample() was called with."""
