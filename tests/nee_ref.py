"""Float64 numpy model of Scene.render_nee (include/pt_api.h pins the estimator): the same LCG stream, the same light-sample
hash, brute-force intersection; the path loop itself is tests/path_ref.py's PathModel, of which Model is the plainest configuration.  For scenes of a few dozen triangles (tests/test_gpu_nee.py); also the host replay of
pt_nee_rand and of the light table."""
import numpy as np

from path_ref import PathModel

M31 = 2147483647
SHADOW_CUT = 1.0001


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def nee_rand(state, segment, dim):
    """pt_nee_rand, vectorised: lowbias32(lowbias32(state) + 0x9e3779b9 * (3 segment + dim + 1)) in uint32."""
    state = np.asarray(state).astype(np.int64).astype(np.uint32)
    c = (np.asarray(segment, dtype=np.int64) * 3 + np.asarray(dim, dtype=np.int64) + 1).astype(np.uint32)
    with np.errstate(over="ignore"):
        return lowbias32(lowbias32(state) + np.uint32(0x9E3779B9) * c)


def nee_unit(h):
    return float(np.float32(int(h) >> 8) * np.float32(2.0 ** -24))


def lcg(seed):
    """prog.cl:72-77 on one int state: (new state, float32 value as a Python float)"""
    n = (int(seed) * 48271) % M31 if seed >= 0 else ((int(seed) % (1 << 64)) * 48271) % M31
    return n, float(np.float32(n) / np.float32(2147483648.0))


def light_table(verts, mats, mat_of):
    """(tri indices, P_sel) of the lights in add order: type 3, emission sum > 0, area > 0; P_sel ~ area x emission sum."""
    idx, w = [], []
    for i, v in enumerate(np.asarray(verts, dtype=np.float64)):
        m = mats[int(mat_of[i])]
        es = float(m["emission"][0]) + float(m["emission"][1]) + float(m["emission"][2])
        area = 0.5 * np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0]))
        if int(m["type"]) == 3 and es > 0 and area > 0:
            idx.append(i)
            w.append(area * es)
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(idx, dtype=np.int64), (w / w.sum() if len(w) else w)


def selection_probs(cdf):
    """The probability that u0 = m 2^-24 (m < 2^24) picks light j -- the first j with cdf[j] > u0 -- as P_sel of pt_api.h"""
    up = np.ceil(np.asarray(cdf, dtype=np.float64) * 2.0 ** 24)
    return np.diff(np.concatenate([[0.0], up])) / 2.0 ** 24


class Model(PathModel):
    """PathModel with nothing but the light table: verts (n,3,3), normals (n,3) (the Triangle records' N), mats (MATERIAL records),
    mat_of (n,), camera (CAMERA record), flat triangles (side_margins off: tests/path_ref.py)."""

    def __init__(self, verts, normals, mats, mat_of, cam, table=None, margin=1e-4):
        super().__init__(verts, normals, mats, mat_of, cam, table=table, margin=margin, side_margins=False)
