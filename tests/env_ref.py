"""Float64 numpy model of Scene.render_nee under an environment map (include/pt_api.h pins the estimator), built on
tests/nee_ref.py's Model: the same LCG stream, the same hashes, brute-force intersection; the sampling tables come from
Scene.debug_environment() as nee_ref takes the light table.  Also the numpy statements of the direction -> texel mapping and of
the tables themselves (tests/test_env_host.py)."""
import numpy as np

import nee_ref as R
from path_ref import PathModel

EDGE_MARGIN = 1e-4          # radians: a miss direction this close to a texel edge may read the neighbour in float32
SELECT_MARGIN = 2.0 ** -20


def yaw_radians(yaw_degrees):
    return float(np.float32(float(np.float32(yaw_degrees)) * np.pi / 180.0))


def lookup(w, h, yaw_degrees, d):
    """(row, col, angular distance to the nearest texel edge) of unit direction d, in float64."""
    d = np.asarray(d, dtype=np.float64)
    theta = float(np.arccos(np.clip(d[1], -1.0, 1.0)))
    phi = float(np.arctan2(d[2], d[0])) - yaw_radians(yaw_degrees)
    fr = theta / np.pi * h
    row = min(h - 1, int(np.floor(fr)))
    turn = phi / (2.0 * np.pi)
    fc = (turn - np.floor(turn)) * w
    col = min(w - 1, int(np.floor(fc)))
    dist = np.inf
    k = np.rint(fr)
    if 0 < k < h:                                   # the poles are no edges
        dist = abs(fr - k) * np.pi / h
    if w > 1:
        dist = min(dist, abs(fc - np.rint(fc)) * (2.0 * np.pi / w) * np.sin(theta))
    return row, col, float(dist)


def luminance(rgb):
    rgb = np.asarray(rgb, dtype=np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def solid_angles(w, h):
    th = np.arange(h + 1) * np.pi / h
    return (2.0 * np.pi / w) * (np.cos(th[:-1]) - np.cos(th[1:]))


def tables(rgb):
    """The double-precision build of the distribution: (row_cdf (h,), col_cdf (h, w), has_distribution); rows of weight 0 get a
    uniform column cdf, a map without a distribution uniform tables."""
    rgb = np.asarray(rgb, dtype=np.float64)
    h, w = rgb.shape[:2]
    lum = luminance(rgb)
    rs = lum.sum(axis=1)
    col = np.where(rs[:, None] > 0, np.cumsum(lum, axis=1) / np.where(rs > 0, rs, 1.0)[:, None], (np.arange(w) + 1.0)[None, :] / w)
    col[:, -1] = 1.0
    roww = rs * solid_angles(w, h) * w / (2.0 * np.pi)
    has = bool(roww.sum() > 0)
    row = np.cumsum(roww) / roww.sum() if has else (np.arange(h) + 1.0) / h
    row[-1] = 1.0
    return row, col, has


def texel_pdf(row_cdf, col_cdf):
    """p_env per texel from the stored float cdfs' own steps."""
    row_cdf = np.asarray(row_cdf, dtype=np.float64)
    col_cdf = np.asarray(col_cdf, dtype=np.float64)
    h, w = col_cdf.shape
    pr = np.diff(np.concatenate([[0.0], row_cdf]))
    pc = np.diff(np.concatenate([np.zeros((h, 1)), col_cdf], axis=1), axis=1)
    return pr[:, None] * pc / solid_angles(w, h)[:, None]


class EnvModel(PathModel):
    """nee_ref.Model plus an environment: rgb (h, w, 3), scale, yaw_degrees, and Scene.debug_environment()'s tables (no triangles at all:
    only the camera and the sky)."""

    def __init__(self, verts, normals, mats, mat_of, cam, rgb, env_tables, scale=1.0, yaw_degrees=0.0, table=None, margin=1e-4):
        super().__init__(verts, normals, mats, mat_of, cam, table=table, margin=margin, side_margins=False,
                         env=dict(rgb=rgb, tables=env_tables, scale=scale, yaw_degrees=yaw_degrees))
