"""CPU replay of an adaptive frame (pt_render_adaptive): the float32 noise estimate and the tile decisions, in numpy.

The estimate is bit-defined (include/pt_api.h): e = ((|M.r-A.r| + |M.g-A.g|) + |M.b-A.b|) / (1e-4 + sqrt((M.r + M.g) + M.b)) in
float32, IEEE sqrt and divide; a tile's error is the max over its pixels inside the frame, +inf if any e is not finite."""
import numpy as np


def rounds(min_spp, max_spp):
    b = [min_spp // 2, min_spp]
    while b[-1] != max_spp:
        b.append(min(2 * b[-1], max_spp))
    return b


def pixel_estimate(M, A):
    """M, A: (..., >= 3) float32 colours -> (...) float32 estimates (non-finite ones as +inf)."""
    M = np.asarray(M, dtype=np.float32)
    A = np.asarray(A, dtype=np.float32)
    d = (np.abs(M[..., 0] - A[..., 0]) + np.abs(M[..., 1] - A[..., 1])) + np.abs(M[..., 2] - A[..., 2])
    s = (M[..., 0] + M[..., 1]) + M[..., 2]
    with np.errstate(all="ignore"):
        e = d / (np.float32(1e-4) + np.sqrt(s))
    e = np.asarray(e, dtype=np.float32)
    return np.where(np.isfinite(e), e, np.float32(np.inf)).astype(np.float32)


def tile_errors(M, A, width, height):
    """Per 8x8 tile of a width x height frame (raster order): the max estimate over the tile's pixels inside the frame."""
    e = pixel_estimate(np.asarray(M).reshape(height, width, -1), np.asarray(A).reshape(height, width, -1))
    tx, ty = (width + 7) // 8, (height + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), dtype=np.float32)      # (estimates are >= 0: padding never wins the max)
    pad[:height, :width] = e
    return pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).reshape(-1)


def tile_of_pixel(width, height):
    y, x = np.mgrid[0:height, 0:width]
    return ((y // 8) * ((width + 7) // 8) + x // 8).reshape(-1)


def replay(snapshots, width, height, min_spp, max_spp, threshold):
    """snapshots[b] = (colors (npix, 4) float32, rnds (npix,)) of a uniform render at every boundary b.  Returns what the adaptive
    frame must leave: per-tile counts, per-tile last errors (+inf: none), per-pixel colours and rnds, and the boundaries per round
    with their active tile counts."""
    bounds = rounds(min_spp, max_spp)
    n_tiles = ((width + 7) // 8) * ((height + 7) // 8)
    spp = np.zeros(n_tiles, dtype=np.int32)
    err = np.full(n_tiles, np.inf, dtype=np.float32)
    active = np.ones(n_tiles, dtype=bool)
    ran, act = [], []
    thr = np.float32(threshold)
    for k, b in enumerate(bounds):
        if not active.any():
            break
        ran.append(b)
        act.append(int(active.sum()))
        spp[active] = b
        if k >= 1 and b < max_spp:
            e = tile_errors(snapshots[b][0], snapshots[bounds[k - 1]][0], width, height)
            err[active] = e[active]
            active = active & ~(e < thr)
    tp = tile_of_pixel(width, height)
    cols = np.empty_like(snapshots[bounds[0]][0])
    rnds = np.empty_like(snapshots[bounds[0]][1])
    for b in set(spp.tolist()):
        sel = spp[tp] == b
        cols[sel] = snapshots[b][0][sel]
        rnds[sel] = snapshots[b][1][sel]
    return {"spp": spp, "err": err, "colors": cols, "rnds": rnds, "rounds": ran, "active_tiles": act, "pixel_spp": spp[tp]}
