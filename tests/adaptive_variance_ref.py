"""CPU replay of an adaptive frame of pt_render_adaptive_ex: the variance metric's float32 tile estimate and the tile decisions, in numpy.

include/pt_api.h pins the estimate.  At boundary b, per pixel inside the frame: mu = l(colors.xyz), v = fmaxf(fmaf(-mu, mu, colors.w), 0) /
(float)(b - 1); tonemapped: d = 1 + mu, v = v / ((d*d)*(d*d)); lane (y&7)*8 + (x&7) of the tile's 64 holds v (0 outside the frame); the
sum is the xor butterfly s = s + s[lane ^ off] for off = 32 .. 1; e = sqrtf(s / (float)pixels inside), +inf if that is not finite."""
import numpy as np

import adaptive_ref as R
from adaptive_ref import rounds, tile_of_pixel
from variance_ref import fmaf, luminance, variance  # noqa: F401  (fmaf: the rounding luminance and variance are built on)

HALF, VARIANCE = 0, 1
_LANES = np.arange(64)


def butterfly_sum(lanes):
    """(..., 64) float32 -> (..., 64) float32: what every lane holds after s = s + shfl_xor(s, off) for off = 32, 16, 8, 4, 2, 1."""
    s = np.asarray(lanes, dtype=np.float32).copy()
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _LANES ^ off]
    return s


def pixel_variance(colors, b, tonemapped):
    """(npix, 4) float32 colours with the second moment in .w -> (npix,) float32: the per-pixel term of the estimate at boundary b."""
    colors = np.asarray(colors, np.float32)
    v = variance(colors, b)
    if tonemapped:
        d = np.float32(1.0) + luminance(colors)
        with np.errstate(all="ignore"):
            v = v / ((d * d) * (d * d))
    return np.asarray(v, np.float32)


def tile_lanes(values, width, height):
    """(npix,) per-pixel values -> (n_tiles, 64) float32, lane (y&7)*8 + (x&7) of the pixel's tile, 0 outside the frame."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), dtype=np.float32)
    pad[:height, :width] = np.asarray(values, np.float32).reshape(height, width)
    return pad.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)


def pixels_inside(width, height):
    tx, ty = (width + 7) // 8, (height + 7) // 8
    nx = np.minimum(width - 8 * np.arange(tx), 8)
    ny = np.minimum(height - 8 * np.arange(ty), 8)
    return (ny[:, None] * nx[None, :]).reshape(-1)


def tile_errors(colors, b, width, height, tonemapped):
    """Per 8x8 tile (raster order): the root mean square of the pixels' variance of the mean luminance at b samples."""
    s = butterfly_sum(tile_lanes(pixel_variance(colors, b, tonemapped), width, height))
    with np.errstate(all="ignore"):
        e = np.sqrt(s[:, 0] / pixels_inside(width, height).astype(np.float32))
    e = np.asarray(e, np.float32)
    return np.where(np.isfinite(e), e, np.float32(np.inf)).astype(np.float32)


def replay(snapshots, width, height, min_spp, max_spp, threshold, metric=VARIANCE, tonemapped=0):
    """snapshots[b] = (colors (npix, 4) float32 with the moment in .w, rnds (npix,), further per-pixel arrays ...) of a uniform render
    at every boundary b.  Returns what the adaptive frame must leave, like adaptive_ref.replay, and under "extra" the further arrays
    picked per pixel at the boundary its tile stopped at."""
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
            if metric == HALF:
                e = R.tile_errors(snapshots[b][0], snapshots[bounds[k - 1]][0], width, height)
            else:
                e = tile_errors(snapshots[b][0], b, width, height, tonemapped)
            err[active] = e[active]
            active = active & ~(e < thr)
    tp = tile_of_pixel(width, height)
    first = snapshots[bounds[0]]
    out = [np.empty_like(a) for a in first]
    for b in set(spp.tolist()):
        sel = spp[tp] == b
        for o, a in zip(out, snapshots[b]):
            o[sel] = a[sel]
    return {"spp": spp, "err": err, "colors": out[0], "rnds": out[1], "extra": out[2:], "rounds": ran, "active_tiles": act,
            "pixel_spp": spp[tp]}
