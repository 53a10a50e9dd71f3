"""Float64 statement of the medium's density grid (Scene.set_medium_density; include/pt_api.h pins the walk): walk(), the regular
tracking the grid instances of k_nee run in float32, step for step, and GridModel, tests/medium_ref.py's MediumModel with the free
flight and the transmittance taken from walk() (the setting `density` of tests/path_ref.py's PathModel).  tests/test_grid_host.py checks walk() against brute-force integration of the density along
random rays and GridModel against MediumModel on a 1 x 1 x 1 unit grid; tests/test_gpu_grid.py holds pt_debug_grid and the frames to them."""
import numpy as np

import medium_ref as M

SCATTER_MARGIN = 2e-5         # the scatter decision d < seg of a voxel is a near tie when |d - seg| is within this share of the
                              # larger (medium_ref.FLIGHT_MARGIN's reasoning: float32 log1pf, the divide, the clip, the planes)
PLANE_MARGIN = 1e-5           # ... and the voxel sequence when two tnext lie this close (a ray through an edge or a corner: float32
                              # may cross the planes in the other order) or a segment is this short, as a share of the walk's span


def grid_of(density, lo, hi):
    """(density (nz, ny, nx) float64, n = (nx, ny, nz), cell sizes) of a grid over the box"""
    rho = np.asarray(density, dtype=np.float64)
    n = np.array(rho.shape[::-1], dtype=np.int64)
    return rho, n, (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)) / n


def walk(sigma_t, density, lo, hi, P, D, t, tau):
    """Walk(P, D, t, tau) of include/pt_api.h in float64: dict(a, b, scatter, s, acc, visited, voxel, near, near_clip, margin, voxels).
    voxels: [(linear index, t_cur, t_exit)] in visiting order; margin: the smallest relative |d - seg| among the voxels with sigma > 0
    (inf without one); near_clip: medium_ref.clip's near tie (the interval itself is in doubt); near: that, or the sequence of voxels is a
    near tie (PLANE_MARGIN: the depth is not in doubt then, only which voxels of no length are visited)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    P, D = np.asarray(P, dtype=np.float64), np.asarray(D, dtype=np.float64)
    rho, n, cell = grid_of(density, lo, hi)
    a, b, near = M.clip(lo, hi, P, D, t)
    out = dict(a=a, b=b, scatter=False, s=-1.0, acc=0.0, visited=0, voxel=-1, near=bool(near), near_clip=bool(near), margin=np.inf, voxels=[])
    if not max(b - a, 0.0) > 0.0:
        return out
    idx, step, tnext, tdelta = [0, 0, 0], [0, 0, 0], [np.inf] * 3, [0.0] * 3
    for ax in range(3):
        g = np.floor((D[ax] * a + P[ax] - lo[ax]) / cell[ax])
        frac = (D[ax] * a + P[ax] - lo[ax]) / cell[ax]
        # the walk starts on an inner plane of this axis (or, with D = 0 there, lies in it): float32 may start in the voxel next door
        near |= bool(0 < np.round(frac) < n[ax] and abs(frac - np.round(frac)) * cell[ax] < PLANE_MARGIN * (abs(a) + abs(b) + abs(P[ax])))
        idx[ax] = int(min(max(g, 0.0), n[ax] - 1.0))
        if D[ax] != 0.0 and np.isfinite(1.0 / D[ax]):
            up = D[ax] > 0.0
            kb = idx[ax] + (1 if up else 0)
            plane = hi[ax] if kb == n[ax] else lo[ax] + kb * cell[ax]
            step[ax] = 1 if up else -1
            tnext[ax] = (plane - P[ax]) / D[ax]
            tdelta[ax] = cell[ax] / abs(D[ax])
    span = abs(a) + abs(b)
    tc, acc = a, 0.0
    for _ in range(int(n.sum()) + 3):
        lin = (idx[2] * n[1] + idx[1]) * n[0] + idx[0]
        sigma = sigma_t * rho[idx[2], idx[1], idx[0]]
        out["visited"] += 1
        te = min(tnext[0], tnext[1], tnext[2], b)
        seg = max(te - tc, 0.0)
        out["voxels"].append((int(lin), tc, te))
        near |= te - tc < PLANE_MARGIN * span and te < b            # a plane right at the start of the voxel: float32 may start beyond it
        finite = sorted(v for v in tnext if np.isfinite(v))
        for u, v in zip(finite[:-1], finite[1:]):                   # two planes crossed (almost) together, before the walk's end
            near |= abs(u - v) < PLANE_MARGIN * span and u <= te + PLANE_MARGIN * span and u < b
        if sigma > 0.0:
            d = (tau - acc) / sigma
            if np.isfinite(d):
                out["margin"] = min(out["margin"], abs(d - seg) / max(d, seg, 1e-300))
            if d < seg:
                out.update(scatter=True, s=tc + d, voxel=int(lin), d=d, t_cur=tc)
                break
        acc += sigma * seg
        if te >= b:
            break
        ax = 0 if tnext[0] <= tnext[1] and tnext[0] <= tnext[2] else (1 if tnext[1] <= tnext[2] else 2)
        idx[ax] += step[ax]
        tnext[ax] += tdelta[ax]
        if not 0 <= idx[ax] < n[ax]:
            break
        tc = te
    out["acc"] = acc
    out["near"] = bool(near)
    return out


def brute_depth(sigma_t, density, lo, hi, P, D, t0, t1, steps=200000):
    """the optical depth of [t0, t1] by the midpoint rule: the density looked up at each sample point on its own, no walk"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    rho, n, cell = grid_of(density, lo, hi)
    ts = t0 + (np.arange(steps) + 0.5) * ((t1 - t0) / steps)
    x = np.asarray(P, dtype=np.float64)[None, :] + np.asarray(D, dtype=np.float64)[None, :] * ts[:, None]
    g = np.floor((x - lo[None, :]) / cell[None, :]).astype(np.int64)
    inside = ((g >= 0) & (g < n[None, :])).all(axis=1)
    g = np.clip(g, 0, n[None, :] - 1)
    return float((sigma_t * rho[g[:, 2], g[:, 1], g[:, 0]] * inside).sum() * ((t1 - t0) / steps))


EVENTS = M.EVENTS + ("grid_scatter_thin", "grid_scatter_dense", "grid_empty_crossed", "grid_light_partial")


class GridModel(M.MediumModel):
    """medium_ref.MediumModel with a density grid: density = Scene.medium_density() (None: the model is MediumModel's).  The free flight
    and the transmittance of a light sample come from walk() in place of flight() and transmittance() (clip stays, and leaves the
    segment with the flight), and the walk's near ties (SCATTER_MARGIN, PLANE_MARGIN) are added to the sample's.  dense_from: a scatter
    vertex counts as "dense" in a voxel of at least this density, else "thin"."""

    EVENTS = EVENTS

    def __init__(self, *args, density=None, dense_from=2.0, **settings):
        settings.setdefault("events", M.S.BASE_EVENTS + EVENTS)
        super().__init__(*args, density=density, dense_from=dense_from, **settings)
