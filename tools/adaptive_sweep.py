"""Adaptive frames (pt_render_adaptive) against uniform ones: samples spent, wall time, rounds and error against a high-spp frame.

usage: python tools/adaptive_sweep.py scene=cornell|mesh100k [W=1920 H=1080] [min=16] [max=1024] [ref=4096] [bounces=8]
                                      [thr=2,1.5,1,0.7,0.5,0.3,0.2,0.1,0] [uniform_steps=4]

The reference is a uniform render of `ref` samples on its own context.  For every threshold: samples spent, wall time of the
call (host clock around render_adaptive + sync, which includes the per-round synchronisation), the rounds with their active
tiles, and RMSE / rel-L2 of the colours against the reference; the same for uniform renders of max, max/2, max/4 and max/8 samples."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def scene_spec(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell or mesh100k")


def errors(cols, ref):
    d = cols[:, :3].astype(np.float64) - ref[:, :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d))), float(np.linalg.norm(d) / np.linalg.norm(ref[:, :3].astype(np.float64)))


def main():
    a = dict(kv.split("=", 1) for kv in sys.argv[1:])
    name = a.get("scene", "cornell")
    W, H = int(a.get("W", 1920)), int(a.get("H", 1080))
    lo, hi, ref_spp, bounces = int(a.get("min", 16)), int(a.get("max", 1024)), int(a.get("ref", 4096)), int(a.get("bounces", 8))
    thrs = [float(t) for t in a.get("thr", "2,1.5,1,0.7,0.5,0.3,0.2,0.1,0").split(",")]
    spec = scene_spec(name)

    def ctx():
        sc = api.Scene(W, H).load(spec)
        sc.iterations = bounces
        return sc

    sc = ctx()
    sc.render(2)                                     # warm-up: code objects, LDS attributes
    sc.sync()
    sc.close()
    sc = ctx()
    t0 = time.perf_counter()
    sc.render(ref_spp)
    sc.sync()
    ref = sc.read_colors()
    print("%s %dx%d, %d bounces; reference: uniform %d spp (%.2f s)" % (name, W, H, bounces, ref_spp, time.perf_counter() - t0))
    sc.close()
    rows = []
    for spp in [hi >> k for k in range(int(a.get("uniform_steps", 4))) if (hi >> k) >= lo]:     # the uniform curve, for equal-RMSE reads
        sc = ctx()
        t0 = time.perf_counter()
        sc.render(spp)
        sc.sync()
        dt = time.perf_counter() - t0
        rmse, rel = errors(sc.read_colors(), ref)
        rows.append(("uniform %d" % spp, W * H * spp, dt, rmse, rel, ""))
        sc.close()
    for thr in thrs:
        sc = ctx()
        t0 = time.perf_counter()
        res = sc.render_adaptive(lo, hi, thr)
        sc.sync()
        dt = time.perf_counter() - t0
        rmse, rel = errors(sc.read_colors(), ref)
        rounds = " ".join("%d:%d" % (b, n) for b, n in zip(res["rounds"], res["active_tiles"]))
        rows.append(("adaptive %d-%d thr %g" % (lo, hi, thr), res["samples"], dt, rmse, rel, rounds))
        sc.close()
    print("%-28s %14s %9s %9s %10s %10s  %s" % ("run", "samples", "x uniform", "wall ms", "RMSE", "rel-L2", "rounds (boundary:active tiles)"))
    for r in rows:
        print("%-28s %14d %9.3f %9.1f %10.5f %10.5f  %s" % (r[0], r[1], r[1] / float(rows[0][1]), 1e3 * r[2], r[3], r[4], r[5]))


if __name__ == "__main__":
    main()
