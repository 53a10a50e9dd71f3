"""The medium's density grid (Scene.set_medium_density): launch time of render_nee on the fogged Cornell box, homogeneous and through a grid.

usage: python tools/grid_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [reps=7] [fog=0.001] [n=64]

render_nee(spp, "mis"): wall clock around one launch and a sync, after one warm-up launch per context; `reps` launches each, the
contexts alternating -- fog: cornell_box(fog=...) (k_nee<kNeeMedium>); unit: the same with a 1 x 1 x 1 grid of 1 (k_nee<kNeeGrid> computing the
same frame: what the walk's set-up costs by itself); plume: the same with smoke_plume(n) (k_nee<kNeeGrid> walking n^3 voxels; the frame
differs: the plume is mostly empty room with a dense column).  One JSON line on stdout."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def main():
    kw = dict(W=1920, H=1080, bounces=8, spp=16, reps=7, fog=1e-3, n=64)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        kw[k] = type(kw[k])(v)
    ctx = {}
    for name in ("fog", "unit", "plume"):
        sc = api.Scene(kw["W"], kw["H"]).load(scenes.cornell_box(fog=kw["fog"]))
        sc.iterations = kw["bounces"]
        if name == "unit":
            sc.set_medium_density(np.ones((1, 1, 1), dtype=np.float32))
        if name == "plume":
            sc.set_medium_density(scenes.smoke_plume(kw["n"]))
        sc.render_nee(kw["spp"], "mis")
        sc.sync()
        ctx[name] = sc
    ms = {name: [] for name in ctx}
    for _ in range(kw["reps"]):
        for name, sc in ctx.items():
            sc.current_sample = 0
            sc.seed_default()
            sc.sync()
            t0 = time.perf_counter()
            sc.render_nee(kw["spp"], "mis")
            sc.sync()
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 2))
    out = dict(kw)
    for name, sc in ctx.items():
        out[name + "_ms"] = ms[name]
        out[name + "_median_ms"] = sorted(ms[name])[len(ms[name]) // 2]
        out[name + "_family"] = int(sc.stat("nee_family"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
