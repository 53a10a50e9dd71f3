"""Analytic lights (Scene.set_lights): launch time of render_nee on the Cornell box lit by its lamp quad, by a point light of the same
power in its place, and by the quad plus one extra point light.

usage: python tools/lights_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [reps=5]

render_nee(spp, "mis"): wall clock around one launch and a sync, after one warm-up launch per context; `reps` launches each, the
contexts alternating -- quad: cornell_box() (k_nee); point: cornell_box(lamp="point"), no emitter, P_ana = 1 (k_nee<kNeeLights>); quad_plus:
cornell_box() with one more point light, P_ana = 0.5 (k_nee<kNeeLights>).  For an A/B against another commit run it once per tree and
alternate: PTAMD_TREE=<root of the other checkout, built> selects the package the script imports (the default is this tree; the symbols
differ between commits, so PTAMD_LIB alone is not enough).  A tree from before pt_set_lights runs the quad context only.  One JSON
line on stdout."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("PTAMD_TREE", "."))
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def main():
    kw = dict(W=1920, H=1080, bounces=8, spp=16, reps=5)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        kw[k] = type(kw[k])(v)
    names = ("quad", "point", "quad_plus") if hasattr(api.Scene, "set_lights") else ("quad",)
    ctx = {}
    for name in names:
        sc = api.Scene(kw["W"], kw["H"]).load(scenes.cornell_box(lamp="point") if name == "point" else scenes.cornell_box())
        sc.iterations = kw["bounces"]
        if name == "quad_plus":
            sc.set_lights([api.point_light((200.0, 800.0, 100.0), (4e6, 3e6, 2e6))])
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
    for name in ctx:
        out[name + "_ms"] = ms[name]
        out[name + "_median_ms"] = sorted(ms[name])[len(ms[name]) // 2]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
