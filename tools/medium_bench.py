"""The homogeneous medium (Scene.set_medium): launch time of render_nee on the Cornell box clear and in fog.

usage: python tools/medium_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [reps=5] [fog=0.001]

render_nee(spp, "mis"): wall clock around one launch and a sync, after one warm-up launch per context; `reps` launches each, the
contexts alternating -- clear: cornell_box() (k_nee); far: the same with a medium whose box the scene never enters (k_nee<kNeeMedium> doing
k_nee's work: what the medium instances cost by themselves); fog: cornell_box(fog=...), the room filled wall to wall (k_nee<kNeeMedium> with
scatter vertices).  For an A/B against another commit run it once per tree and alternate: PTAMD_TREE=<root of the other checkout,
built> selects the package the script imports.  A tree from before pt_set_medium runs the clear context only.  One JSON line on
stdout."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("PTAMD_TREE", "."))
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def main():
    kw = dict(W=1920, H=1080, bounces=8, spp=16, reps=5, fog=1e-3)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        kw[k] = type(kw[k])(v)
    names = ("clear", "far", "fog") if hasattr(api.Scene, "set_medium") else ("clear",)
    ctx = {}
    for name in names:
        sc = api.Scene(kw["W"], kw["H"]).load(scenes.cornell_box(fog=kw["fog"]) if name == "fog" else scenes.cornell_box())
        sc.iterations = kw["bounces"]
        if name == "far":
            sc.set_medium(kw["fog"], albedo=0.9, g=0.6, bounds=((-100.0, -3000.0, -100.0), (100.0, -2000.0, 100.0)))      # under the floor: no ray gets there
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
