"""The variance-guided filter (Scene.denoise_variance, pt_denoise_variance): RMSE sweep at 16 spp and its cost.

usage: python tools/denoise_variance_bench.py [scene=cornell|mesh100k|both|cornell_st] [W=1920 H=1080] [bounces=8] [spp=16] [ref=4096]
                                              [reps=10] [guides=geometric|shaded] [out=FILE]

Per scene, at W x H and `bounces` bounces, against a uniform `ref`-spp frame: one `spp`-spp frame rendered with option moments = 1
and guides from render_aovs(2, 4); RMSE of the raw frame, of pt_denoise with its defaults, and of pt_denoise_variance over
demodulate x iterations x sigma_luminance (normal and depth at their defaults); then the wall time of the filter with its
defaults (synchronised, median of `reps`) and of the render with moments 0 / 1.  One JSON line per scene on stdout.
scene=cornell_st is cornell_box(smooth=True, textured=True) under options smooth_normals and textures, rendered by render_nee (MIS), the
path those options run on; guides=shaded renders the guides with render_aovs(2, 4, shading="shaded") (any scene)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

ITERATIONS = (2, 3, 4, 5, 6)
SIGMA_L = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)


def scene_spec(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "cornell_st":
        return scenes.cornell_box(smooth=True, textured=True)
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell, cornell_st, mesh100k or both")


def make_scene(name, spec, W, H, bounces):
    """the scene and its render call: cornell_st shades with vertex normals and textures, which only the NEE path does"""
    sc = api.Scene(W, H).load(spec)
    sc.iterations = bounces
    if name != "cornell_st":
        return sc, sc.render
    sc.set_option("smooth_normals", 1)
    sc.set_option("textures", 1)
    return sc, lambda n: sc.render_nee(n, "mis")


def rmse(a, b):
    d = a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def median_ms(fn, sync, reps):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def run(name, W, H, bounces, spp, ref_spp, reps, shading="geometric"):
    spec = scene_spec(name)
    ref, render = make_scene(name, spec, W, H, bounces)
    for _ in range(ref_spp // 64):
        render(64)
    gt = ref.read_colors()
    ref.close()
    sc, render = make_scene(name, spec, W, H, bounces)
    sc.set_option("moments", 1)
    render(spp)
    raw = sc.read_colors()
    sc.render_aovs(2, 4, shading=shading)
    res = {"scene": name, "W": W, "H": H, "bounces": bounces, "spp": spp, "ref_spp": ref_spp, "guides": shading,
           "rmse_raw": rmse(raw, gt), "rmse_denoise_defaults": rmse(sc.denoise(), gt), "sweep": []}
    for dm in (0, 1):
        for L in ITERATIONS:
            for sl in SIGMA_L:
                res["sweep"].append({"demodulate": dm, "iterations": L, "sigma_luminance": sl,
                                     "rmse": rmse(sc.denoise_variance(demodulate=dm, iterations=L, sigma_luminance=sl), gt)})
    best = min(res["sweep"], key=lambda r: r["rmse"])
    res["best"] = best
    d = sc.denoise_variance()
    res["rmse_defaults"] = rmse(d, gt)
    res["mean_ref"], res["mean_defaults"] = float(gt[:, :3].astype(np.float64).mean()), float(d[:, :3].astype(np.float64).mean())
    res["filter_ms_defaults"] = median_ms(lambda: sc.denoise_variance(), sc.sync, reps)
    res["denoise_ms_defaults"] = median_ms(lambda: sc.denoise(), sc.sync, reps)
    for m in (0, 1):
        sc.set_option("moments", m)

        def frame():
            sc.current_sample = 0
            render(spp)
        res["render_ms_moments%d" % m] = median_ms(frame, sc.sync, max(3, reps // 3))
    sc.close()
    return res


def main():
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    names = ("cornell", "mesh100k") if kv.get("scene", "both") == "both" else (kv["scene"],)
    out = []
    for name in names:
        r = run(name, int(kv.get("W", 1920)), int(kv.get("H", 1080)), int(kv.get("bounces", 8)), int(kv.get("spp", 16)),
                int(kv.get("ref", 4096)), int(kv.get("reps", 10)), kv.get("guides", "geometric"))
        print(json.dumps(r), flush=True)
        out.append(r)
    if "out" in kv:
        with open(kv["out"], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
