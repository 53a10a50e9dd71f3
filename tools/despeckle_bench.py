"""The variance-gated firefly filter (Scene.despeckle, pt_despeckle): its cost next to the variance-guided filter, and the RMSE sweep.

usage: python tools/despeckle_bench.py [scene=cornell|mesh100k|both] [W=1920 H=1080] [bounces=8] [spp=16] [ref=4096] [reps=20]
                                       [sweep=1] [out=FILE]

Per scene, at W x H and `bounces` bounces, against a uniform `ref`-spp frame: one `spp`-spp frame rendered with option moments = 1
and guides from render_aovs(2, 4).
  time   pt_despeckle per radius and spread (source FRAME, so the k_variance launch of the read-out is inside), one k_atrous_var
         iteration (pt_denoise_variance, iterations 1: the same k_variance launch inside) and pt_denoise_variance / pt_denoise_despeckled
         with their defaults: HIP events around the call on the context's stream, median of `reps` after a warm-up; with the byte model
         of the stage (16 B colour + 4 B variance read, 24 B written per pixel; the halo is served by L2)
  sweep  threshold x rank x radius x min_rel_sigma, spread on and off: RMSE and mean shift (relative to the raw frame's mean) of the
         despeckled frame and of denoise_despeckled with the filter's defaults
One JSON line per scene on stdout."""
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

THRESHOLD = (1.5, 2.0, 3.0, 4.0, 8.0)
RANK = (1, 2, 3)
RADIUS = (1, 2, 3)
MIN_REL_SIGMA = (0.0, 0.25, 0.5, 1.0)


def scene_spec(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell, mesh100k or both")


def rmse(a, b):
    d = a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def mean(a):
    return float(a[:, :3].astype(np.float64).mean())


def event_ms(sc, call, reps):
    """median over reps of the device time of call() (a C entry point that only enqueues), after three warm-up calls"""
    ts = []
    for i in range(reps + 3):
        sc.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call()
        e1.record()
        e1.synchronize()
        if rc != api.PT_OK:
            raise SystemExit("call failed: %d %s" % (rc, api.LIB.pt_last_error(sc._h)))
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def run(name, W, H, bounces, spp, ref_spp, reps, sweep):
    spec = scene_spec(name)
    ref = api.Scene(W, H).load(spec)
    ref.iterations = bounces
    for _ in range(ref_spp // 64):
        ref.render(64)
    gt = ref.read_colors()
    ref.close()
    sc = api.Scene(W, H).load(spec)
    sc.iterations = bounces
    sc.set_option("moments", 1)
    sc.render(spp)
    raw = sc.read_colors()
    sc.render_aovs(2, 4)
    res = {"scene": name, "W": W, "H": H, "bounces": bounces, "spp": spp, "ref_spp": ref_spp, "defaults": api.despeckle_defaults(),
           "rmse_raw": rmse(raw, gt), "mean_ref": mean(gt), "mean_raw": mean(raw), "time_ms": {}}
    # ---- time
    for radius in RADIUS:
        for spread in (0, 1):
            p = api.DespeckleParams(**dict(api.despeckle_defaults(), radius=radius, spread=spread))
            res["time_ms"]["despeckle_r%d_spread%d" % (radius, spread)] = event_ms(sc, lambda: api.LIB.pt_despeckle(sc._h, C.byref(p)), reps)
    one = api.DenoiseVarianceParams(**dict(api.denoise_variance_defaults(), iterations=1))
    dflt = api.DenoiseVarianceParams(**api.denoise_variance_defaults())
    res["time_ms"]["atrous_var_one_iteration"] = event_ms(sc, lambda: api.LIB.pt_denoise_variance(sc._h, C.byref(one)), reps)
    res["time_ms"]["denoise_variance_defaults"] = event_ms(sc, lambda: api.LIB.pt_denoise_variance(sc._h, C.byref(dflt)), reps)
    sc.despeckle()
    res["time_ms"]["denoise_despeckled_defaults"] = event_ms(sc, lambda: api.LIB.pt_denoise_despeckled(sc._h, C.byref(dflt)), reps)
    res["model_mb"] = W * H * (16 + 4 + 24) / 1e6
    # ---- quality
    dv = sc.denoise_variance()
    res["denoise_variance"] = {"rmse": rmse(dv, gt), "mean_shift": mean(dv) / mean(raw) - 1.0}

    def point(**kw):
        rgbv, flags = sc.despeckle(**kw)
        dd = sc.denoise_despeckled()
        return dict(kw, flagged=int((flags == 1).sum()), rmse=rmse(rgbv, gt), mean_shift=mean(rgbv) / mean(raw) - 1.0,
                    rmse_filtered=rmse(dd, gt), mean_shift_filtered=mean(dd) / mean(raw) - 1.0)
    res["at_defaults"] = point()
    if sweep:
        res["sweep"] = [point(threshold=t, rank=k, radius=r, min_rel_sigma=g, spread=s)
                        for s in (1, 0) for r in RADIUS for k in RANK for t in THRESHOLD for g in MIN_REL_SIGMA]
        res["best_filtered"] = min(res["sweep"], key=lambda q: q["rmse_filtered"])
        res["best_alone"] = min(res["sweep"], key=lambda q: q["rmse"])
    sc.close()
    return res


def main():
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    names = ("cornell", "mesh100k") if kv.get("scene", "both") == "both" else (kv["scene"],)
    out = []
    for name in names:
        r = run(name, int(kv.get("W", 1920)), int(kv.get("H", 1080)), int(kv.get("bounces", 8)), int(kv.get("spp", 16)),
                int(kv.get("ref", 4096)), int(kv.get("reps", 20)), int(kv.get("sweep", 1)))
        print(json.dumps(r), flush=True)
        out.append(r)
    if "out" in kv:
        with open(kv["out"], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
