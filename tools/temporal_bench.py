"""Temporal accumulation with reprojection (Scene.temporal_accumulate, pt_temporal_accumulate): kernel time, quality, parameter sweep.

usage: python tools/temporal_bench.py [scene=cornell|mesh100k|both|cornell_st] [W=1920 H=1080] [bounces=8] [spp=4] [frames=16] [ref=1024]
                                      [reps=20] [sweep=0|1] [guides=geometric|shaded] [out=FILE]

Per scene, at W x H and `bounces` bounces, with option moments = 1 and guides from render_aovs(1, 4):
  * the time of one pt_temporal_accumulate (defaults, a history in place): HIP events around each synchronised call after a warm-up,
    median of `reps`, each on a fresh frame (an accumulate refuses a frame it has seen), next to the byte model;
  * the quality sequence: `frames` frames of `spp` samples while the camera pans half a pixel per frame (yaw), and again while it moves
    sideways by half a pixel's footprint at 1,300 units; RMSE of the last raw frame, of the accumulated colour, of pt_denoise_temporal
    and of pt_denoise_variance on the last frame, against a `ref`-spp frame of the final camera with other seeds;
  * sweep=1: the pan sequence over max_history x normal_cos x depth_tolerance.
scene=cornell_st is cornell_box(smooth=True, textured=True) under options smooth_normals and textures, rendered by render_nee (MIS);
guides=shaded renders every frame's guides with render_aovs(1, 4, shading="shaded").  "kept_history" is the share of pixels whose
accumulated sample count exceeds the frame's own, over the frame and over the pixels whose guide material is a sphere's.
One JSON line per scene on stdout."""
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

MAX_HISTORY = (8, 16, 32, 64, 128)
NORMAL_COS = (0.8, 0.9, 0.95)
DEPTH_TOL = (0.01, 0.02, 0.05)
# bytes per pixel: colour, albedo (material), normal + depth of the frame; one footprint's worth of the previous set (the 2x2 taps
# of neighbouring pixels overlap: each history pixel is read about once); the new set and the variance
READ_B, HIST_B, WRITE_B = 48, 40, 44


def scene_spec(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "cornell_st":
        return scenes.cornell_box(smooth=True, textured=True)
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell, cornell_st, mesh100k or both")


GUIDES = "geometric"          # guides=... on the command line


def make_scene(spec, W, H, bounces):
    """the scene; cornell_st shades with vertex normals and textures, which only the NEE path does (frame() renders accordingly)"""
    sc = api.Scene(W, H).load(spec)
    sc.iterations = bounces
    sc.nee = bool(spec.normals or spec.textures)
    if sc.nee:
        sc.set_option("smooth_normals", 1)
        sc.set_option("textures", 1)
    return sc


def render(sc, n):
    if sc.nee:
        sc.render_nee(n, "mis")
    else:
        sc.render(n)


def views(spec, W, steps, mode):
    fov, yaw, pitch, shift = spec.fov, spec.yaw, spec.pitch, tuple(spec.shift)
    out = [(fov, yaw, pitch, shift)]
    for _ in range(steps - 1):
        if mode == "pan":
            yaw += 0.5 * fov / W
        else:
            shift = api.camera_move(shift, yaw, pitch, 0.0, 0.5 * 2.0 * 1300.0 * np.tan(np.radians(fov / 2.0)) / W, 0.0)
        out.append((fov, yaw, pitch, shift))
    return out


def frame(sc, view, spp):
    sc.set_view(*view)
    sc.current_sample = 0
    render(sc, spp)
    sc.render_aovs(1, 4, shading=GUIDES)


def accumulate(sc, **kw):
    p = api.TemporalParams(**dict(api.temporal_defaults(), **kw))
    sc._ck(api.LIB.pt_temporal_accumulate(sc._h, C.byref(p)))


def rmse(a, gt):
    d = a[:, :3].astype(np.float64) - gt
    return float(np.sqrt(np.mean(d * d)))


def reference(spec, W, H, bounces, view, ref_spp):
    ref = make_scene(spec, W, H, bounces)
    ref.set_view(*view)
    ref.upload_seeds(np.random.default_rng(12345).integers(1, 2 ** 31 - 1, W * H, dtype=np.int64).astype(np.int32))
    for _ in range(ref_spp // 64):
        render(ref, 64)
    gt = ref.read_colors()[:, :3].astype(np.float64)
    ref.close()
    return gt


def sequence(spec, W, H, bounces, spp, vs, gt, filters=True, **kw):
    sc = make_scene(spec, W, H, bounces)
    sc.set_option("moments", 1)
    for v in vs:
        frame(sc, v, spp)
        accumulate(sc, **kw)
    rgbv, n = sc.read_temporal()
    r = {"temporal": rmse(rgbv, gt), "raw": rmse(sc.read_colors(), gt), "mean_n": float(n.mean()),
         "mean_temporal": float(rgbv[:, :3].astype(np.float64).mean()), "mean_ref": float(gt.mean())}
    mat = sc.read_aovs()[0][:, 3]
    spheres = (mat == scenes.CHROMIUM) | (mat == scenes.GLASS)
    r["kept_history"] = float(np.mean(n > spp))
    if spheres.any():
        r["kept_history_spheres"] = float(np.mean(n[spheres] > spp))
    if filters:
        r["denoise_temporal"] = rmse(sc.denoise_temporal(), gt)
        r["denoise_variance"] = rmse(sc.denoise_variance(), gt)
    sc.close()
    return r


def time_accumulate(spec, W, H, bounces, spp, reps):
    sc = make_scene(spec, W, H, bounces)
    sc.set_option("moments", 1)
    vs = views(spec, W, reps + 3, "pan")
    ts = []
    for i, v in enumerate(vs):
        frame(sc, v, spp)
        sc.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        accumulate(sc)
        e1.record()
        e1.synchronize()
        if i >= 3:                                       # warm-up: the allocation, the first launch, a first history
            ts.append(e0.elapsed_time(e1))
    sc.close()
    return float(np.median(ts))


def run(name, W, H, bounces, spp, frames, ref_spp, reps, sweep):
    spec = scene_spec(name)
    res = {"scene": name, "W": W, "H": H, "bounces": bounces, "spp": spp, "frames": frames, "ref_spp": ref_spp, "guides": GUIDES,
           "defaults": api.temporal_defaults()}
    ms = time_accumulate(spec, W, H, bounces, spp, reps)
    mb = W * H * (READ_B + HIST_B + WRITE_B) / 1e6
    res.update(accumulate_ms=ms, model_mb=mb, achieved_tb_s=mb / 1e6 / (ms / 1e3))
    for mode in ("pan", "sideways"):
        vs = views(spec, W, frames, mode)
        gt = reference(spec, W, H, bounces, vs[-1], ref_spp)
        res[mode] = sequence(spec, W, H, bounces, spp, vs, gt)
        if sweep and mode == "pan":
            res["sweep"] = []
            for mh in MAX_HISTORY:
                for nc in NORMAL_COS:
                    for dt in DEPTH_TOL:
                        r = sequence(spec, W, H, bounces, spp, vs, gt, filters=False, max_history=mh, normal_cos=nc, depth_tolerance=dt)
                        res["sweep"].append({"max_history": mh, "normal_cos": nc, "depth_tolerance": dt, "temporal_over_raw": r["temporal"] / r["raw"]})
            res["best"] = min(res["sweep"], key=lambda r: r["temporal_over_raw"])
    return res


def main():
    global GUIDES
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    GUIDES = kv.get("guides", "geometric")
    names = ("cornell", "mesh100k") if kv.get("scene", "both") == "both" else (kv["scene"],)
    out = []
    for name in names:
        r = run(name, int(kv.get("W", 1920)), int(kv.get("H", 1080)), int(kv.get("bounces", 8)), int(kv.get("spp", 4)),
                int(kv.get("frames", 16)), int(kv.get("ref", 1024)), int(kv.get("reps", 20)), int(kv.get("sweep", 1)))
        print(json.dumps(r), flush=True)
        out.append(r)
    if "out" in kv:
        with open(kv["out"], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
