"""Lit guide buffers (option aov_lights): what they change for the denoisers on a frame with a visible sphere light.  A record, no gate.

usage: python tools/aov_lights_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [frames=16] [tspp=4] [ref=1024] [rim=4] [out=FILE]

Scene: scenes.cornell_box(lamp="sphere"), rendered by render_nee (MIS) with option moments = 1.  With the option off and on:
  * denoise_variance on a frame of `spp` samples with guides from render_aovs(2, 4);
  * `frames` frames of `tspp` samples accumulated by temporal_accumulate under the panning camera of tools/temporal_bench.py (half a
    pixel of yaw per frame), guides from render_aovs(1, 4): the accumulated colour and denoise_temporal;
each as RMSE against a `ref`-spp frame of the same (final) camera with other seeds, over the whole frame and over the pixels within `rim`
pixels of the lamp's rim, seen directly and in the chromium sphere.  The rim comes from the lit guides' material (-2 where a chain ends
on the lamp); "in the mirror" are those of its pixels whose primary hit is the chromium sphere (guides of specular depth 0).  Also the time
of one guide pass (subpixels 1) off and on, HIP events, median of 20.  One JSON line on stdout."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from opencl_path_tracer_amd import api, scenes  # noqa: E402
import temporal_bench as TB  # noqa: E402


def make_scene(spec, W, H, bounces, option):
    sc = api.Scene(W, H).load(spec)
    sc.iterations = bounces
    sc.set_option("moments", 1)
    sc.set_option("aov_lights", option)
    return sc


def reference(spec, W, H, bounces, view, ref_spp):
    ref = make_scene(spec, W, H, bounces, 0)
    ref.set_view(*view)
    ref.upload_seeds(np.random.default_rng(12345).integers(1, 2 ** 31 - 1, W * H, dtype=np.int64).astype(np.int32))
    for _ in range(max(ref_spp // 64, 1)):
        ref.render_nee(min(ref_spp, 64), "mis")
    gt = ref.read_colors()[:, :3].astype(np.float64)
    ref.close()
    return gt


def near_boundary(mask, r):
    """the pixels within r of the boundary of a (H, W) mask: some pixel of the disc around them is inside and some is outside"""
    some, every = np.zeros_like(mask), np.ones_like(mask)
    H, W = mask.shape
    pad = np.pad(mask, r, mode="edge")
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > r * r:
                continue
            m = pad[r + dy:r + dy + H, r + dx:r + dx + W]
            some |= m
            every &= m
    return some & ~every


def regions(spec, W, H, view, rim):
    sc = make_scene(spec, W, H, 1, 1)
    sc.set_view(*view)
    sc.render_aovs(1, 4)
    lamp = (sc.read_aovs()[0][:, 3] <= -2).reshape(H, W)
    sc.set_option("aov_lights", 0)
    sc.render_aovs(1, 0)
    chrome = (sc.read_aovs()[0][:, 3] == scenes.CHROMIUM).reshape(H, W)
    sc.close()
    band = near_boundary(lamp, rim)
    return {"frame": np.ones(W * H, bool), "rim_direct": (band & ~chrome).reshape(-1), "rim_mirror": (band & chrome).reshape(-1)}


def rmse(a, gt, where):
    d = a[where, :3].astype(np.float64) - gt[where]
    return float(np.sqrt(np.mean(d * d))) if where.any() else None


def guide_ms(sc, reps=20):
    ts = []
    for i in range(reps + 3):
        sc.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sc.render_aovs(1, 4)
        sc.sync()
        e1.record()
        e1.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    W, H, bounces = int(kv.get("W", 1920)), int(kv.get("H", 1080)), int(kv.get("bounces", 8))
    spp, frames, tspp, ref_spp, rim = int(kv.get("spp", 16)), int(kv.get("frames", 16)), int(kv.get("tspp", 4)), int(kv.get("ref", 1024)), int(kv.get("rim", 4))
    spec = scenes.cornell_box(lamp="sphere")
    res = {"scene": "cornell_box(lamp='sphere')", "W": W, "H": H, "bounces": bounces, "spp": spp, "frames": frames, "tspp": tspp, "ref_spp": ref_spp, "rim": rim}
    still = (spec.fov, spec.yaw, spec.pitch, tuple(spec.shift))
    pan = TB.views(spec, W, frames, "pan")
    for name, view in (("still", still), ("pan", pan[-1])):
        gt = reference(spec, W, H, bounces, view, ref_spp)
        where = regions(spec, W, H, view, rim)
        res[name] = {"pixels": {k: int(v.sum()) for k, v in where.items()}}
        for option in (0, 1):
            sc = make_scene(spec, W, H, bounces, option)
            r = {}
            if name == "still":
                sc.set_view(*view)
                sc.render_nee(spp, "mis")
                sc.render_aovs(2, 4)
                out = {"raw": sc.read_colors(), "denoise_variance": sc.denoise_variance()}
                r["guide_pass_ms"] = guide_ms(sc)
            else:
                for v in pan:
                    sc.set_view(*v)
                    sc.current_sample = 0
                    sc.render_nee(tspp, "mis")
                    sc.render_aovs(1, 4)
                    sc.temporal_accumulate()
                rgbv, n = sc.read_temporal()
                out = {"raw": sc.read_colors(), "temporal": rgbv, "denoise_temporal": sc.denoise_temporal()}
                r["mean_n"] = {k: float(n[v].mean()) for k, v in where.items() if v.any()}
            r["aov_lights_stat"] = int(sc.stat("aov_lights"))
            r["rmse"] = {what: {k: rmse(a, gt, v) for k, v in where.items()} for what, a in out.items()}
            res[name]["on" if option else "off"] = r
            sc.close()
    print(json.dumps(res), flush=True)
    if "out" in kv:
        with open(kv["out"], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
