"""Guide buffers (render_aovs) and the a-trous denoiser (denoise): kernel times, bytes moved, and what the filter buys in RMSE.

usage: python tools/denoise_bench.py [scene=cornell|mesh100k|both] [W=1920 H=1080] [bounces=8] [ref=4096] [reps=20] [sweep=1]
                                     [out=DIR]

One JSON line per scene on stdout; with out=DIR also DIR/<scene>_<W>x<H>.json.

Per scene, at W x H and `bounces` bounces, against a uniform `ref`-spp frame of the same GPU:
  * AOV pass (specular_depth 4) at subpixels 1 and 2, and pt_denoise at L = 1 and the defaults' L: HIP events around the call on
    the library's stream, after a warm-up, median of `reps`; bytes from the byte model below and the rate against the 6.29 TB/s
    float4 copy measured on MI355X;
  * RMSE of raw and denoised frames (defaults, render_aovs(2, 4)) at 4 / 16 / 64 / 256 spp;
  * the uniform spp a denoised 16-spp frame matches in RMSE (log-log interpolation of the raw curve), and the wall time of both;
  * with sweep=1, RMSE at 16 spp over a small grid of sigma_color, sigma_normal, sigma_depth and iterations (one axis at a time
    around the defaults, then the best of each axis together).
Byte model (compulsory traffic; the 25 taps of a pixel are served by the caches): AOV pass 32 B/px written; one filter iteration
16 B colour in + 16 B guide in + 16 B out, + 16 B albedo in the first (demodulation) and in the last (remodulation)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

COPY_TBS = 6.29


def scene_spec(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell, mesh100k or both")


def rmse(a, b):
    d = a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def timed(fn, reps):
    """Median ms of fn() between two HIP events on the null stream (the library's default), each call synchronised."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_scene(name, W, H, bounces, ref_spp, reps, sweep):
    spec = scene_spec(name)
    npix = W * H
    res = {"scene": name, "W": W, "H": H, "bounces": bounces, "ref_spp": ref_spp}

    def ctx():
        sc = api.Scene(W, H, device=0).load(spec)
        sc.iterations = bounces
        return sc

    sc = ctx()
    sc.render(2)
    sc.sync()
    sc.current_sample = 0
    sc.seed_default()
    res["ref_ms"] = wall(lambda: sc.render(ref_spp))
    gt = sc.read_colors()
    sc.close()

    # ---- kernel times
    sc = ctx()
    sc.render(16)
    sc.sync()
    defaults = api.denoise_defaults()
    L = defaults["iterations"]
    for sub in (1, 2):
        ms = timed(lambda: sc.render_aovs(sub, 4), reps)
        res["aov_ms_sub%d" % sub] = ms
        res["aov_gbs_sub%d" % sub] = 32.0 * npix / (ms * 1e-3) / 1e9
    sc.render_aovs(2, 4)
    sc.sync()
    p = api.DenoiseParams(**defaults)
    import ctypes as C

    def den(iters):
        p.iterations = iters
        rc = api.LIB.pt_denoise(sc._h, C.byref(p))
        assert rc == 0, rc
    for iters in (1, L):
        ms = timed(lambda: den(iters), reps)
        nbytes = npix * (48 * iters + (32 if defaults["demodulate"] else 0))
        res["denoise_ms_L%d" % iters] = ms
        res["denoise_bytes_L%d" % iters] = nbytes
        res["denoise_tbs_L%d" % iters] = nbytes / (ms * 1e-3) / 1e12
        res["denoise_copy_frac_L%d" % iters] = nbytes / (ms * 1e-3) / 1e12 / COPY_TBS
    res["denoise_ms_per_iteration"] = res["denoise_ms_L%d" % L] / L
    sc.close()

    # ---- quality: raw and denoised against the reference
    curve = {}
    for spp in (4, 16, 64, 256):
        sc = ctx()
        t_render = wall(lambda: sc.render(spp))
        raw = sc.read_colors()
        t_den = wall(lambda: (sc.render_aovs(2, 4), den(L)))
        out = sc.read_denoised()
        curve[spp] = {"raw_rmse": rmse(raw, gt), "denoised_rmse": rmse(out, gt), "render_ms": t_render, "aov_denoise_ms": t_den,
                      "mean_rel": float(out[:, :3].astype(np.float64).mean() / gt[:, :3].astype(np.float64).mean() - 1.0)}
        if spp == 16:
            sc16 = sc
        else:
            sc.close()
    res["curve"] = curve
    xs = np.log(np.array(sorted(curve), dtype=np.float64))
    ys = np.log(np.array([curve[s]["raw_rmse"] for s in sorted(curve)]))
    target = np.log(curve[16]["denoised_rmse"])
    # raw RMSE falls with spp: spp(RMSE) on the log-log curve (clamped to its ends: report "> 256" as 256)
    res["matches_uniform_spp"] = float(np.exp(np.interp(target, ys[::-1], xs[::-1])))
    res["denoised16_wall_ms"] = curve[16]["render_ms"] + curve[16]["aov_denoise_ms"]

    # ---- sweep at 16 spp
    if sweep:
        raw16 = sc16.read_colors()
        sc16.render_aovs(2, 4)
        grid = {"sigma_color": [0.125, 0.25, 0.5, 1.0, 2.0, 4.0, float("inf")], "sigma_normal": [0.0, 8.0, 32.0, 64.0, 128.0],
                "sigma_depth": [0.05, 0.1, 0.25, 0.5, 1.0, float("inf")], "iterations": [3, 4, 5, 6, 7], "demodulate": [0, 1]}
        table = []
        best = dict(defaults)
        for key, vals in grid.items():
            row = []
            for v in vals:
                out = sc16.denoise(**dict(defaults, **{key: v}))
                row.append((v, rmse(out, gt)))
            table.append({"param": key, "rmse": [[v, r] for v, r in row]})
            best[key] = min(row, key=lambda t: t[1])[0]
        res["sweep"] = table
        res["sweep_best_per_axis"] = best
        res["sweep_best_combined_rmse"] = rmse(sc16.denoise(**best), gt)
        res["sweep_defaults_rmse"] = rmse(sc16.denoise(), gt)
        res["raw16_rmse"] = rmse(raw16, gt)
    sc16.close()
    return res


def main():
    a = dict(kv.split("=", 1) for kv in sys.argv[1:])
    names = ["cornell", "mesh100k"] if a.get("scene", "both") == "both" else [a["scene"]]
    W, H, B = int(a.get("W", 1920)), int(a.get("H", 1080)), int(a.get("bounces", 8))
    ref, reps, sweep = int(a.get("ref", 4096)), int(a.get("reps", 20)), int(a.get("sweep", 1))
    out_dir = a.get("out")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    for name in names:
        r = run_scene(name, W, H, B, ref, reps, sweep)
        print(json.dumps(r), flush=True)
        if out_dir:
            with open(os.path.join(out_dir, "%s_%dx%d.json" % (name, W, H)), "w") as f:
                json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
