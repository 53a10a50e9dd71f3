"""Records what the float64 path models of tests/*_ref.py compute, for tests/test_path_models_host.py: every class of the family, in every
configuration the suite constructs it in, on the replay scenes of the test_gpu_* files at a reduced frame size, on host-only contexts.

    python tests/golden/make_path_model_golden.py            # writes tests/golden/path_models.npz

For each case and strategy the file holds the colours of model.render() as uint64 bit patterns, the final LCG states, the near-tie mask and
every pixel_events array.  CASES is the one list of configurations: the test imports it and rebuilds each through the same builders, so the
file and the test cannot disagree about what a case is.  The file is a recording of the models as they were when it was written: it is
regenerated only when the estimator itself changes, never to make a refactor of the models pass."""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "path_models.npz")
STRATEGIES = {"bsdf": 0, "light": 1, "mis": 2}


def seeds_of(W, H, stream=17):
    return np.random.default_rng(stream).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)


@contextlib.contextmanager
def sized(W, H):
    """the replay builders that read their frame size from a module's REPLAY, at W x H"""
    import test_gpu_arealights as TA
    import test_gpu_frosted as TF
    import test_gpu_lights as TL
    saved = [(d, d["W"], d["H"]) for d in (TL.REPLAY, TA.REPLAY, TF.REPLAY)]
    try:
        for d, _, _ in saved:
            d["W"], d["H"] = W, H
        yield
    finally:
        for d, w, h in saved:
            d["W"], d["H"] = w, h


def parts(api, spec, smooth=True):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    normals = getattr(spec, "normals", None) or [None] * len(spec.objects)
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None or not smooth else n for (v, _), n in zip(spec.objects, normals)])
    return verts, api.triangles_from_vertices(verts, mo)["N"], mats, mo, vn


def sun_sky(sc):
    from opencl_path_tracer_amd import scenes
    rgb = scenes.sun_and_sky()
    sc.set_environment(rgb)
    return dict(rgb=rgb, tables=sc.debug_environment())


# ---------------------------------------------------------------------------- the builders: (api, W, H, **config) -> model
def nee(api, W, H):
    import nee_ref as R
    import test_gpu_nee as T
    spec = T.replay_spec(api)
    sc = api.Scene(W, H, device=None).load(spec)
    verts, N, mats, mo, _ = parts(api, spec)
    return R.Model(verts, N, mats, mo, sc.camera[0], table=sc.debug_light_table())


def env(api, W, H):
    import test_gpu_env as T
    spec, rgb = T.replay_spec(), T.replay_map()
    sc = api.Scene(W, H, device=None).load(spec)
    sc.set_environment(rgb, scale=T.REPLAY["scale"], yaw_degrees=T.REPLAY["yaw_degrees"], select=T.REPLAY["select"])
    return T.replay_model(api, sc, spec, rgb)


def lighttree(api, W, H):
    import lighttree_ref as LT
    import test_gpu_lighttree as T
    from opencl_path_tracer_amd import scenes
    spec = scenes.many_lights(16)
    sc = T.corridor(api, W, H, device=None)
    verts, N, mats, mo, _ = parts(api, spec)
    return LT.TreeModel(verts, N, mats, mo, sc.camera[0], table=sc.debug_light_table(), tree=LT.Tree(*sc.debug_light_tree()))


def smooth(api, W, H, sky):
    import test_gpu_smooth as T
    spec = T.replay_spec()
    sc = api.Scene(W, H, device=None).load(spec)
    e = sun_sky(sc) if sky else None
    sc.set_option("smooth_normals", 1)
    return T.replay_model(api, sc, spec, e)


def texture(api, W, H, sky, bound=True):
    import test_gpu_texture as T
    import texture_ref as TX
    spec = T.replay_spec()
    sc = api.Scene(W, H, device=None).load(spec)
    e = sun_sky(sc) if sky else None
    sc.set_option("smooth_normals", 1)
    sc.set_option("textures", 1)
    if bound:
        return T.replay_model(api, sc, spec, e)
    verts, N, mats, mo, vn = parts(api, spec)           # the guide-buffer tests' form: uvs, but nothing bound
    return TX.TextureModel(verts, N, mats, mo, sc.camera[0], vn, np.concatenate(spec.uvs), [], {}, table=sc.debug_light_table())


def glossy(api, W, H, sky, smooth=True, **flags):
    import glossy_ref as G
    import test_gpu_glossy as T
    spec = T.replay_spec()
    sc, e = T.replay_scene(api, spec, sky, W, H, smooth, device=None)
    if not flags:
        return T.replay_model(api, sc, spec, e, table=sc.debug_light_table(), smooth=smooth)
    verts, N, mats, mo, vn = parts(api, spec, smooth)
    return G.GlossyModel(verts, N, mats, mo, sc.camera[0], vn, env=e, table=sc.debug_light_table(), **flags)


def coated(api, W, H, sky, smooth=True, **flags):
    import coated_ref as K
    import test_gpu_coated as T
    spec = T.replay_spec()
    ps_err = T.float32_restatement(T.coated_inputs())[4]
    sc, e = T.replay_scene(api, spec, sky, W, H, smooth, device=None)
    if not flags:
        return T.replay_model(api, sc.camera[0], spec, e, table=sc.debug_light_table(), smooth=smooth, ps_margin=ps_err)
    verts, N, mats, mo, vn = parts(api, spec, smooth)
    return K.CoatedModel(verts, N, mats, mo, sc.camera[0], vn, env=e, table=sc.debug_light_table(), ps_margin=ps_err, **flags)


def frosted(api, W, H, sky, smooth=True, **flags):
    import frosted_ref as F
    import test_gpu_coated as TC
    import test_gpu_frosted as T
    spec = T.replay_spec()
    ps_err = TC.float32_restatement(TC.coated_inputs())[4]
    r = T.float32_restatement(T.frosted_inputs())
    sc, e = T.replay_scene(api, spec, sky, W, H, smooth, device=None)
    kw = dict(env=e, table=sc.debug_light_table(), ps_margin=ps_err, fm_margin=max(r[4], r[5]))
    if not flags:
        return T.replay_model(api, sc.camera[0], spec, smooth=smooth, **kw)
    verts, N, mats, mo, vn = parts(api, spec, smooth)
    return F.FrostedModel(verts, N, mats, mo, sc.camera[0], vn, **kw, **flags)


def lens(api, W, H, config):
    import test_gpu_lens as T
    from opencl_path_tracer_amd import scenes
    cfg = T.CONFIGS[config]
    spec = scenes.focus_row()
    sc = api.Scene(W, H, device=None).load(spec)
    e = sun_sky(sc) if cfg["sky"] else None
    for opt in ("smooth_normals", "textures", "glossy", "coated"):
        sc.set_option(opt, cfg["options"])
    sc.set_lens(*T.REPLAY["lens"])
    return T.replay_model(api, sc.camera[0], spec, cfg["options"], e, table=sc.debug_light_table())


def lights(api, W, H, sky=False, scene="box", empty=False):
    import lights_ref as L
    import medium_ref as M
    import test_gpu_lights as T
    with sized(W, H):
        if scene == "glossy":
            if not empty:
                sc, spec = T.glossy_replay_scene(api, device=None)
                return T.glossy_replay_model(api, sc, spec)
            spec = T.glossy_replay_spec()                # no set is held: the empty one
            sc = api.Scene(W, H, device=None).load(spec)
            verts, N, mats, mo, vn = parts(api, spec)
            return L.LightsModel(verts, N, mats, mo, sc.camera[0], M.NO_LIGHTS, vnormals=vn, table=sc.debug_light_table())
        sc, spec, rgb = T.replay_scene(api, sky, device=None)
        return T.replay_model(api, sc, spec, rgb, sky)


def medium(api, W, H, sky=False, scene="box", none=False):
    import medium_ref as M
    import test_gpu_lights as TL
    import test_gpu_medium as T
    with sized(W, H):
        if scene == "glossy":
            if none:                                    # nothing held: lights = None, medium = None
                spec = TL.glossy_replay_spec()
                sc = api.Scene(W, H, device=None).load(spec)
                verts, N, mats, mo, vn = parts(api, spec)
                return M.MediumModel(verts, N, mats, mo, sc.camera[0], None, sc.medium(), vnormals=vn, table=sc.debug_light_table())
            sc, spec = T.fog_glossy_replay_scene(api, device=None)
            return T.fog_glossy_replay_model(api, sc, spec)
        sc, spec, rgb = T.fog_replay_scene(api, sky, device=None)
        return T.fog_replay_model(api, sc, spec, rgb, sky)


def grid(api, W, H, sky=False, density=True):
    import grid_ref as GR
    import test_gpu_grid as T
    import test_gpu_medium as TM
    with sized(W, H):
        if density:
            sc, spec, rgb = T.grid_replay_scene(api, sky, device=None)
            return T.grid_replay_model(api, sc, spec, rgb, sky)
        sc, spec, rgb = TM.fog_replay_scene(api, sky, device=None)          # tests/test_grid_host.py's null case: density = None
        verts, N, mats, mo, _ = parts(api, spec)
        return GR.GridModel(verts, N, mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), table=sc.debug_light_table(), density=None)


def arealights(api, W, H, scene):
    import test_gpu_arealights as T
    with sized(W, H):
        if scene == "glossy":
            sc, spec = T.glossy_replay_scene(api, device=None)
            return T.glossy_replay_model(api, sc, spec)
        sky = scene != "box"
        sc, spec, rgb = T.replay_scene(api, sky, device=None, fog=scene == "fog")
        return T.replay_model(api, sc, spec, rgb, sky)


def interior(api, W, H, scene, bound=True):
    import interior_ref as IR
    import test_gpu_frosted as TF
    import test_gpu_interior as T
    with sized(W, H):
        if scene == "energy":
            saved = T.ENERGY["W"], T.ENERGY["H"]
            try:
                T.ENERGY["W"], T.ENERGY["H"] = W, H
                sc, spec, rgb = T.energy_scene(api, device=None)
            finally:
                T.ENERGY["W"], T.ENERGY["H"] = saved
            return T.energy_model(api, sc, spec, rgb)
        if scene == "frosted":
            sc, spec = T.frosted_replay_scene(api, device=None)
            model = T.frosted_replay_model(api, sc, spec)
            if not bound:
                verts, N, mats, mo, vn = parts(api, spec)
                model = IR.InteriorFrostedModel(verts, N, mats, mo, sc.camera[0], vn, table=sc.debug_light_table(), ps_margin=model.ps_margin,
                                                fm_margin=model.fm_margin, interiors={})
            return model
        sc, spec = T.interior_replay_scene(api, scene == "fog", device=None)
        if bound:
            return T.interior_replay_model(api, sc, spec)
        verts, N, mats, mo, vn = parts(api, spec)
        return IR.InteriorModel(verts, N, mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), {}, vnormals=vn, table=sc.debug_light_table())


ALL = ("bsdf", "light", "mis")
S, G, K, F = ("spec_fallback", "lobe_end", "ng_reject"), ("glossy_vertex", "glossy_end_wz", "glossy_light", "glossy_emitter_wb"), \
    ("coated_coat", "coated_base", "coated_end_wz", "coated_light", "coated_emitter_wb", "glossy_vertex"), \
    ("frosted_reflect", "frosted_refract", "frosted_tir", "frosted_inside", "frosted_light", "coated_coat", "glossy_vertex")
FOG = ("scatter", "scatter_light", "scatter_delta", "delta")
INT = ("interior_scatter", "interior_absorbed", "interior_exit", "interior_then_light")

# name: (builder, config, (W, H), spp, bounces, strategies, the events the GPU test of that scene asserts > 0 under mis in its kept pixels;
# a tuple inside stands for "their sum").  One further run per case with a single segment records the preview colour of iterations == 1.
CASES = {
    "nee": (nee, {}, (24, 16), 2, 4, ALL, ()),
    "env": (env, {}, (24, 16), 2, 4, ALL, ()),
    "lighttree": (lighttree, {}, (16, 16), 2, 4, ALL, ()),
    "smooth": (smooth, dict(sky=False), (24, 16), 2, 4, ALL, S),
    "smooth_sky": (smooth, dict(sky=True), (24, 16), 2, 4, ("mis",), S),
    "texture": (texture, dict(sky=False), (24, 16), 2, 4, ALL, ()),
    "texture_sky": (texture, dict(sky=True), (24, 16), 2, 4, ("mis",), ()),
    "texture_unbound": (texture, dict(sky=False, bound=False), (16, 12), 2, 4, ("mis",), ()),
    "glossy": (glossy, dict(sky=False), (32, 24), 2, 4, ("mis",), G + ("glossy_end_ng",)),
    "glossy_small": (glossy, dict(sky=False), (16, 12), 2, 4, ALL, ()),
    "glossy_sky": (glossy, dict(sky=True), (32, 24), 2, 4, ("mis",), G + ("glossy_end_ng", "glossy_sky")),
    "glossy_flat": (glossy, dict(sky=False, smooth=False), (32, 24), 2, 4, ("mis",), G),
    "glossy_off": (glossy, dict(sky=False, glossy=False), (16, 12), 2, 4, ("mis",), ()),
    "coated": (coated, dict(sky=False), (32, 24), 4, 4, ("mis",), K + ("coated_end_ng",)),
    "coated_small": (coated, dict(sky=False), (16, 12), 4, 4, ALL, ()),
    "coated_sky": (coated, dict(sky=True), (32, 24), 4, 4, ("mis",), K + ("coated_end_ng", "coated_sky")),
    "coated_flat": (coated, dict(sky=False, smooth=False), (32, 24), 4, 4, ("mis",), K),
    "coated_off": (coated, dict(sky=False, glossy=False, coated=False), (16, 12), 4, 4, ("mis",), ()),
    "frosted": (frosted, dict(sky=False), (24, 18), 4, 4, ("mis",), F + ("frosted_end_ng",)),
    "frosted_small": (frosted, dict(sky=False), (16, 12), 4, 4, ALL, ()),
    "frosted_sky": (frosted, dict(sky=True), (24, 18), 4, 4, ("mis",), F + ("frosted_end_ng", ("frosted_sky", "frosted_through_sky"))),
    "frosted_flat": (frosted, dict(sky=False, smooth=False), (24, 18), 4, 4, ("mis",), F),
    "frosted_off": (frosted, dict(sky=False, glossy=False, coated=False, frosted=False), (16, 12), 4, 4, ("mis",), ()),
    "lens_on": (lens, dict(config="on"), (32, 24), 4, 4, ("mis",), ("glossy_vertex", "coated_coat", "coated_base")),
    "lens_off": (lens, dict(config="off"), (16, 12), 4, 4, ALL, ()),
    "lens_sky": (lens, dict(config="sky"), (32, 24), 4, 4, ("mis",), ("glossy_vertex", "coated_coat", "coated_base")),
    "lights": (lights, dict(sky=False), (24, 16), 2, 4, ALL, ()),
    "lights_sky": (lights, dict(sky=True), (24, 16), 2, 4, ("light", "mis"), ()),
    "lights_glossy": (lights, dict(scene="glossy"), (32, 24), 2, 4, ("mis",),
                      ("delta", "delta_glossy", "delta_ng_reject", "glossy_vertex", "glossy_light", "glossy_emitter_wb", "spec_fallback")),
    "lights_empty": (lights, dict(scene="glossy", empty=True), (16, 12), 2, 4, ("mis",), ()),
    "medium": (medium, dict(sky=False), (24, 16), 2, 4, ALL, FOG),
    "medium_sky": (medium, dict(sky=True), (24, 16), 2, 4, ("light", "mis"), FOG + ("scatter_sky",)),
    "medium_glossy": (medium, dict(scene="glossy"), (24, 16), 2, 4, ("mis",),
                      ("scatter", "scatter_light", "scatter_delta", "glossy_vertex", "glossy_light", "delta_glossy")),
    "medium_none": (medium, dict(scene="glossy", none=True), (16, 12), 2, 4, ("mis",), ()),
    "grid": (grid, {}, (24, 16), 2, 4, ALL, FOG + ("grid_scatter_thin", "grid_scatter_dense", "grid_empty_crossed", "grid_light_partial")),
    "grid_none": (grid, dict(density=False), (16, 12), 2, 4, ("mis",), ()),
    "area_box": (arealights, dict(scene="box"), (24, 16), 2, 4, ALL, ("sphere_end", "sun_miss", "area_sample", "sphere_blocks")),
    "area_sky": (arealights, dict(scene="box_sky"), (24, 16), 2, 4, ALL, ("sphere_end", "sun_miss", "area_sample")),
    "area_fog": (arealights, dict(scene="fog"), (24, 16), 2, 4, ALL, ("scatter", "scatter_light", "sphere_end", "sphere_end_scatter", "area_sample")),
    "area_glossy": (arealights, dict(scene="glossy"), (24, 16), 2, 4, ("mis",),
                    ("sphere_end_rough", "area_glossy", "area_ng_reject", "glossy_vertex", "sphere_blocks")),
    "interior": (interior, dict(scene="clear"), (32, 24), 2, 8, ("mis",), INT),
    "interior_fog": (interior, dict(scene="fog"), (32, 24), 2, 8, ("mis",), INT + ("scatter",)),
    "interior_small": (interior, dict(scene="fog"), (16, 12), 2, 8, ALL, ()),
    "interior_unbound": (interior, dict(scene="clear", bound=False), (16, 12), 2, 8, ("mis",), ()),
    "interior_energy": (interior, dict(scene="energy"), (48, 32), 1, 12, ("bsdf",), ()),
    "interior_frosted": (interior, dict(scene="frosted"), (32, 24), 4, 8, ("mis",), INT + ("frosted_refract", "frosted_inside")),
    "interior_frosted_small": (interior, dict(scene="frosted"), (16, 12), 4, 8, ALL, ()),
    "interior_frosted_unbound": (interior, dict(scene="frosted", bound=False), (16, 12), 4, 8, ("mis",), ()),
}
PREVIEW_PIXELS = 192                                             # of the frame's first rows
NO_PREVIEW = ("texture", "texture_sky", "texture_unbound")       # TextureModel does not model iterations == 1


def runs(name):
    """the (key, strategy, iterations) of a case's recorded runs"""
    _, _, _, _, bounces, strategies, _ = CASES[name]
    out = [(s, STRATEGIES[s], bounces) for s in strategies]
    if name not in NO_PREVIEW:
        out.append(("preview", 2, 1))
    return out


def record(api, name):
    """{"<case>/<run>/<array>": array} of one case, and the model's events under mis"""
    build, config, (W, H), spp, _, _, _ = CASES[name]
    model = build(api, W, H, **config)
    seeds = seeds_of(W, H)
    out = {}
    for key, strategy, iterations in runs(name):
        cols, states, ties = model.render(seeds if iterations > 1 else seeds[:PREVIEW_PIXELS], iterations, spp, strategy)
        pre = "%s/%s/" % (name, key)
        out[pre + "colors"] = np.ascontiguousarray(cols, dtype=np.float64).view(np.uint64)
        out[pre + "seeds"] = np.asarray(states, dtype=np.int32)
        out[pre + "ties"] = np.asarray(ties, dtype=bool)
        events = getattr(model, "pixel_events", {})
        out[pre + "event_names"] = np.asarray(sorted(events), dtype="U32")
        out[pre + "events"] = np.asarray([events[e] for e in sorted(events)], dtype=np.int32).reshape(len(events), len(ties))
        if hasattr(model, "textured_vertices"):
            out[pre + "textured_vertices"] = np.asarray(model.textured_vertices, dtype=np.int64)
    return out


def check_events(name, rec):
    """every event the scene's GPU test needs is in the recorded frame's kept pixels (strategy mis)"""
    need = CASES[name][6]
    if not need:
        return
    keep = ~rec["%s/mis/ties" % name]
    names = rec["%s/mis/event_names" % name].tolist()
    for e in need:
        group = e if isinstance(e, tuple) else (e,)
        assert sum(int(rec["%s/mis/events" % name][names.index(g)][keep].sum()) for g in group) > 0, (name, e)


def main():
    import time
    from opencl_path_tracer_amd import api
    out = {}
    for name in CASES:
        t0 = time.time()
        rec = record(api, name)
        check_events(name, rec)
        out.update(rec)
        print("%-26s %5.1f s, near ties %s" % (name, time.time() - t0, {k.split("/")[1]: int(v.sum()) for k, v in rec.items() if k.endswith("/ties")}))
    np.savez_compressed(PATH, **out)
    print("%s: %d arrays, %d bytes" % (PATH, len(out), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
