"""-m gpu: every k_nee instance -- nine families x four forms x four node modes (tests/nee_instances.py).

  (a) per (configuration, form): on the small scene the frames of the tree in LDS, BVH2 nodes from global memory, 4-wide nodes and
  4-wide nodes with the stack overflowing into global memory are equal bit for bit; on the mesh those of BVH2 nodes from global
  memory, the treelet and 4-wide nodes.  After every render stats node_mode, nee_family, nee_form and nee_block are the cell's, so
  a cell counts only when its instance ran.  (b) the 512-thread treelet shape of the medium family against tests/medium_ref.py.

The mode-0 instances are held to float64 models and to the families below them by the feature tests (test_gpu_smooth.py ..
test_gpu_medium.py); the bit-equalities here carry that to the other three modes of every instance."""

import time

import numpy as np
import pytest

import nee_instances as I
import test_gpu_lights as TL
import test_gpu_medium as TM

pytestmark = pytest.mark.gpu

same_bits = TL.same_bits
COVERED = {}                # (family, form, mode) -> the workgroup size read from stat "nee_block"
FRAMES = {}                 # (configuration, form, scene) -> the colours of the frame, every mode's


def check_cell(sc, config, form, mode):
    got = tuple(int(sc.stat(k)) for k in ("node_mode", "nee_family", "nee_form", "nee_block"))
    family = I.family_of(config)
    assert got == (mode, family, form, I.block_of(family, form, mode)), (config, I.FORMS[form], got)
    COVERED[(family, form, mode)] = got[3]


def threshold_of(sc):
    """tests/test_gpu_smooth.py's: with threshold 0 nothing retires and tile_state() holds every tile's estimate at the last decision;
    their median retires about half of the tiles there and the quietest ones earlier"""
    sc.render_adaptive(4, 16, 0.0, metric="half", path="nee", strategy="mis")
    thr = float(np.median(sc.tile_state()[1]))
    assert np.isfinite(thr) and thr > 0.0
    sc.current_sample = 0
    sc.seed_default()
    return thr


def render(sc, form, thr):
    """the compared state: test_gpu_lights.state, or colours, rnds and sample counts of a tiled form"""
    sc.iterations = TL.CB_BOUNCES
    if form & 2:
        sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy="mis")
        return sc.read_colors().copy(), sc.read_rnds().copy(), sc.sample_counts().copy()
    sc.render_nee(3, "mis")
    return TL.state(sc)


def same_frames(a, b):
    return len(a) == len(b) and all(same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))


def scene_frames(api, scene, config, form):
    """{placement: state} of one scene, every placement's cell checked; the tiled forms share one threshold, taken in the first"""
    out, thr = {}, None
    for placement in I.PLACEMENTS[scene]:
        sc, mode = I.build(api, scene, config, placement, sky=bool(form & 1))
        assert sc.stat("node_mode") == mode
        if placement == "wide_overflow":          # wide_stack_entries(pending) = ((pending + 4) + 1) & ~1 entries, of which 6 stay in LDS
            assert ((int(sc.stat("wide_pending")) + 5) & ~1) > I.OVERFLOW_LDS_ENTRIES and sc.stat("wide_nodes") > 0
        if form & 2 and thr is None:
            sc.iterations = TL.CB_BOUNCES
            thr = threshold_of(sc)
        out[placement] = render(sc, form, thr)
        check_cell(sc, config, form, mode)
        sc.close()
    return out


def reference_frame(api, scene, config, form):
    """the colours of (configuration, form) on a scene: the main test's, or -- when that has not run in this process -- one render with
    BVH2 nodes from global memory, which both scenes serve"""
    key = (config, form, scene)
    if key not in FRAMES:
        sc, _ = I.build(api, scene, config, "global", sky=bool(form & 1))
        thr = None
        if form & 2:
            sc.iterations = TL.CB_BOUNCES
            thr = threshold_of(sc)
        FRAMES[key] = render(sc, form, thr)[0]
        sc.close()
    return FRAMES[key]


@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
@pytest.mark.parametrize("config", I.CONFIGS)
def test_node_modes_render_the_same_bits(api, config, form):
    t0 = time.time()
    differs = []
    for scene, first in (("small", "lds"), ("mesh", "treelet")):
        frames = scene_frames(api, scene, config, form)
        want = frames[first]
        assert np.isfinite(want[0]).all() and want[0][:, :3].mean() > 0.0, scene
        if form & 2:
            seen = sorted(set(int(c) for c in np.unique(want[2])))
            assert set(seen) <= {4, 8, 16} and len(seen) >= 2, (scene, seen)
        for placement, got in frames.items():
            assert same_frames(got, want), (config, I.FORMS[form], scene, placement)
        FRAMES[(config, form, scene)] = want[0]
        if I.below(config) is not None:               # the feature is live: the frame is not the one of the configuration below
            differs.append(not same_bits(want[0], reference_frame(api, scene, I.below(config), form)))
    assert I.below(config) is None or any(differs), config
    print("%s / %s: %.2f s; blocks %s" % (config, I.FORMS[form], time.time() - t0,
                                         {m: COVERED[(I.family_of(config), form, m)] for m in I.MODES}))


# ---------------------------------------------------------------------------- (b) the float64 anchor of the 512-thread treelet shape
@pytest.mark.parametrize("sky", [False, True])
def test_treelet_shape_matches_float64_model(api, sky):
    """nee_instances.build_anchor: the 6,062-triangle mesh with bands WHITE, CHROMIUM, GLASS and type 4, computed vertex normals,
    options smooth_normals and glossy, a point and a spot light, fog in scenes.CORNELL_ROOM, with and without scenes.sun_and_sky();
    strategy mis, 2 spp, 4 bounces, 32 x 24, rendered by k_nee_medium / k_nee_env_medium in the treelet mode's 512-thread shape and
    compared by test_gpu_medium.check_replay (its tolerance, its 10 % cap on near ties).
    The model alone, on these seeds, flags 2.08 % (no sky) / 1.43 % (sky) of the 768 pixels as near ties (measured on a host-only
    context before the first GPU run).  In the kept pixels, without / with the sky: 2,939 / 2,956 scatter vertices in 1,536 samples
    (745 / 750 pixels scatter at least once), 1,482 / 969 light samples at one reach their light, 363 / 366 of them a delta light's;
    199 / 200 glossy vertices with 87 / 63 light samples at one, 225 / 227 delta samples at a surface (32 weighted at a rough vertex),
    11 specular fall-backs to Ng, 12 / 8 light samples refused by Ng alone, 9 / 10 emitter hits after a scatter vertex with W_b < 1,
    and 38 sky misses after a scatter vertex.  The model takes 7.5 s of CPU time per sky setting (brute force over 6,062 triangles).
    The same scene's frames with BVH2 nodes from global memory and with 4-wide nodes are the treelet frame bit for bit."""
    frames = {}
    for placement in ("treelet", "global", "wide"):
        sc, mode, spec, rgb = I.build_anchor(api, placement, sky)
        seeds = I.anchor_seeds()
        sc.upload_seeds(seeds)
        sc.iterations = TL.REPLAY["bounces"]
        sc.render_nee(TL.REPLAY["spp"], "mis")
        assert (sc.stat("nee_family"), sc.stat("node_mode"), sc.stat("nee_block"), sc.stat("nee_form")) == (8, mode, 512 if mode == 2 else 256, int(sky))
        frames[placement] = TL.state(sc)
        if placement == "treelet":
            model = I.anchor_model(api, sc, spec, rgb)
            assert model.pa == I.ANCHOR["select"] and len(model.set) == 2 and len(model.lights) > 0 and model.medium["sigma_t"] == float(np.float32(I.FOG_SIGMA_T))
            need = ("scatter", "scatter_light", "scatter_delta", "delta", "glossy_vertex", "glossy_light", "spec_fallback") + (("scatter_sky",) if sky else ())
            TM.check_replay(sc, model, seeds, 2, need)
        sc.close()
    assert TL.same_state(frames["global"], frames["treelet"]) and TL.same_state(frames["wide"], frames["treelet"])
