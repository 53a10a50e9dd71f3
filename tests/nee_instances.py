"""The table of k_nee instances and the scenes that reach them (tests/test_nee_instances_host.py, tests/test_gpu_nee_instances.py;
DESIGN.md section 5.18).  Importable without a device.

pt_nee.hip compiles nine kernel families (NeeFamily, pt_internal.hpp), each in four forms (k_nee<family, mode, block, ENV, TILED>: plain, env, tiles, env_tiles), each
for four node modes: 144 device functions.  CELLS lists them with the scene that serves each and the workgroup size its launch must
take; the rest of the module builds the two scenes, the ten configurations that select the families, and the node placements."""
import functools
from collections import namedtuple

import numpy as np

FAMILIES = ("plain", "smooth", "tex", "glossy", "coated", "lens", "frosted", "lights", "medium")      # stat "nee_family" 0..8
FORMS = ("plain", "env", "tiles", "env_tiles")              # stat "nee_form" 0..3: bit 0 an environment is drawn, bit 1 tiled
MODES = (0, 1, 2, 3)                                        # stat "node_mode": whole tree in LDS, BVH2 from global memory, treelet, 4-wide
# launch_nee's kNeeWide table per family (kWidePlain = 1, kWideEnv = 2, kWideTiles = 4, kWideEnvTiles = 8: bit f is form f): the forms
# that launch through launch_lanes_wide, whose treelet shape has 512 threads, instead of launch_lanes, whose has 1,024
WIDE_SHAPES = (0, 8, 2 | 8, 15, 15, 15, 15, 15, 15)
SCENES_OF_MODE = {0: ("small",), 1: ("small", "mesh"), 2: ("mesh",), 3: ("small", "mesh")}


def block_of(family, form, mode):
    """the workgroup size of the instance's launch: the switch statements of launch_lanes and launch_lanes_wide"""
    if mode in (1, 3):
        return 256
    if mode == 0:
        return 512
    return 512 if WIDE_SHAPES[family] >> form & 1 else 1024


Cell = namedtuple("Cell", "family form mode scenes block")
CELLS = [Cell(f, form, mode, SCENES_OF_MODE[mode], block_of(f, form, mode)) for f in range(len(FAMILIES)) for form in range(len(FORMS)) for mode in MODES]

FRAME = (52, 36)            # neither side a multiple of 8: partial tiles; 1,872 pixels: no multiple of 256, 512 or 1,024
OVERFLOW_LDS_ENTRIES = 6    # tests/test_gpu_nee.py's wide_lds_entries: the rest of the 4-wide stack lives in global memory

# (options set before load, options set after load, the node mode they select) -- as tests/test_gpu_smooth.py, test_gpu_nee.py and
# test_gpu_parity.py select the modes
PLACEMENTS = {
    "small": {"lds": ({}, {}, 0), "global": ({}, {"lds_scene": 0}, 1), "wide": ({"wide_nodes": 2}, {}, 3),
              "wide_overflow": ({"wide_nodes": 2, "wide_lds_entries": OVERFLOW_LDS_ENTRIES}, {}, 3)},
    "mesh": {"global": ({"wide_nodes": 0, "treelet": 0}, {}, 1), "treelet": ({"treelet": 40, "wide_nodes": 1}, {}, 2), "wide": ({"wide_nodes": 2}, {}, 3)},
}

# ---------------------------------------------------------------------------- configurations
# one per family with every feature up to that family live, and the medium alone on an otherwise plain scene
FEATURES = FAMILIES[1:]
CONFIGS = FAMILIES + ("medium_alone",)
OPTION_OF = {"smooth": "smooth_normals", "tex": "textures", "glossy": "glossy", "coated": "coated", "frosted": "frosted"}
LENS = (25.0, 1600.0)
LIGHT = dict(position=(200.0, 800.0, 100.0), intensity=(4e6, 3e6, 2e6), select=0.4)      # test_gpu_lights.box_light: under the ceiling
FOG_SIGMA_T = 1e-3          # one mean free path per room width, as scenes.cornell_box(fog=1e-3)


def features(config):
    if config == "medium_alone":
        return ("medium",)
    return FEATURES[:FAMILIES.index(config)]


def family_of(config):
    return FAMILIES.index("medium" if config == "medium_alone" else config)


def below(config):
    """the configuration whose frame this one's must differ from (None: plain)"""
    if config == "medium_alone":
        return "plain"
    k = FAMILIES.index(config)
    return FAMILIES[k - 1] if k else None


# ---------------------------------------------------------------------------- scenes
def _rich_materials(scenes):
    chromium, glass = scenes.BUILTIN_MATERIALS[scenes.CHROMIUM], scenes.BUILTIN_MATERIALS[scenes.GLASS]
    return [tuple(chromium[:5]) + (50.0, 4),                                                        # rough metal
            ((0.7, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (1.5, 1.5, 1.5), (0, 0, 0), 300.0, 5),          # red plastic
            tuple(glass[:5]) + (30.0, 6)]                                                           # frosted glass


def small_spec():
    """scenes.cornell_box with every feature's data (1,932 triangles: the whole tree fits in LDS).  The first sphere is a third rough
    metal (type 4), a third chromium and a third plastic (type 5, appended); the second half frosted (type 6), half glass."""
    from opencl_path_tracer_amd import scenes
    spec = scenes.cornell_box(smooth=True, textured=True, glossy=True, frosted=True)
    spec.name = "nee_instances_small"
    spec.materials.append(_rich_materials(scenes)[1])
    plastic = len(spec.materials) - 1
    v1, m1 = spec.objects[1]
    m1 = m1.copy()
    n = len(m1)
    m1[n // 3:2 * n // 3] = scenes.CHROMIUM
    m1[2 * n // 3:] = plastic
    spec.objects[1] = (v1, m1)
    v2, m2 = spec.objects[2]
    m2 = m2.copy()
    m2[len(m2) // 2:] = scenes.GLASS
    spec.objects[2] = (v2, m2)
    return spec


def mesh_spec(rich=True):
    """scenes.displaced_grid_mesh(6000) (6,062 triangles: too large for LDS, so a treelet can be cut).  rich: six material bands --
    WHITE, CHROMIUM, GLASS and appended types 4, 5 and 6 --, uvs (x, z) / 1000 on the mesh and a bilinear checker bound to WHITE.
    Not rich (the float64 anchor, whose model has no type 5, type 6 or textures): four bands, WHITE, CHROMIUM, GLASS and type 4.
    The mesh's vertex normals are computed on the context (Scene.compute_vertex_normals(60.0, obj=1))."""
    from opencl_path_tracer_amd import scenes
    spec = scenes.displaced_grid_mesh(6000)
    spec.name = "nee_instances_mesh" if rich else "nee_instances_anchor"
    extra = _rich_materials(scenes) if rich else _rich_materials(scenes)[:1]
    first = len(spec.materials)
    spec.materials.extend(extra)
    verts, _ = spec.objects[1]
    nt = len(verts)
    ids = [scenes.WHITE_DIFFUSE, scenes.CHROMIUM, scenes.GLASS] + list(range(first, first + len(extra)))
    band = (np.arange(nt) * len(ids)) // nt
    spec.objects[1] = (verts, np.asarray(ids, dtype=np.uint16)[band])
    if rich:
        spec.uvs = [None, (verts[:, :, [0, 2]] / np.float32(1000.0)).astype(np.float32)]
        spec.textures = [(scenes.checker_texture(8, (1.0, 1.0, 1.0), (0.25, 0.25, 0.25)), dict(filter=1, srgb=0))]
        spec.material_textures = {scenes.WHITE_DIFFUSE: 0}
    return spec


@functools.lru_cache(maxsize=None)
def scene_spec(scene, smooth, tex):
    """the scene's spec as a configuration loads it: without smooth the vertex normals are left out, without tex the uvs, the texture
    and its binding, so the plain and medium-alone configurations hand their kernels null views and not merely cleared options"""
    spec = small_spec() if scene == "small" else mesh_spec()
    if not smooth:
        spec.normals = []
    if not tex:
        spec.uvs, spec.textures, spec.material_textures = [], [], {}
    return spec


def _place(api, spec, scene, placement, device, size):
    before, after, mode = PLACEMENTS[scene][placement]
    sc = api.Scene(size[0], size[1], device=device)
    for k, v in before.items():
        sc.set_option(k, v)
    sc.load(spec)
    for k, v in after.items():
        sc.set_option(k, v)
    return sc, mode


def build(api, scene, config, placement, sky=False, device=0, size=FRAME):
    """(context, the node mode the placement selects): the scene loaded for the configuration, every feature of it switched on"""
    from opencl_path_tracer_amd import scenes
    feats = features(config)
    sc, mode = _place(api, scene_spec(scene, "smooth" in feats, "tex" in feats), scene, placement, device, size)
    if scene == "mesh" and "smooth" in feats:
        sc.compute_vertex_normals(60.0, obj=1)
    for f in feats:
        if f in OPTION_OF:
            sc.set_option(OPTION_OF[f], 1)
    if "lens" in feats:
        sc.set_lens(*LENS)
    if "lights" in feats:
        sc.set_lights([api.point_light(LIGHT["position"], LIGHT["intensity"])], select=LIGHT["select"])
    if "medium" in feats:
        sc.set_medium(FOG_SIGMA_T, albedo=(0.9, 0.9, 0.9), g=0.6, bounds=scenes.CORNELL_ROOM)
    if sky:
        sc.set_environment(scenes.sun_and_sky())
    return sc, mode


# ---------------------------------------------------------------------------- the float64 anchor of the 512-thread treelet shape
ANCHOR = dict(W=32, H=24, seed=29, select=0.5)


def anchor_lights(api):
    """inside the room, over the mesh: a point light, and a spot that shines down onto the rough-metal band"""
    return [api.point_light((300.0, 700.0, 0.0), (3e6, 2.8e6, 2.4e6)),
            api.spot_light((700.0, 800.0, 400.0), (-0.1, -1.0, 0.2), (9e6, 8e6, 6e6), 25.0, 45.0)]


def anchor_seeds():
    return np.random.default_rng(ANCHOR["seed"]).integers(1, 2 ** 31 - 2, ANCHOR["W"] * ANCHOR["H"]).astype(np.int32)


def build_anchor(api, placement, sky, device=0):
    """(context, mode, spec, sky map or None): mesh_spec(rich=False) with computed normals, options smooth_normals and glossy, two
    lights and the room's fog: what tests/medium_ref.py's MediumModel composes"""
    from opencl_path_tracer_amd import scenes
    spec = mesh_spec(rich=False)
    sc, mode = _place(api, spec, "mesh", placement, device, (ANCHOR["W"], ANCHOR["H"]))
    sc.compute_vertex_normals(60.0, obj=1)
    sc.set_option("smooth_normals", 1)
    sc.set_option("glossy", 1)
    sc.set_lights(anchor_lights(api), select=ANCHOR["select"])
    sc.set_medium(FOG_SIGMA_T, albedo=(0.9, 0.7, 0.5), g=0.6, bounds=scenes.CORNELL_ROOM)
    rgb = None
    if sky:
        rgb = scenes.sun_and_sky()
        sc.set_environment(rgb)
    return sc, mode, spec, rgb


def anchor_model(api, sc, spec, rgb):
    import medium_ref as M
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn, has = sc.debug_vertex_normals()
    vn = np.where(has[:, None, None], vn, np.float32(0.0))
    env = dict(rgb=rgb, tables=sc.debug_environment()) if rgb is not None else None
    return M.MediumModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), vnormals=vn, env=env, table=sc.debug_light_table())
