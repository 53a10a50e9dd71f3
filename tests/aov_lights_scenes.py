"""The authored scenes of the lit guide buffers' tests (option aov_lights), shared by tests/test_aov_lights_host.py, which checks on the
CPU that none of their per-pixel decisions lies within 1e-3 relative of its other outcome (tests/aov_lights_ref.py), and by
tests/test_gpu_aov_lights.py, which renders them.  Every scene is seen from the origin along +z with a 60 degree field of view; a scene
is (SceneSpec with its area lights, W, H)."""
import numpy as np

EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)
TAN_HALF = 8.0 / 13.856404           # the camera's half width at unit distance

WALL = ((0.7, 0.6, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)
GREY = ((0.4, 0.4, 0.4), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)


def quad(a, b, c, d):
    return [(a, b, c), (a, c, d)]


def wall_at(z, half=30.0):
    """a wall across the view (off centre: no pixel centre on its diagonal)"""
    return quad((-half - 0.3, -half + 0.8, z), (half - 0.9, -half + 0.8, z), (half - 0.9, half + 1.4, z), (-half - 0.3, half + 1.4, z))


def sphere(center, radius, radiance):
    return dict(kind="sphere", center=tuple(float(v) for v in center), radius=float(radius), radiance=tuple(float(v) for v in radiance))


def sun(axis, diameter_degrees, radiance):
    """a sun seen in the direction `axis` (its light travels along -axis)"""
    return dict(kind="sun", direction=tuple(-float(v) for v in axis), angular_diameter_degrees=float(diameter_degrees),
                radiance=tuple(float(v) for v in radiance))


def pixel_direction(x, y, W, H):
    """the unit direction of pixel (x, y)'s centre ray"""
    d = np.array([TAN_HALF * ((2.0 * (x + 0.5)) / W - 1.0), TAN_HALF * ((2.0 * (y + 0.5)) / H - 1.0), 1.0])
    return d / np.linalg.norm(d)


def _spec(name, tris, mati, lights, materials=(WALL, GREY)):
    from opencl_path_tracer_amd import scenes
    spec = scenes.SceneSpec(materials=list(materials), shift=EYE_AT_ORIGIN, name=name)
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mati, dtype=np.uint16)))
    spec.area_lights = list(lights)
    return spec


BEHIND = [((-1.0, -1.0, -5.0), (1.0, -1.0, -5.0), (0.0, 1.0, -5.0))]        # a triangle no camera ray meets: the scene of "nothing"


def primary_scenes():
    """{name: (spec, W, H)}: the scenes of the primary-ray test"""
    out = {}
    out["front"] = (_spec("front", wall_at(10.0), [0, 0], [sphere((0.42, 0.41, 6.0), 1.3, (5.0, 4.0, 3.0))]), 16, 16)
    out["nothing"] = (_spec("nothing", BEHIND, [0], [sphere((0.42, 0.41, 6.0), 1.3, (5.0, 4.0, 3.0))]), 16, 16)
    out["hidden"] = (_spec("hidden", wall_at(4.0), [0, 0], [sphere((0.42, 0.41, 6.0), 1.3, (5.0, 4.0, 3.0))]), 16, 16)
    out["two"] = (_spec("two", wall_at(14.0), [0, 0], [sphere((0.7, 0.1, 9.0), 2.55, (1.0, 2.0, 3.0)), sphere((0.41, 0.28, 5.0), 0.8, (5.0, 4.0, 3.0))]), 16, 16)
    out["inside"] = (_spec("inside", wall_at(10.0), [0, 0], [sphere((0.1, -0.2, 0.5), 2.0, (9.0, 9.0, 9.0)), sphere((0.42, 0.41, 6.0), 1.3, (5.0, 4.0, 3.0))]), 16, 16)
    # 64 spheres, each on the centre ray of every other pixel of a 16 x 16 frame at a distance of its own, with the angular radius
    # asin(sqrt(0.0015)): its own pixel's ray meets it with a discriminant of 1.5e-3 b^2 and every other ray misses it by more than 1e-3 b^2
    W = H = 16
    many = []
    for k in range(64):
        i, j = k % 8, k // 8
        dist = 5.0 + 0.05 * ((k * 37) % 64)
        many.append(sphere(pixel_direction(2 * i + (j & 1), 2 * j + 1, W, H) * dist, np.sqrt(0.0015) * dist, (1.0 + k, 0.5 * (64 - k), 2.0 + (k % 5))))
    out["sixtyfour"] = (_spec("sixtyfour", wall_at(12.0), [0, 0], many), W, H)
    out["suns"] = (suns_scene(), 16, 16)
    return out


SUN_A = dict(axis=(0.10, 0.30, 1.0), diameter=17.0, radiance=(40.0, 36.0, 30.0))
SUN_B = dict(axis=(0.21, 0.36, 1.0), diameter=13.0, radiance=(1.0, 2.0, 4.0))


def suns_scene():
    """suns only: a wall over the lower part of the frame, two overlapping suns in the sky above it and a third behind the camera"""
    low = quad((-30.0, -30.0, 10.0), (30.0, -30.0, 10.0), (30.0, 0.53, 10.0), (-30.0, 0.53, 10.0))
    lights = [sun(SUN_A["axis"], SUN_A["diameter"], SUN_A["radiance"]), sun(SUN_B["axis"], SUN_B["diameter"], SUN_B["radiance"]),
              sun((0.0, 0.0, -1.0), 20.0, (7.0, 7.0, 7.0))]
    return _spec("suns", low, [0, 0], lights)


# ---------------------------------------------------------------------------- the chains
# 8 x 8: the 64 centre rays and the 256 rays of subpixels 2 all stay clear of every rim by 1e-3 (the placements were searched for on the CPU)
CHAIN = dict(W=8, H=8, depth=4)
CHAIN_LIGHTS = [
    sphere((1.92, 0.21, 8.61), 1.28, (6.0, 5.0, 4.0)),             # 0 behind the glass slab
    sphere((-3.93, 1.63, -0.23), 2.33, (3.0, 6.0, 9.0)),            # 1 beside the camera, out of its view: seen in the mirror only
    sphere((-2.38, -1.31, 4.0), 0.62, (8.0, 1.0, 1.0)),           # 2 in front of the mirror: it ends the chain at d = 0
    sun((-0.25, -0.23, -1.0), 21.4, (20.0, 18.0, 15.0)),         # 3 behind the camera: seen in the mirror only
]
MIRROR_BEND = 0.06             # the mirror's vertex normals lean outwards by this much: under smooth_normals it is slightly convex


def chain_spec(lights=None):
    """a flat mirror with bent vertex normals on the left (a sphere light in front of it, one beside the camera and a sun behind it), a
    glass slab with a sphere light behind it on the right, and a back wall"""
    from opencl_path_tracer_amd import scenes
    mats = [WALL, GREY, scenes.BUILTIN_MATERIALS[scenes.CHROMIUM], scenes.BUILTIN_MATERIALS[scenes.GLASS]]
    back = wall_at(12.0, 11.0)
    corners = [(-4.1, -3.6, 6.0), (-0.23, -3.6, 6.0), (-0.23, 3.3, 6.0), (-4.1, 3.3, 6.0)]
    mirror = quad(*corners)
    slab = quad((0.31, -3.3, 5.0), (3.6, -3.3, 5.0), (3.6, 3.4, 5.0), (0.31, 3.4, 5.0)) + quad((0.31, -3.3, 5.4), (3.6, -3.3, 5.4), (3.6, 3.4, 5.4), (0.31, 3.4, 5.4))
    tris = np.asarray(back + mirror + slab, dtype=np.float32)
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="aov_lights_chain")
    spec.objects.append((tris, np.asarray([0, 0, 2, 2, 3, 3, 3, 3], dtype=np.uint16)))
    bent = {c: (MIRROR_BEND * np.sign(c[0] + 2.165), MIRROR_BEND * np.sign(c[1] + 0.15), -1.0) for c in corners}
    vn = np.zeros(tris.shape, dtype=np.float32)
    for t in (2, 3):
        for k in range(3):
            n = np.asarray(bent[tuple(mirror[t - 2][k])])
            vn[t, k] = n / np.linalg.norm(n)
    spec.normals = [vn]
    spec.area_lights = list(CHAIN_LIGHTS if lights is None else lights)
    return spec


def model_of(api, spec, W, H, area):
    """the float64 chain model of a scene (texture_ref.TextureModel, no textures) behind aov_lights_ref.LitModel"""
    import aov_lights_ref as AL
    import texture_ref as TX
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    normals = list(spec.normals) + [None] * (len(spec.objects) - len(spec.normals))
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, normals)])
    cam = api.Camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)[0]
    uv = np.full((len(verts), 3, 2), np.nan, dtype=np.float32)
    return AL.LitModel(TX.TextureModel(verts, recs["N"], mats, mo, cam, vn, uv, [], {}), area)


def host_area(api, spec):
    """Scene.debug_area_lights() of the scene's set, from a host-only context"""
    sc = api.Scene(8, 8, device=None)
    sc.set_area_lights(spec.area_lights)
    area = sc.debug_area_lights()
    sc.close()
    return area
