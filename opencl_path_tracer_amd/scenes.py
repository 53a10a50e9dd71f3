"""Synthetic scene DATA for the BASELINE configs.

No reference assets exist (its OBJ models live outside the repository, main.cpp:1002-1010),
so the scenes are generated here.  Coordinates and material parameters of the Cornell box
are the ones the reference's scene-authoring code lists (cited per item); everything else
is a deterministic generator.
"""
from dataclasses import dataclass, field

import numpy as np

# (kd, ks, emission, N, K, shininess, type) -- the ten built-in materials, main.cpp:753-762
LAMP, SUN, WHITE_DIFFUSE, RED_DIFFUSE, GREEN_DIFFUSE, PURPLE_SPECULAR, BLACK_SPECULAR, CHROMIUM, GOLD, GLASS = range(10)
BUILTIN_MATERIALS = [
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (60.0 * 2, 50.0 * 2, 40.0 * 2), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, 3),
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (60.0 * 5, 50.0 * 5, 40.0 * 5), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, 3),
    ((0.3, 0.3, 0.3), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 50.0, 0),
    ((0.3, 0.1, 0.1), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 50.0, 0),
    ((0.1, 0.3, 0.1), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 50.0, 0),
    ((0.3, 0.0, 0.0), (0.3, 0.3, 0.3), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 200.0, 0),
    ((0.05, 0.05, 0.05), (0.3, 0.3, 0.3), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 200.0, 0),
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (3.10, 3.05, 2.05), (3.3, 3.3, 2.9), 0.0, 1),
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.17, 0.35, 1.50), (3.1, 2.7, 1.9), 0.0, 1),
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.50, 1.50, 1.50), (0.0, 0.0, 0.0), 0.0, 2),
]


@dataclass
class SceneSpec:
    materials: list
    objects: list = field(default_factory=list)      # [(verts (n,3,3) f32, mati (n,) u16)] -- one end_Obj each
    fov: float = 60.0                                # the reference's "canonical" view, main.cpp:33-35,40
    yaw: float = 0.0
    pitch: float = 0.0
    shift: tuple = (0.0, 0.0, 0.0)
    name: str = ""
    normals: list = field(default_factory=list)      # optional, per object: vertex normals (n,3,3) f32 or None (Scene.load applies them)
    uvs: list = field(default_factory=list)          # optional, per object: corner uvs (n,3,2) f32 (NaN: none) or None
    textures: list = field(default_factory=list)     # optional: (h,w,3) f32 images, or (image, dict(filter=, srgb=)) (Scene.add_texture)
    material_textures: dict = field(default_factory=dict)   # optional: {index into materials: index into textures}
    lights: list = field(default_factory=list)       # optional: analytic lights as api.light_from takes them, dict(kind="point" | "spot" |
                                                     # "directional", ...) (Scene.load applies them with Scene.set_lights)
    lights_select: float = 0.5                       # ... and set_lights' select
    area_lights: list = field(default_factory=list)  # optional: sphere lights and suns as api.area_light_from takes them, dict(kind="sphere" |
                                                     # "sun", ...) (Scene.load applies them with Scene.set_area_lights)
    area_lights_select: float = 0.5                  # ... and set_area_lights' select
    medium: dict = field(default_factory=dict)       # optional: a homogeneous medium, Scene.set_medium's arguments: dict(sigma_t=, albedo=,
                                                     # g=, bounds=(lo, hi)) (Scene.load applies it)
    medium_density: object = None                    # optional: a voxel density for that medium, an array (nz, ny, nx) as
                                                     # Scene.set_medium_density takes it (Scene.load applies it after the medium)
    interiors: dict = field(default_factory=dict)    # optional: {index into materials: Scene.set_material_interior's arguments as a dict}, the
                                                     # medium inside a type-2 or type-6 material (Scene.load applies it)

    @property
    def ntris(self):
        return sum(v.shape[0] for v, _ in self.objects)


def _quad_tris(rows, mat):
    v = np.asarray(rows, dtype=np.float32).reshape(-1, 3, 3)
    return v, np.full(v.shape[0], mat, dtype=np.uint16)


def cornell_walls():
    """6 quads = 12 triangles, vertex order as listed in the reference."""
    rows, mats = [], []

    def tri(a, b, c, m):
        rows.append((a, b, c))
        mats.append(m)

    # lamp, main.cpp:765-766
    tri((300.0, 999.9, 700.0), (300.0, 999.9, 300.0), (700.0, 999.9, 700.0), LAMP)
    tri((700.0, 999.9, 700.0), (300.0, 999.9, 300.0), (700.0, 999.9, 300.0), LAMP)
    # far wall z=1000, main.cpp:794-795
    tri((-100.0, 0.0, 1000.0), (-100.0, 1000.0, 1000.0), (1100.0, 1000.0, 1000.0), WHITE_DIFFUSE)
    tri((1100.0, 1000.0, 1000.0), (1100.0, 0.0, 1000.0), (-100.0, 0.0, 1000.0), WHITE_DIFFUSE)
    # left wall x=-100, main.cpp:798-799
    tri((-100.0, 0.0, 1000.0), (-100.0, 0.0, -1000.0), (-100.0, 1000.0, 1000.0), RED_DIFFUSE)
    tri((-100.0, 1000.0, 1000.0), (-100.0, 0.0, -1000.0), (-100.0, 1000.0, -1000.0), RED_DIFFUSE)
    # right wall x=1100, main.cpp:802-803
    tri((1100.0, 1000.0, 1000.0), (1100.0, 0.0, -1000.0), (1100.0, 0.0, 1000.0), GREEN_DIFFUSE)
    tri((1100.0, 1000.0, -1000.0), (1100.0, 0.0, -1000.0), (1100.0, 1000.0, 1000.0), GREEN_DIFFUSE)
    # ceiling y=1000, main.cpp:806-807
    tri((-100.0, 1000.0, 1000.0), (-100.0, 1000.0, -1000.0), (1100.0, 1000.0, 1000.0), WHITE_DIFFUSE)
    tri((1100.0, 1000.0, 1000.0), (-100.0, 1000.0, -1000.0), (1100.0, 1000.0, -1000.0), WHITE_DIFFUSE)
    # floor y=0, main.cpp:814-815
    tri((-10000.0, 0.0, -10000.0), (-10000.0, 0.0, 10000.0), (10000.0, 0.0, 10000.0), WHITE_DIFFUSE)
    tri((10000.0, 0.0, 10000.0), (10000.0, 0.0, -10000.0), (-10000.0, 0.0, -10000.0), WHITE_DIFFUSE)
    return np.asarray(rows, dtype=np.float32), np.asarray(mats, dtype=np.uint16)


def uv_sphere(center, radius, segments=32, rings=16):
    """Tessellated sphere (the reference has no analytic sphere: prog.cl:18-21).
    segments*2 cap triangles + (rings-2)*segments*2 band triangles."""
    cx, cy, cz = center
    tris = []

    def p(i, j):
        th = np.pi * i / rings
        ph = 2.0 * np.pi * (j % segments) / segments
        return (cx + radius * np.sin(th) * np.cos(ph), cy + radius * np.cos(th), cz + radius * np.sin(th) * np.sin(ph))

    for j in range(segments):
        tris.append((p(0, 0), p(1, j + 1), p(1, j)))
    for i in range(1, rings - 1):
        for j in range(segments):
            a, b, c, d = p(i, j), p(i, j + 1), p(i + 1, j), p(i + 1, j + 1)
            tris.append((a, b, d))
            tris.append((a, d, c))
    for j in range(segments):
        tris.append((p(rings, 0), p(rings - 1, j), p(rings - 1, j + 1)))
    return np.asarray(tris, dtype=np.float64).astype(np.float32)


def uv_sphere_normals(center, radius, segments=32, rings=16):
    """The analytic normals (v - c) / r of uv_sphere's corners, (n, 3, 3) float32, for Scene.set_vertex_normals."""
    v = uv_sphere(center, radius, segments, rings).astype(np.float64)
    return ((v - np.asarray(center, dtype=np.float64)) / float(radius)).astype(np.float32)


def uv_sphere_uvs(rings=16, segments=32):
    """The lat-long uvs of uv_sphere's corners in its triangle order, (n, 3, 2) float32, for Scene.set_vertex_uvs: u = j / segments
    around the axis (1 at the seam's far side, the middle of its segment at a pole), v = 1 - i / rings (1 at the +y pole)."""
    tris = []

    def q(i, j):
        return (j / segments, 1.0 - i / rings)

    for j in range(segments):
        tris.append((((j + 0.5) / segments, 1.0), q(1, j + 1), q(1, j)))
    for i in range(1, rings - 1):
        for j in range(segments):
            a, b, c, d = q(i, j), q(i, j + 1), q(i + 1, j), q(i + 1, j + 1)
            tris.append((a, b, d))
            tris.append((a, d, c))
    for j in range(segments):
        tris.append((((j + 0.5) / segments, 0.0), q(rings - 1, j), q(rings - 1, j + 1)))
    return np.asarray(tris, dtype=np.float64).astype(np.float32)


def checker_texture(n, a, b):
    """An n x n checkerboard (n, n, 3) float32 for Scene.add_texture: colour a where row + column is even, b elsewhere."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    even = ((i + j) % 2 == 0)[:, :, None]
    return np.where(even, np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)).astype(np.float32)


LAMP_LIGHT_Y = 990.0           # cornell_box(lamp="point" / "spot"): the light hangs this high, under the ceiling at 1000
LAMP_SPOT_DEGREES = (60.0, 90.0)      # ... and the spot's inner and outer half angles
LAMP_SPHERE_RADIUS = 60.0      # cornell_box(lamp="sphere"): the sphere light's radius; it hangs 10 under the ceiling


CORNELL_ROOM = ((-100.0, 0.0, -1000.0), (1100.0, 1000.0, 1000.0))      # cornell_box(fog=...): the fog's box, the room wall to wall


def smoke_plume(n=32):
    """A procedural density (n, n, n) float32 for Scene.set_medium_density, index (k, j, i) = (z, y, x) with y up: a plume that rises
    from the middle of the floor of the medium's box, widens and thins with height and sways along x, over a thin ground mist.
    Densities lie in [0, 4]; outside the plume and above the mist they are exactly 0 (empty voxels the walk crosses for free)."""
    c = (np.arange(n, dtype=np.float64) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    cx = 0.5 + 0.12 * np.sin(7.0 * y) * y                       # the axis sways with height
    cz = 0.5 + 0.08 * np.sin(5.0 * y + 1.0) * y
    radius = 0.06 + 0.22 * y                                    # and the plume widens
    r2 = ((x - cx) ** 2 + (z - cz) ** 2) / (radius * radius)
    puff = 0.75 + 0.25 * np.sin(19.0 * x + 3.0 * y) * np.sin(17.0 * z - 5.0 * y) * np.sin(23.0 * y)
    plume = np.where(r2 < 1.0, 4.0 * (1.0 - r2) * (1.0 - 0.7 * y) * puff, 0.0)
    mist = np.where(y < 0.1, 0.5 * (1.0 - y / 0.1), 0.0)
    return np.maximum(plume, mist).astype(np.float32)


def cornell_box(segments=32, rings=16, smooth=False, textured=False, glossy=False, coated=False, frosted=False, lamp="quad", fog=0.0, density=None, tint=None, wax=0.0):
    """Scene CB of SURVEY 8(d): 12 wall/lamp triangles + two tessellated spheres
    (radius 200; CHROMIUM at (250,200,300), GLASS at (750,200,-200)), 3 objects.
    smooth: the spheres carry their analytic vertex normals (shaded with them under option smooth_normals).
    textured: the floor carries uvs (one repeat per 1,600 units) and WHITE_DIFFUSE an 8 x 8 checker with nearest filtering, so under
    option textures the floor shows checks of 200 units; the other white walls have no uvs and keep their kd.
    glossy: the chromium sphere gets a copy of its material with type 4 and shininess 50, appended to the materials: a rough metal under
    option glossy (and inert without it).
    coated: the other sphere gets, in place of GLASS, a red plastic appended to the materials: type 5, kd (0.7, 0.1, 0.1), N = 1.5 and
    K = 0 (F0 = 0.04), shininess 300; a diffuse base under a rough dielectric coat under option coated (and inert without it).
    frosted: the other sphere gets, in place of GLASS, a copy of GLASS with type 6 and shininess 30, appended to the materials: a rough
    dielectric (frosted glass) under option frosted (and inert without it).  The sphere wears one material: not together with coated.
    lamp: "quad" (default) the reference's emitting quad; "point" / "spot" remove it and hang an analytic light of the same total power
    below its centre (Scene.set_lights through Scene.load; only render_nee renders the scene then).  The quad of area A and emission E
    radiates pi E A; a point light of intensity I radiates 4 pi I, so I = E A / 4; the spot points down, full inside 60 degrees of its
    axis and dark from 90 on, and the smoothstep between integrates to half its width: 2 pi I (1 - cos 60 + cos 60 / 2), so
    I = E A / 1.5.  "sphere" removes the quad too and hangs a sphere light (Scene.set_area_lights through Scene.load) of radius
    LAMP_SPHERE_RADIUS and the same total power under its centre: a sphere of radiance L radiates 4 pi^2 R^2 L, so L = E A / (4 pi R^2).
    It casts soft shadows and is seen by the camera and in the chromium sphere.
    fog: sigma_t > 0 fills the room (CORNELL_ROOM) with a white medium of that extinction per unit, albedo 0.9 and g = 0.6
    (Scene.set_medium through Scene.load; only render_nee renders the scene then).  1e-3 is a mean free path of the room's width.
    density: with fog, a voxel density (nz, ny, nx) over the room, such as smoke_plume(): the extinction is fog x density
    (Scene.set_medium_density through Scene.load).
    tint, wax: the glass sphere (GLASS, or its frosted copy) gets an interior (Scene.set_material_interior through Scene.load; only render_nee
    renders the scene then).  tint: the colour (rgb in (0, 1]) white light has left after crossing the sphere's diameter, 400 units:
    sigma_a = -ln(tint) / 400.  wax > 0: grey scattering with that many mean free paths per diameter, sigma_s = wax / 400, and g = 0.8.
    Not together with coated, whose plastic has no inside."""
    if (tint is not None or wax > 0.0) and coated:
        raise ValueError("cornell_box: tint and wax fill the glass sphere, which coated replaces with an opaque plastic")
    if coated and frosted:
        raise ValueError("cornell_box: coated and frosted both replace the glass sphere's material")
    if lamp not in ("quad", "point", "spot", "sphere"):
        raise ValueError("cornell_box: lamp must be \"quad\", \"point\", \"spot\" or \"sphere\"")
    spec = SceneSpec(materials=list(BUILTIN_MATERIALS), name="cornell_box")
    walls, wall_mats = cornell_walls()
    if lamp != "quad":
        quad = walls[:2].astype(np.float64)                  # the lamp's two triangles come first
        area = 0.5 * sum(np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) for t in quad)
        centre = quad.reshape(-1, 3).mean(axis=0)
        emission = np.asarray(BUILTIN_MATERIALS[LAMP][2], dtype=np.float64)
        position = (float(centre[0]), LAMP_LIGHT_Y, float(centre[2]))
        if lamp == "sphere":
            R = LAMP_SPHERE_RADIUS
            spec.area_lights = [dict(kind="sphere", center=(float(centre[0]), 1000.0 - 10.0 - R, float(centre[2])), radius=R,
                                     radiance=tuple(emission * area / (4.0 * np.pi * R * R)))]
        elif lamp == "point":
            spec.lights = [dict(kind="point", position=position, intensity=tuple(emission * area / 4.0))]
        else:
            spec.lights = [dict(kind="spot", position=position, direction=(0.0, -1.0, 0.0), intensity=tuple(emission * area / 1.5),
                                inner_degrees=LAMP_SPOT_DEGREES[0], outer_degrees=LAMP_SPOT_DEGREES[1])]
        walls, wall_mats = walls[2:], wall_mats[2:]
    spec.objects.append((walls, wall_mats))
    s1 = uv_sphere((250.0, 200.0, 300.0), 200.0, segments, rings)
    chromium = CHROMIUM
    if glossy:
        spec.materials.append(tuple(BUILTIN_MATERIALS[CHROMIUM][:5]) + (50.0, 4))
        chromium = len(spec.materials) - 1
    spec.objects.append((s1, np.full(s1.shape[0], chromium, dtype=np.uint16)))
    s2 = uv_sphere((750.0, 200.0, -200.0), 200.0, segments, rings)
    glass = GLASS
    if coated:
        spec.materials.append(((0.7, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (1.5, 1.5, 1.5), (0, 0, 0), 300.0, 5))
        glass = len(spec.materials) - 1
    if frosted:
        spec.materials.append(tuple(BUILTIN_MATERIALS[GLASS][:5]) + (30.0, 6))
        glass = len(spec.materials) - 1
    spec.objects.append((s2, np.full(s2.shape[0], glass, dtype=np.uint16)))
    if smooth:
        spec.normals = [None, uv_sphere_normals((250.0, 200.0, 300.0), 200.0, segments, rings),
                        uv_sphere_normals((750.0, 200.0, -200.0), 200.0, segments, rings)]
    if textured:
        walls = spec.objects[0][0]
        uv = np.full((walls.shape[0], 3, 2), np.nan, dtype=np.float32)
        uv[-2:] = walls[-2:][:, :, [0, 2]] / np.float32(1600.0)            # the floor, the last two wall triangles: (x, z)
        spec.uvs = [uv, None, None]
        spec.textures = [(checker_texture(8, (1.0, 1.0, 1.0), (0.25, 0.25, 0.25)), dict(filter=0, srgb=0))]
        spec.material_textures = {WHITE_DIFFUSE: 0}
    if fog > 0.0:
        spec.medium = dict(sigma_t=float(fog), albedo=(0.9, 0.9, 0.9), g=0.6, bounds=CORNELL_ROOM)
        if density is not None:
            spec.medium_density = np.ascontiguousarray(density, dtype=np.float32)
    elif density is not None:
        raise ValueError("cornell_box: density needs fog > 0 (the medium whose extinction it scales)")
    if tint is not None or wax > 0.0:
        c = np.ones(3) if tint is None else np.asarray(tint, dtype=np.float64).reshape(3)
        if not (np.all(c > 0.0) and np.all(c <= 1.0)):
            raise ValueError("cornell_box: tint must lie in (0, 1] per channel")
        spec.interiors = {glass: dict(sigma_a=tuple(float(v) for v in (-np.log(c) / 400.0 + 0.0)), sigma_s=float(wax) / 400.0,
                                      g=0.8 if wax > 0.0 else 0.0)}
    return spec


def light_shaft(sigma_t=0.12):
    """The beam picture for Scene.set_medium: a dark closed room (x in [-6, 6], y in [-3, 5], z in [-1, 14]) with grey walls, seen from the
    origin along +z; a spot light under the ceiling at the back left shines down and to the right through a slot (1.2 wide along x, 5
    deep along z) in a black occluder at y = 3, and bounded fog (albedo 0.95, g = 0.7, the room's own box) makes the shaft visible between
    the slot and the lit patch on the floor.  No emitter and no sky: only the spot lights the scene (Scene.set_lights through
    Scene.load), and only render_nee renders it."""
    mats = [
        ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 0 walls
        ((0.02, 0.02, 0.02), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),          # 1 the occluder
    ]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    x0, x1, y0, y1, z0, z1 = -6.0, 6.0, -3.0, 5.0, -1.0, 14.0
    tris, mo = [], []
    for q, m in ((quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), 0),      # floor
                 (quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)), 0),      # ceiling
                 (quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), 0),      # back
                 (quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), 0),      # left
                 (quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)), 0),      # right
                 (quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), 0)):     # behind the camera
        tris += q
        mo += [m] * len(q)
    sx0, sx1, sz0, sz1, oy = -2.6, -1.4, 6.0, 11.0, 3.0                                   # the slot in the occluder
    for q in (quad((x0, oy, z0), (sx0, oy, z0), (sx0, oy, z1), (x0, oy, z1)), quad((sx1, oy, z0), (x1, oy, z0), (x1, oy, z1), (sx1, oy, z1)),
              quad((sx0, oy, z0), (sx1, oy, z0), (sx1, oy, sz0), (sx0, oy, sz0)), quad((sx0, oy, sz1), (sx1, oy, sz1), (sx1, oy, z1), (sx0, oy, z1))):
        tris += q
        mo += [1] * len(q)
    spec = SceneSpec(materials=mats, name="light_shaft", shift=(-500.0, -500.0, 1299.0378))
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    spec.lights = [dict(kind="spot", position=(-3.2, 4.8, 8.5), direction=(0.45, -1.0, 0.0), intensity=(900.0, 850.0, 700.0),
                        inner_degrees=25.0, outer_degrees=40.0)]
    spec.medium = dict(sigma_t=float(sigma_t), albedo=(0.95, 0.95, 0.95), g=0.7, bounds=((x0, y0, z0), (x1, y1, z1)))
    return spec


def many_lights(n=16, spacing=3.0, lamp=0.4):
    """The many-emitter scene for option light_tree: a closed diffuse corridor (x in [-2, 2], y in [-1.5, 1.5], z in [-1, spacing n + 2]) seen
    from the origin along +z, with n square lamps of side `lamp` (two triangles each) just under its ceiling, `spacing` apart along z and
    alternating between x = -0.8 and x = 0.8.  Even lamps emit (20, 18, 15), odd ones a quarter of that.  Lamp n // 2 lies a unit below the
    floor instead, where nothing sees it: a light the table holds and every floor point's horizon culls.  The lamps come first, lamp i being
    triangles 2 i and 2 i + 1, in one object with the walls.  n >= 2."""
    if n < 2:
        raise ValueError("many_lights: n must be >= 2")
    mats = [
        ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 0 walls
        ((0, 0, 0), (0, 0, 0), (20.0, 18.0, 15.0), (0, 0, 0), (0, 0, 0), 0.0, 3),          # 1 bright lamps
        ((0, 0, 0), (0, 0, 0), (5.0, 4.5, 3.75), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 2 dim lamps
    ]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, -1.5, 1.5, -1.0, float(spacing) * n + 2.0
    tris, mo = [], []
    h = 0.5 * float(lamp)
    for i in range(n):
        cx, cz = (-0.8 if i % 2 == 0 else 0.8), 1.5 + float(spacing) * i
        cy = y0 - 1.0 if i == n // 2 else y1 - 0.05
        tris += quad((cx - h, cy, cz - h), (cx + h, cy, cz - h), (cx + h, cy, cz + h), (cx - h, cy, cz + h))
        mo += [1 + i % 2] * 2
    for q in (quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)),      # floor
              quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),      # ceiling
              quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)),      # far end
              quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)),      # left
              quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),      # right
              quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0))):     # behind the camera
        tris += q
        mo += [0] * len(q)
    spec = SceneSpec(materials=mats, name="many_lights_%d" % n, shift=(-500.0, -500.0, 1299.0378))
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    return spec


FOCUS_ROW_SPHERES = [((-2.4, -1.1, 5.0), 0), ((-0.8, -1.1, 8.0), 4), ((0.8, -1.1, 12.0), 5), ((2.4, -1.1, 17.0), 6)]


def focus_row(segments=8, rings=4):
    """A depth-of-field scene for Scene.set_lens: a grey floor (y = -2) under an area light (y = 6), seen from the origin along +z, and on
    it a diagonal row of four spheres of radius 0.9 at depths 5, 8, 12 and 17: a red type-0 one with a specular lobe, a glass one, a
    rough-gold type-4 one (option glossy) and a blue type-5 plastic one (option coated), each with its analytic vertex normals (option
    smooth_normals).  Nothing closes the scene, so a sky set with Scene.set_environment is seen above the floor."""
    gold = BUILTIN_MATERIALS[GOLD]
    mats = [
        ((0.6, 0.1, 0.1), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 red, specular lobe
        ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 floor
        ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),             # 2 lamp
        ((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 0.0, 0),                   # 3 (spare: black)
        BUILTIN_MATERIALS[GLASS],                                                            # 4 glass
        tuple(gold[:5]) + (50.0, 4),                                                         # 5 rough gold
        ((0.1, 0.2, 0.6), (0, 0, 0), (0, 0, 0), (1.5, 1.5, 1.5), (0, 0, 0), 20.0, 5),      # 6 blue plastic
    ]
    spec = SceneSpec(materials=mats, name="focus_row", shift=(-500.0, -500.0, 1299.0378))
    x0, x1, z0, z1 = -8.0, 8.0, 0.5, 30.0
    tris = [((x0, -2.0, z0), (x1, -2.0, z0), (x1, -2.0, z1)), ((x0, -2.0, z0), (x1, -2.0, z1), (x0, -2.0, z1)),
            ((-3.0, 6.0, 4.0), (3.0, 6.0, 4.0), (3.0, 6.0, 16.0)), ((-3.0, 6.0, 4.0), (3.0, 6.0, 16.0), (-3.0, 6.0, 16.0))]
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray([1, 1, 2, 2], dtype=np.uint16)))
    spec.normals = [None]
    for c, m in FOCUS_ROW_SPHERES:
        v = uv_sphere(c, 0.9, segments, rings)
        spec.objects.append((v, np.full(len(v), m, dtype=np.uint16)))
        spec.normals.append(uv_sphere_normals(c, 0.9, segments, rings))
    return spec


def sun_and_sky(width=64, height=32, sun_dir=(0.3, 0.8, 0.5), sun_radius_deg=5.0, sun_radiance=(400.0, 360.0, 300.0),
                zenith=(0.25, 0.45, 0.9), horizon=(0.8, 0.85, 0.9), ground=(0.1, 0.09, 0.08)):
    """A procedural lat-long map (height, width, 3) float32 for Scene.set_environment, row 0 at the +y pole: a sky that fades from
    `zenith` to `horizon`, a dim `ground` below it, and a sun disc of angular radius sun_radius_deg and radiance sun_radiance around
    sun_dir (texel centres inside the disc; at least the one nearest to sun_dir)."""
    th = (np.arange(height) + 0.5) * np.pi / height
    ph = (np.arange(width) + 0.5) * 2.0 * np.pi / width
    d = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(width)), np.outer(np.sin(th), np.sin(ph))], axis=-1)
    up = np.clip(d[..., 1], 0.0, 1.0)[..., None]
    img = np.where(d[..., 1:2] >= 0.0, np.asarray(horizon) * (1.0 - up) + np.asarray(zenith) * up, np.asarray(ground))
    s = np.asarray(sun_dir, dtype=np.float64)
    cosang = d @ (s / np.linalg.norm(s))
    disc = cosang >= np.cos(np.radians(sun_radius_deg))
    disc.flat[int(np.argmax(cosang))] = True
    img[disc] = np.asarray(sun_radiance)
    return img.astype(np.float32)


def sun_and_sky_light(sun_dir=(0.3, 0.8, 0.5), sun_radius_deg=5.0, sun_radiance=(400.0, 360.0, 300.0), **kw):
    """(map, sun): sun_and_sky's map with the same arguments, and the description of the sun light that matches its disc, as
    api.area_light_from and SceneSpec.area_lights take it: the light travels along -sun_dir, with the disc's angular diameter and radiance.
    The map still holds its disc: set either the map or the light as the scene's sun, since a frame lit by both counts it twice."""
    img = sun_and_sky(sun_dir=sun_dir, sun_radius_deg=sun_radius_deg, sun_radiance=sun_radiance, **kw)
    s = np.asarray(sun_dir, dtype=np.float64)
    sun = dict(kind="sun", direction=tuple(float(-v) for v in s), angular_diameter_degrees=2.0 * float(sun_radius_deg),
               radiance=tuple(float(v) for v in sun_radiance))
    return img, sun


def _lcg_floats(n, seed=1):
    """minstd (48271) stream mapped to [0,1): deterministic displacement noise."""
    out = np.empty(n, dtype=np.float64)
    x = seed
    for i in range(n):
        x = (x * 48271) % 2147483647
        out[i] = x / 2147483647.0
    return out


def displaced_grid_mesh(ntris_target, seed=1):
    """MESH-100k / MESH-1M of SURVEY 8(d): CB walls + one displaced height-field grid inside
    the box, material bands WHITE/CHROMIUM/GLASS by face index."""
    n = int(np.ceil(np.sqrt(ntris_target / 2.0)))
    xs = np.linspace(0.0, 1000.0, n + 1)
    zs = np.linspace(-600.0, 800.0, n + 1)
    rng = np.random.RandomState(seed)           # deterministic; numpy's MT19937 is stable across versions
    h = rng.rand(n + 1, n + 1)
    gx, gz = np.meshgrid(xs, zs, indexing="ij")
    gy = 80.0 + 120.0 * (np.sin(gx / 97.0) * np.cos(gz / 131.0) + 1.0) + 25.0 * h
    P = np.stack([gx, gy, gz], axis=-1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[:-1, 1:], P[1:, 1:]
    t1 = np.stack([a, c, d], axis=2).reshape(-1, 3, 3)
    t2 = np.stack([a, d, b], axis=2).reshape(-1, 3, 3)
    verts = np.empty((t1.shape[0] * 2, 3, 3), dtype=np.float32)
    verts[0::2] = t1
    verts[1::2] = t2
    nt = verts.shape[0]
    band = (np.arange(nt) * 3) // nt
    mati = np.choose(band, [WHITE_DIFFUSE, CHROMIUM, GLASS]).astype(np.uint16)
    spec = SceneSpec(materials=list(BUILTIN_MATERIALS), name="mesh_%d" % nt)
    spec.objects.append(cornell_walls())
    spec.objects.append((verts, mati))
    return spec


# ------------------------------------------------------------------------------------------------
# MESH-* as files: SURVEY 8(d) specifies the mesh configs "written as OBJ+MTL with Kd/Ks/Ke/Ns/Kn/Kk/Tp
# and loaded through the build's loader with add_Obj semantics" (main.cpp:552-617).
def _mtl_block(name, m):
    kd, ks, ke, N, K, shininess, mtype = m
    return ("newmtl %s\nKd %r %r %r\nKs %r %r %r\nKe %r %r %r\nNs %r\nKn %r %r %r\nKk %r %r %r\nTp %d\n\n" %
            ((name,) + tuple(float(x) for x in kd) + tuple(float(x) for x in ks) + tuple(float(x) for x in ke) + (float(shininess),) +
             tuple(float(x) for x in N) + tuple(float(x) for x in K) + (int(mtype),)))


def write_grid_mesh_obj(ntris_target, directory, pos=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0), pitch=0.0, yaw=0.0, name=None, seed=1):
    """The height field of displaced_grid_mesh() as <name>.obj + <name>.mtl with SHARED vertices, one shape,
    three `usemtl` bands (WHITE_DIFFUSE, CHROMIUM, GLASS).  The file holds the coordinates add_Obj's
    transform (negate x, rotate_x(pitch), rotate_y(yaw), * scale + pos: main.cpp:598-606) maps back onto the
    height field -- up to rounding: what the loader must reproduce bit for bit is ITS OWN arithmetic on the
    file's numbers, which the tests restate with the oracle.  Returns (obj_path, vertices (nv,3) f32 as
    written, faces (nt,3) int vertex indices, material index per face relative to the file's materials)."""
    import os
    spec = displaced_grid_mesh(ntris_target, seed)
    verts = spec.objects[1][0].astype(np.float64)                 # (nt, 3, 3) world coordinates
    nt = verts.shape[0]
    flat = verts.reshape(-1, 3)
    uniq, inv = np.unique(flat, axis=0, return_inverse=True)
    faces = inv.reshape(nt, 3)
    # inverse of the loader's transform, in double
    w = (uniq - np.asarray(pos, np.float64)) / np.asarray(scale, np.float64)
    b = np.float64(np.float32(yaw) / np.float32(180.0) * np.float32(3.141593))
    g = np.float64(np.float32(pitch) / np.float32(180.0) * np.float32(3.141593))
    x0 = w[:, 0] * np.cos(b) - w[:, 2] * np.sin(b)                # rotate_y(-yaw)
    z0 = w[:, 0] * np.sin(b) + w[:, 2] * np.cos(b)
    y1 = w[:, 1] * np.cos(g) + z0 * np.sin(g)                     # rotate_x(-pitch)
    z1 = -w[:, 1] * np.sin(g) + z0 * np.cos(g)
    local = np.stack([-x0, y1, z1], 1).astype(np.float32)
    name = name or ("mesh_%d" % nt)
    band_mats = [WHITE_DIFFUSE, CHROMIUM, GLASS]
    band = (np.arange(nt) * 3) // nt
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, name + ".mtl"), "w") as f:
        for k, mi in enumerate(band_mats):
            f.write(_mtl_block("band%d" % k, BUILTIN_MATERIALS[mi]))
    path = os.path.join(directory, name + ".obj")
    with open(path, "w") as f:
        f.write("# displaced grid, %d triangles, %d vertices\nmtllib %s.mtl\no %s\n" % (nt, local.shape[0], name, name))
        f.write("".join("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])) for v in local))
        for k in range(3):
            f.write("usemtl band%d\n" % k)
            sel = faces[band == k] + 1
            f.write("".join("f %d %d %d\n" % (a, b_, c) for a, b_, c in sel))
    return path, local, faces, band.astype(np.uint16)
