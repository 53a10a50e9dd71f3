"""Test helper: small and degenerate scenes for the device BVH builders (pt_lbvh.hip, pt_sahdev.hip, pt_widedev.hip), the
case table of test_builder_scenes_host.py / test_gpu_device_builders.py, and their fixed ray sets.  Scene data only; imports
without a device.

Every generator returns a scenes.SceneSpec with the built-in materials, `n` triangles that end up in the TREE (two of them
emit, so a render is not black) and, for some geometries, further triangles that must end up in the big-triangle list or
nowhere (non-finite ones).  The sizes sit on either side of what the builders' kernels are organised by: 2 * kMaxLeaf = 8
(the largest scene build_on_device leaves to the host), a 64-lane wave, a 256-thread block, two blocks, and 1,024 (four
blocks; PLOC's tile of 256 + 2R positions is crossed from 257 on).

The column `sah` / `lbvh` of a case says where the tree must end up being built when the device is asked (bvh_policy 5 / 2 / 3
with bvh_device 1, and bvh_policy 4): 1 on the device, 0 handed back to the host.  It is written down here and checked against
the HOST builder alone (test_builder_scenes_host.py::test_expected_column_follows_from_the_host_builder):
    0  when n <= 8 (pt_builder.cpp build_on_device: ns <= 2 * kMaxLeaf),
    0  when a coordinate is not finite (stage_upload counts them; the host path keeps such triangles out of the tree),
    0  for the SAH policies when the host builder itself split a range at the median (stat "bvh_median_splits": coincident
       centroids have no order the device could reproduce, pt_sahdev.hip eval_split -> `unsupported`),
    1  otherwise.  (The LBVH's only further hand-back, depth + 5 > kStackEntries, is hit by no case here.)"""
from dataclasses import dataclass

import numpy as np

from opencl_path_tracer_amd import scenes

RAY = np.dtype([("P", "<f4", 4), ("D", "<f4", 4)])
SIZES = (8, 9, 10, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025)
EYE = np.array([500.0, 500.0, -1299.037842], dtype=np.float64)        # the default camera's eye (test_closest_hit_unit_level)
SAH_POLICIES = (5, 2, 3)                                                # (5: policy 0's tree, on the device)
N_RAYS = 2048

_TREE_MATS = np.array([scenes.WHITE_DIFFUSE, scenes.RED_DIFFUSE, scenes.GREEN_DIFFUSE, scenes.CHROMIUM, scenes.GLASS, scenes.PURPLE_SPECULAR],
                      dtype=np.uint16)


def _mats(n, rng):
    """materials of n tree triangles: the first two emit, the others are a mix of diffuse, mirror and glass"""
    m = _TREE_MATS[rng.randint(0, len(_TREE_MATS), n)]
    m[:2] = scenes.LAMP
    return m


def _unit(rng, shape):
    d = rng.normal(size=shape + (3,))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _soup_verts(n, rng, lo=(150.0, 150.0, -300.0), hi=(850.0, 850.0, 700.0), size=None):
    """n random triangles: centres uniform in [lo, hi], corners `size` (within one octave) away from the centre; by default the
    size shrinks with n so that the triangles cover about the same part of the view (and none is 1/16 of the others' box from 63 on)"""
    if size is None:
        s0 = min(80.0, 250.0 / np.sqrt(n))
        size = (s0, 2.0 * s0)
    c = rng.uniform(lo, hi, (n, 1, 3))
    r = rng.uniform(size[0], size[1], (n, 3, 1))
    return (c + _unit(rng, (n, 3)) * r).astype(np.float32)


NARROW_FOV = 25.0        # the soups fill the frame of the default eye at this field of view (the default 60 shows the whole room)


def _spec(name, objects, **kw):
    return scenes.SceneSpec(materials=list(scenes.BUILTIN_MATERIALS), objects=objects, name=name, **kw)


def soup(n, seed):
    rng = np.random.RandomState(seed)
    return _spec("soup_%d" % n, [(_soup_verts(n, rng), _mats(n, rng))], fov=NARROW_FOV)


def walls_soup(n, seed):
    """the Cornell walls (all twelve are listed: the soup is compact, so each wall is bigger than 1/16 of its box) in front of a small tree"""
    rng = np.random.RandomState(seed)
    v = _soup_verts(n, rng, lo=(350.0, 250.0, 50.0), hi=(650.0, 550.0, 350.0), size=(10.0, 20.0))
    return _spec("walls_soup_%d" % n, [scenes.cornell_walls(), (v, _mats(n, rng))])


def zero_area(n, seed):
    """soup in which every third triangle is degenerate, the three kinds of test_degenerate_triangles in turn: two equal corners,
    three collinear corners, a needle 1e-4 wide"""
    rng = np.random.RandomState(seed)
    v = _soup_verts(n, rng)
    for k, i in enumerate(range(2, n, 3)):
        a, b = v[i, 0].astype(np.float64), v[i, 2].astype(np.float64)
        v[i, 1] = (a, (a + b) / 2, a + 1e-4)[k % 3]
    return _spec("zero_area_%d" % n, [(v, _mats(n, rng))], fov=NARROW_FOV)


def planar(n, seed):
    """a regular grid in the plane y = 0 (the boxes' pads are symmetric about it: every box centre has y == 0 exactly)"""
    rng = np.random.RandomState(seed)
    g = int(np.ceil(np.sqrt(n / 2.0)))
    xs, zs = np.linspace(200.0, 800.0, g + 1), np.linspace(-200.0, 900.0, g + 1)
    gx, gz = np.meshgrid(xs, zs, indexing="ij")
    P = np.stack([gx, np.zeros_like(gx), gz], axis=-1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[:-1, 1:], P[1:, 1:]
    v = np.empty((2 * g * g, 3, 3), dtype=np.float32)
    v[0::2] = np.stack([a, c, d], axis=2).reshape(-1, 3, 3)
    v[1::2] = np.stack([a, d, b], axis=2).reshape(-1, 3, 3)
    return _spec("planar_%d" % n, [(v[:n].copy(), _mats(n, rng))])


def line(n, seed):
    """triangles in the plane y = 0, each symmetric about the line x = 0: box centres differ along z only"""
    rng = np.random.RandomState(seed)
    z = np.linspace(0.0, 2000.0, n)
    w = rng.randint(60, 121, n).astype(np.float64)
    d = rng.randint(30, 61, n).astype(np.float64)
    zero = np.zeros(n)
    v = np.stack([np.stack([-w, zero, z], -1), np.stack([w, zero, z], -1), np.stack([zero, zero, z + d], -1)], axis=1).astype(np.float32)
    return _spec("line_%d" % n, [(v, _mats(n, rng))])


CONCENTRIC_LISTED = 16                                   # option flat_list's default
CONCENTRIC_SHIFT = (-500.0, -500.0, 999.0378)            # the eye at (0, 0, -300): the triangles surround the origin


def concentric(n, seed):
    """n + 16 triangles of different sizes and orientations whose boxes are all centred on the origin, exactly: two corners are
    opposite corners of the box (integers: -a and +a pad to -x and +x), the third lies inside it.  Half extents within
    [30, 60]: any box is more than 1/16 of the box around all the others, so the 16 biggest (option flat_list's default) are listed and n stay in the tree.
    Objects of six: the reference's own mean split never has to separate them (pt_end_obj)."""
    rng = np.random.RandomState(seed)
    m = n + CONCENTRIC_LISTED
    h = rng.randint(30, 61, (m, 3)).astype(np.float64)
    s = rng.choice([-1.0, 1.0], (m, 3))
    inner = rng.uniform(-0.9, 0.9, (m, 3)) * h
    v = np.stack([-s * h, s * h, inner], axis=1).astype(np.float32)
    mats = _mats(m, rng)
    return _spec("concentric_%d" % n, [(v[i:i + 6], mats[i:i + 6]) for i in range(0, m, 6)], shift=CONCENTRIC_SHIFT)


def duplicates(n, seed):
    """soup in which every triangle appears twice in a row, bit for bit (an odd n: the last one once)"""
    rng = np.random.RandomState(seed)
    h = (n + 1) // 2
    v, m = _soup_verts(h, rng), _mats(h, rng)
    return _spec("duplicates_%d" % n, [(np.repeat(v, 2, axis=0)[:n].copy(), np.repeat(m, 2)[:n].copy())], fov=NARROW_FOV)


CLUSTERS = ((500.0, 500.0, -1100.0), (8500.0, 4500.0, 300000.0))      # diameter 30 each, 1e4 diameters apart; the near one fills a few pixels


def clustered(n, seed):
    """two clusters of diameter 30, a factor of 1e4 apart: inside a cluster (almost) all Morton codes are equal"""
    rng = np.random.RandomState(seed)
    c = np.asarray(CLUSTERS)[np.arange(n) % 2][:, None, :] + rng.uniform(-15.0, 15.0, (n, 1, 3))
    v = (c + _unit(rng, (n, 3)) * rng.uniform(3.0, 6.0, (n, 3, 1))).astype(np.float32)
    return _spec("clustered_%d" % n, [(v, _mats(n, rng))], fov=10.0)


def huge(n, seed):
    """soup plus, in an object of their own, one triangle near 1e30 and one near 3e38: finite, but the sum of a box's planes and its
    area overflow.  Both areas are +inf, so both are listed (select_flat_list) and the tree holds the soup."""
    rng = np.random.RandomState(seed)
    v = _soup_verts(n, rng)
    big = (np.array([1e30, 3e38])[:, None, None] * rng.uniform(0.9, 1.1, (2, 3, 3))).astype(np.float32)
    return _spec("huge_%d" % n, [(v, _mats(n, rng)), (big, np.full(2, scenes.WHITE_DIFFUSE, dtype=np.uint16))], fov=NARROW_FOV)


def huge_tree(n, seed):
    """the same pair behind a soup of n - 2, for contexts with option flat_list 0: nothing is listed, so the pair stays in the tree and
    every builder meets a centroid sum and a box area that overflow (the host builder answers with median splits)"""
    spec = huge(n - 2, seed)
    spec.name = "huge_tree_%d" % n
    return spec


def nonfinite(n, seed):
    """soup plus, in an object of their own, three triangles with one inf, one -inf and one NaN coordinate: they can never be hit and
    are in no tree and no list"""
    rng = np.random.RandomState(seed)
    v = _soup_verts(n, rng)
    bad = rng.uniform(100.0, 900.0, (3, 3, 3)).astype(np.float32)
    for k, x in enumerate((np.inf, -np.inf, np.nan)):
        bad[k, rng.randint(3), rng.randint(3)] = x
    return _spec("nonfinite_%d" % n, [(v, _mats(n, rng)), (bad, np.full(3, scenes.WHITE_DIFFUSE, dtype=np.uint16))], fov=NARROW_FOV)


GENERATORS = {"soup": soup, "walls_soup": walls_soup, "zero_area": zero_area, "planar": planar, "line": line, "concentric": concentric,
              "duplicates": duplicates, "clustered": clustered, "huge": huge, "huge_tree": huge_tree, "nonfinite": nonfinite}


@dataclass(frozen=True)
class Case:
    geometry: str
    n: int               # triangles in the tree
    listed: int          # triangles in the big-triangle list
    dropped: int         # non-finite triangles (in neither)
    sah: int             # bvh_policy 5 / 2 / 3 with bvh_device 1: 1 built on the device, 0 handed back
    lbvh: int            # bvh_policy 4: the same
    zero_axes: tuple = ()    # axes on which all box centres are equal
    flat_list: int = -1      # option flat_list of every context of the case (-1: see options)

    @property
    def id(self):
        return "%s-%d" % (self.geometry, self.n)

    def spec(self):
        return GENERATORS[self.geometry](self.n, 1000 + self.n)

    def expected(self, policy):
        return self.lbvh if policy == 4 else self.sah

    @property
    def options(self):
        """Options every context of the case gets in front of the scene.  select_flat_list lists the m biggest triangles when each
        is at least 1/16 of the box around all the OTHERS -- so a scene of at most flat_list (16) triangles is listed whole (there
        are no others), and 17 triangles leave one.  Below 63 tree triangles the option is therefore set to the list the case
        intends; from 63 on the default gives exactly that list."""
        if self.flat_list >= 0:
            return {"flat_list": self.flat_list}
        return {"flat_list": self.listed} if self.n < 63 else {}

    def configure(self, sc):
        for k, v in self.options.items():
            sc.set_option(k, v)
        return sc


def _rows(geometry, sizes, listed=0, dropped=0, sah=1, lbvh=1, zero_axes=(), flat_list=-1):
    return [Case(geometry, n, listed, dropped, sah if n > 8 else 0, lbvh if n > 8 else 0, zero_axes, flat_list) for n in sizes]


# geometry, tree sizes | listed, dropped | on the device: SAH, LBVH
CASES = (
    _rows("soup", SIZES)
    + _rows("walls_soup", (8, 9, 65, 257, 1025), listed=12)
    + _rows("zero_area", (9, 63, 256, 1025))
    + _rows("planar", (9, 64, 255, 1025), zero_axes=(1,))
    + _rows("line", (9, 65, 257, 1025), zero_axes=(0, 1))
    + _rows("concentric", (9, 64, 256, 1025), listed=CONCENTRIC_LISTED, sah=0, zero_axes=(0, 1, 2))      # the host's root is a median split
    + _rows("duplicates", (9, 10, 64, 256, 1025))
    + _rows("clustered", (9, 63, 257, 1025))
    + _rows("huge", (9, 65, 255, 1025), listed=2)                                       # the list takes the pair: a second d_sel case
    + _rows("huge_tree", (9, 65, 255, 1025), sah=0, flat_list=0)                          # the pair in the tree; the host splits at the median
    + _rows("nonfinite", (9, 64, 256, 1025), dropped=3, sah=0, lbvh=0)
)
CASE_IDS = [c.id for c in CASES]


def padded_boxes(verts):
    """the padded bounds of triangles (n, 3, 3) as every builder computes them (padded_bounds of pt_builder.cpp, tri_bounds of the
    device builders), in float32 step by step: lo (n, 3), hi (n, 3)"""
    v = np.asarray(verts, dtype=np.float32)
    lo, hi = v.min(axis=1), v.max(axis=1)
    m = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)
    pad = ((m * np.float32(1e-5)).astype(np.float32) + np.float32(1e-6)).astype(np.float32)[:, None]
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def box_centres(verts):
    """centres of those boxes, (n, 3)"""
    lo, hi = padded_boxes(verts)
    with np.errstate(over="ignore"):                          # (the huge pair's sum is +inf, as in the builders)
        return (np.float32(0.5) * (lo + hi).astype(np.float32)).astype(np.float32)


def check_node_boxes(nodes, tris):
    """Every child box of the packed BVH2 is, bit for bit, the union of the padded bounds of the triangles below it (min and max
    round nothing, so any builder must arrive at the same planes)."""
    plo, phi = padded_boxes(tris[:, :9].reshape(-1, 3, 3))
    refs = nodes[:, 12:14].view(np.int32)
    want = {}

    def box_of(ref):
        if ref < 0:
            first, count = (~ref) >> 3, ((~ref) & 7) + 1
            return plo[first:first + count].min(axis=0), phi[first:first + count].max(axis=0)
        return want[ref]
    order, todo = [], [0]                                   # parents in front of their children (the radix tree numbers them freely)
    while todo:
        i = todo.pop()
        order.append(i)
        todo += [int(r) for r in refs[i] if r >= 0]
    assert len(order) == len(set(order)) == nodes.shape[0]
    for i in reversed(order):
        kids = []
        for side in (0, 1):
            ref = int(refs[i, side])
            have_lo, have_hi = nodes[i, [0 + 2 * side, 4 + 2 * side, 8 + 2 * side]], nodes[i, [1 + 2 * side, 5 + 2 * side, 9 + 2 * side]]
            if ref == ~0 and np.all(np.isposinf(have_lo)) and np.all(np.isneginf(have_hi)):
                continue                                   # no child: the inverted box next to a scene that is one leaf (build_attempt)
            lo, hi = box_of(ref)
            assert np.array_equal(have_lo.view(np.uint32), lo.view(np.uint32)) and np.array_equal(have_hi.view(np.uint32), hi.view(np.uint32)), \
                "node %d child %d: box %s %s, the triangles' padded bounds %s %s" % (i, side, have_lo, have_hi, lo, hi)
            kids.append((lo, hi))
        want[i] = (np.min([k[0] for k in kids], axis=0), np.max([k[1] for k in kids], axis=0))


def tree_vertices(case, spec):
    """corners (k, 3, 3) of the finite triangles of `spec` that are small enough to be aimed at (not the walls, not the huge pair)"""
    v = np.concatenate([o[0] for o in spec.objects]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v).all(axis=(1, 2)) & (np.abs(np.nan_to_num(v)).max(axis=(1, 2)) < 1e6)
    if case.geometry == "walls_soup":
        ok[:12] = False
    return v[ok]


def rays(case, spec):
    """The case's 2,048 fixed rays.  The first half is random: origins around the scene's triangles, half of the directions isotropic, half
    towards a random point of the triangles' box.  The second half is aimed, from the eye or from a random origin, at triangle
    centroids and at the midpoints of edges in turn -- of every triangle the edge with the fewest zero components, which in a mesh
    is the diagonal two triangles share.  (Corners, and edges that lie in an axis-aligned face of a box, are left out: there the
    reference's own unpadded slab test loses hits, DESIGN.md section 3, and the oracle's two searches could not be compared.)"""
    rng = np.random.RandomState(7000 + case.n)
    v = tree_vertices(case, spec)
    eye = EYE + np.asarray(spec.shift, dtype=np.float64)
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    span = np.maximum(hi - lo, 1.0)
    h = N_RAYS // 2
    P = np.empty((N_RAYS, 3))
    D = np.empty((N_RAYS, 3))
    P[:h] = rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (h, 3))
    D[:h // 2] = _unit(rng, (h // 2,))
    D[h // 2:h] = rng.uniform(lo, hi, (h - h // 2, 3)) - P[h // 2:h]
    tri = v[np.arange(h) % len(v)]
    kind = (np.arange(h) // len(v) + np.arange(h)) % 2
    edges = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], axis=1)
    pick = np.argmax((np.abs(edges) > 1e-6 * np.linalg.norm(edges, axis=2, keepdims=True)).sum(axis=2), axis=1)
    mid = 0.5 * (tri[np.arange(h), pick] + tri[np.arange(h), (pick + 1) % 3])
    target = np.where((kind == 0)[:, None], tri.mean(axis=1), mid)
    from_eye = rng.rand(h) < 0.5
    P[h:] = np.where(from_eye[:, None], eye, rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (h, 3)))
    D[h:] = target - P[h:]
    D /= np.maximum(np.linalg.norm(D, axis=1, keepdims=True), 1e-30)
    out = np.zeros(N_RAYS, dtype=RAY)
    out["P"][:, :3] = P.astype(np.float32)
    out["D"][:, :3] = D.astype(np.float32)
    return out
