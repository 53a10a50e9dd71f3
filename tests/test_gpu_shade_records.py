"""-m gpu: the per-triangle shading records (ShadeRec; shade_hit<SK, REC = true>) against the CPU oracle, bit for bit.

The schedule-2 item loop of the fused k_render instances with the tree in LDS reads, per hit, a record that was built once per upload: the packed normal, the
material's type / index / kd and the tangent frame of the cosine lobe for BOTH orientations of the triangle.  The other instances
(schedules 0 and 1, nodes from global memory, the split API's trace_ray) compute the same inline.  Every test compares colours and LCG states (and, for
the split API, the rays buffer) with the oracle, which knows nothing of records.

The frame scene: a closed box (the enclosure, seen from inside only) around free-standing two-sided panels whose normals are
+-x, +-y, +-z, the `yaxis` case of the frame on both sides of its 0.001 threshold, and generic oblique ones; all four material types,
one diffuse material with ks != 0.  That both orientations of every panel triangle can be hit is argued on the CPU alone
(test_frame_scene_orientations_cpu) with a PROXY of the rendered paths, not a count of their hits: the oracle's camera rays and
three generations of the oracle's diffuse bounces -- taken off every panel, mirrors, glass and emitters included -- followed with a
float64 intersection in numpy, reach every (panel triangle, side).  It justifies the scene; the bit comparisons are the check.

Materials can only be appended through the API (pt_add_material pushes back; no call edits one), so a triangle's record cannot
change through pt_upload_materials alone: the dirty flag that call sets is not observable through this API and is NOT covered here.
test_records_follow_uploads re-uploads materials after appending two that no triangle uses -- that step only shows that a rebuild
in front of the next launch does no harm, it would pass with stale records -- and then adds triangles that use them (a mirror, and
a diffuse one with another kd): that step fails when the records are not rebuilt after pt_upload_triangles."""
import ctypes as C

import numpy as np
import pytest

from opencl_path_tracer_amd import scenes

W, H, BOUNCES, SPP = 64, 48, 8, 8
SHIFT = (0.0, 0.0, 600.0)            # eye (500, 500, -699): inside the box
E = 0.001                            # the frame's yaxis threshold (prog.cl:206)


def _normal_tri(center, n, size):
    """One triangle around `center` whose geometric normal is (close to) n / |n|."""
    n = np.asarray(n, np.float64)
    n /= np.linalg.norm(n)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(n, a)
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    c = np.asarray(center, np.float64)
    return [c - (u + v) * size / 3.0, c + u * size - (u + v) * size / 3.0, c + v * size - (u + v) * size / 3.0]


def _both_windings(a, b, c, d):
    """Quad a b c d as two triangles of OPPOSITE winding: stored normals N and -N."""
    return [[a, b, c], [a, d, c]]


def frame_scene():
    """-> (SceneSpec, index of the first panel triangle, expected normals of special panels)."""
    M = scenes
    box = []
    lo, hi = (0.0, 0.0, -900.0), (1000.0, 1000.0, 1000.0)
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    for q in ([(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)], [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
              [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], [(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)],
              [(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)], [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]):
        box += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    box_m = [M.WHITE_DIFFUSE] * 2 + [M.RED_DIFFUSE] * 2 + [M.WHITE_DIFFUSE] * 2 + [M.WHITE_DIFFUSE] * 2 + [M.GREEN_DIFFUSE] * 2 + [M.WHITE_DIFFUSE] * 2
    p, pm = [], []
    # +-x, +-y, +-z: both windings of an axis-aligned quad each
    p += _both_windings((200, 100, 0), (200, 500, 0), (200, 500, 400), (200, 100, 400)); pm += [M.WHITE_DIFFUSE, M.RED_DIFFUSE]
    p += _both_windings((400, 300, 100), (700, 300, 100), (700, 300, 500), (400, 300, 500)); pm += [M.RED_DIFFUSE, M.WHITE_DIFFUSE]
    p += _both_windings((600, 100, 600), (900, 100, 600), (900, 500, 600), (600, 500, 600)); pm += [M.PURPLE_SPECULAR, M.PURPLE_SPECULAR]
    # the emitter: a two-sided lamp panel below the ceiling
    p += _both_windings((300, 900, 0), (700, 900, 0), (700, 900, 400), (300, 900, 400)); pm += [M.LAMP, M.LAMP]
    # the yaxis case on both sides of its threshold: |N.x| just above / just below 0.001 with |N.z| below; and |N.z| above with |N.x| below
    special = {}
    for name, n, c, m in (("x_above", (0.0011, 1.0, 0.0002), (250, 650, 300), M.WHITE_DIFFUSE), ("x_below", (0.0009, 1.0, 0.0002), (500, 700, 500), M.RED_DIFFUSE),
                          ("z_above", (0.0002, -1.0, 0.0012), (750, 650, 200), M.GREEN_DIFFUSE), ("x_below_neg", (-0.0008, -1.0, -0.0003), (500, 600, -100), M.WHITE_DIFFUSE)):
        special[name] = len(p)
        p.append(_normal_tri(c, n, 420.0)); pm.append(m)
    # generic oblique normals: diffuse, diffuse with a specular lobe, mirror, dielectric, emitter
    for n, c, m in (((0.3, 0.5, 0.8), (300, 300, 700), M.WHITE_DIFFUSE), ((-0.6, 0.2, 0.77), (800, 700, 700), M.BLACK_SPECULAR),
                    ((-0.5, 0.2, 0.84), (150, 700, 600), M.CHROMIUM), ((0.6, -0.3, 0.74), (700, 300, -50), M.GLASS), ((0.2, -0.9, 0.4), (600, 820, 650), M.SUN)):
        p.append(_normal_tri(c, n, 380.0)); pm.append(m)
    spec = scenes.SceneSpec(materials=list(scenes.BUILTIN_MATERIALS), name="frame_scene", shift=SHIFT)
    spec.objects.append((np.asarray(box, np.float32), np.asarray(box_m, np.uint16)))
    spec.objects.append((np.asarray(p, np.float32), np.asarray(pm, np.uint16)))
    return spec, len(box), special


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check(sc, fr, what):
    cols, rnds = sc.read_colors(), sc.read_rnds()
    assert np.array_equal(rnds, fr.rnds()), "%s: %d pixels ended on a different LCG state" % (what, int((rnds != fr.rnds()).sum()))
    assert same_bits(cols[:, :3], fr.colors()[:, :3]), "%s: colours differ in bits" % what
    assert cols[:, :3].any(), "%s: black frame" % what


@pytest.fixture(scope="module")
def fs():
    return frame_scene()


@pytest.fixture(scope="module")
def fs_oracle(oracle, fs):
    """The oracle's scene and its frames, rendered once: (scene, {(bounces, spp): frame})."""
    spec = fs[0]
    osc = oracle.load_scene(spec)
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    frames = {}
    for bounces, spp in ((BOUNCES, SPP), (1, 3)):
        fr = oracle.OracleFrame(W, H)
        fr.render(osc, cam, bounces, 0, spp, nthreads=16)
        frames[(bounces, spp)] = fr
    return osc, frames


def _first_hits(tris, P, D):
    """float64 Moeller-Trumbore of rays (m) against triangles (n): nearest triangle index (-1: none), t, and whether the ray arrived
    on the side the stored normal (r2 - r1) x (r3 - r1) points to."""
    a, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pv = np.cross(D[:, None, :], e2[None])
    det = (e1[None] * pv).sum(-1)
    ok = np.abs(det) > 1e-12
    inv = 1.0 / np.where(ok, det, 1.0)
    tv = P[:, None, :] - a[None]
    u = (tv * pv).sum(-1) * inv
    qv = np.cross(tv, e1[None])
    v = (D[:, None, :] * qv).sum(-1) * inv
    t = (e2[None] * qv).sum(-1) * inv
    ok &= (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-6)
    t = np.where(ok, t, np.inf)
    idx = t.argmin(1)
    tt = t[np.arange(len(P)), idx]
    n = np.cross(e1, e2)
    front = (D * n[idx]).sum(-1) < 0
    return np.where(np.isfinite(tt), idx, -1), tt, front


@pytest.mark.gpu
def test_frame_scene_orientations_cpu(oracle, fs):
    """CPU only (kept with the GPU tests it justifies): the normals are the cases the frame has, and a proxy of the rendered paths --
    the oracle's camera rays plus three generations of its diffuse bounces off whatever panel was hit, whatever its material -- reaches
    both sides of every panel triangle.  It shows that each side is reachable, not that the rendered paths hit it."""
    spec, first_panel, special = fs
    verts = np.concatenate([v for v, _ in spec.objects]).astype(np.float32)
    N = np.stack([oracle.make_triangle(t[0], t[1], t[2], 0)["N"][0][:3] for t in verts])
    pn = N[first_panel:]
    for axis in range(3):
        for sign in (1.0, -1.0):
            want = np.zeros(3, np.float32)
            want[axis] = sign
            assert any(np.array_equal(n, want) for n in pn), "no panel with normal %s" % want
    ax, bx, az, bn = (pn[special[k]] for k in ("x_above", "x_below", "z_above", "x_below_neg"))
    assert E < abs(ax[0]) < 1.3 * E and abs(ax[2]) <= E                      # not yaxis, by N.x alone
    assert 0.7 * E < abs(bx[0]) <= E and abs(bx[2]) <= E                     # yaxis
    assert abs(az[0]) <= E and E < abs(az[2]) < 1.4 * E                      # not yaxis, by N.z alone
    assert 0.6 * E < abs(bn[0]) <= E and abs(bn[2]) <= E and bn[1] < 0       # yaxis, the stored normal pointing down
    types = {spec.materials[m][6] for _, ms in spec.objects for m in ms}
    assert types == {0, 1, 2, 3}
    assert any(spec.materials[m][6] == 0 and any(spec.materials[m][1]) for m in spec.objects[1][1])      # diffuse with ks != 0

    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    fr.generate_rays(cam)
    rays = fr.rays()
    P, D = rays["P"][:, :3].astype(np.float64), rays["D"][:, :3].astype(np.float64)
    tris = verts.astype(np.float64)
    seen = set()
    L = oracle.lib()
    seed = C.c_int(12345)
    out = np.zeros(1, oracle.RAY)
    for gen in range(4):
        idx, t, front = _first_hits(tris, P, D)
        keep = idx >= 0
        seen |= set(zip(idx[keep].tolist(), front[keep].tolist()))
        if gen == 3:
            break
        nP, nD = [], []
        for i in np.flatnonzero(keep):
            n = N[idx[i]].astype(np.float32) * (1.0 if front[i] else -1.0)
            hp = (P[i] + D[i] * t[i] + n * 0.01).astype(np.float32)
            p4, n4 = np.zeros(4, np.float32), np.zeros(4, np.float32)
            p4[:3], n4[:3] = hp, n
            L.orc_new_ray_diffuse(out.ctypes.data_as(C.c_void_p), p4.ctypes.data_as(C.c_void_p), n4.ctypes.data_as(C.c_void_p),
                                  L.orc_rand(C.byref(seed)), L.orc_rand(C.byref(seed)))
            nP.append(hp.astype(np.float64))
            d = out["D"][0][:3].astype(np.float64)
            nD.append(d / np.linalg.norm(d))
        P, D = np.asarray(nP), np.asarray(nD)
    missing = [(i, s) for i in range(first_panel, len(tris)) for s in (True, False) if (i, s) not in seen]
    assert not missing, "panel (triangle, front side) never reached: %s" % missing


@pytest.mark.gpu
@pytest.mark.parametrize("lds,wide,schedule", [(2, 1, 0), (2, 1, 1), (2, 1, 2), (0, 0, 1), (0, 2, 2)])
def test_frame_scene_render(api, fs, fs_oracle, lds, wide, schedule):
    """render(n) under schedules 0, 1 (inline) and 2 (records) with the tree in LDS, and with lds_scene 0: BVH2 and 4-wide nodes (inline)."""
    spec = fs[0]
    sc = api.Scene(W, H)
    sc.set_option("wide_nodes", wide)
    sc.load(spec)
    sc.set_option("lds_scene", lds)
    sc.set_option("schedule", schedule)
    assert sc.stat("node_mode") == {(2, 1): 0, (0, 0): 1, (0, 2): 3}[(lds, wide)]
    sc.iterations = BOUNCES
    sc.render(SPP // 2)
    sc.render(SPP - SPP // 2)                     # the second launch finds the records built
    check(sc, fs_oracle[1][(BOUNCES, SPP)], "lds_scene %d wide_nodes %d schedule %d" % (lds, wide, schedule))


@pytest.mark.gpu
def test_frame_scene_split_api(api, fs, fs_oracle):
    """generate_rays / trace_rays per sample: colours, LCG states and the rays left in the rays buffer."""
    spec = fs[0]
    sc = api.Scene(W, H).load(spec)
    assert sc.stat("node_mode") == 0
    sc.iterations = BOUNCES
    sc.render(SPP, fused=False)
    fr = fs_oracle[1][(BOUNCES, SPP)]
    check(sc, fr, "split")
    rays, orays = sc.read_rays(), fr.rays()
    assert same_bits(rays["P"][:, :3], orays["P"][:, :3]) and same_bits(rays["D"][:, :3], orays["D"][:, :3])


@pytest.mark.gpu
def test_frame_scene_flat_preview(api, fs, fs_oracle):
    """iterations == 1 (prog.cl:323-325): kd from the record, emission through mati."""
    sc = api.Scene(W, H).load(fs[0])
    assert sc.stat("node_mode") == 0
    sc.set_option("schedule", 2)                  # the item loop that reads records
    sc.iterations = 1
    sc.render(3)
    check(sc, fs_oracle[1][(1, 3)], "iterations 1")


def _author(target, spec, n_mats, objects):
    for m in spec.materials[:n_mats]:
        target.add_Material(*m)
    for verts, mati in objects:
        if hasattr(target, "add_Triangles"):
            from opencl_path_tracer_amd import api
            target.add_Triangles(api.triangles_from_vertices(verts, mati))
        else:
            target.add_triangles(verts, mati)
        target.end_Obj()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [8, 4])
def test_records_follow_uploads(api, oracle, fs, spp):
    """A render after an upload never sees records of the state before it: every result equals the oracle's for the final state.
    Step 1: render; append two materials (a mirror, a diffuse one with another kd) and upload_Materials; render again.  No triangle
    uses them, so no record changes: the step would pass with stale records (see the module docstring).
    Step 2: add_Triangles + end_Obj + upload_Triangles with triangles that use them (+ upload_Materials); render again.  This one
    fails without a rebuild."""
    spec = fs[0]
    mats = list(spec.materials) + [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (2.0, 2.5, 3.0), (3.0, 3.0, 3.0), 0.0, 1),
                                   ((0.1, 0.25, 0.3), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 10.0, 0)]
    full = scenes.SceneSpec(materials=mats, objects=list(spec.objects), shift=SHIFT)
    n0 = len(spec.materials)
    extra = (np.asarray([_normal_tri((450, 450, 250), (0.1, 0.3, -0.95), 500.0), _normal_tri((550, 250, 150), (0.0005, 1.0, 0.0005), 450.0)], np.float32),
             np.asarray([n0, n0 + 1], np.uint16))
    cam = oracle.make_camera(full.fov, full.yaw, full.pitch, full.shift, W, H)

    def oracle_frame(n_mats, objects):
        osc = oracle.OracleScene()
        _author(osc, full, n_mats, objects)
        fr = oracle.OracleFrame(W, H)
        fr.render(osc, cam, BOUNCES, 0, spp, nthreads=16)
        return fr

    sc = api.Scene(W, H)
    _author(sc, full, n0, full.objects)
    sc.upload_Triangles()
    sc.upload_Materials()
    sc.set_view(full.fov, full.yaw, full.pitch, full.shift)
    sc.set_option("schedule", 2)                  # the item loop that reads records
    assert sc.stat("node_mode") == 0
    sc.iterations = BOUNCES
    sc.render(spp)
    before = oracle_frame(n0, full.objects)
    check(sc, before, "before any change")

    for m in mats[n0:]:
        sc.add_Material(*m)
    sc.upload_Materials()
    sc.seed_default()
    sc.current_sample = 0
    sc.render(spp)
    check(sc, before, "after upload_Materials")          # (no triangle uses the new materials yet: not a staleness check)

    sc.add_Triangles(api.triangles_from_vertices(*extra))
    sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    sc.seed_default()
    sc.current_sample = 0
    sc.render(spp)
    after = oracle_frame(len(mats), full.objects + [extra])
    check(sc, after, "after add_Triangles + upload_Triangles")
    fresh = api.Scene(W, H).load(scenes.SceneSpec(materials=mats, objects=full.objects + [extra], shift=SHIFT))
    fresh.set_option("schedule", 2)
    fresh.iterations = BOUNCES
    fresh.render(spp)
    assert same_bits(sc.read_colors(), fresh.read_colors()) and np.array_equal(sc.read_rnds(), fresh.read_rnds())
    assert not same_bits(after.colors(), before.colors())      # the change is visible
