"""The light hierarchy of Scene.render_nee (option light_tree) on host-only contexts: the option, the tree's invariants on small and
degenerate light sets, the two walks of pt_debug_light_tree_eval (their probabilities sum to 1, the pick's P is the weight walk's,
stratified u0 reach each light in proportion to its P), the horizon cull, and tests/lighttree_ref.py's float64 walk against the
library's float32 one.  No device needed."""

import os

import numpy as np
import pytest

import lighttree_ref as LT

NEW_SYMBOLS = ["pt_debug_light_tree", "pt_debug_light_tree_eval"]


def host_scene(api, spec):
    sc = api.Scene(16, 16, device=None)
    for m in spec.materials:
        sc.add_Material(*m)
    for verts, mati in spec.objects:
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def phi_of_spec(spec):
    """{add-order triangle: area x (E.r + E.g + E.b) in float64} of the lights the table keeps, and the scene's vertices"""
    verts = np.concatenate([v for v, _ in spec.objects]).astype(np.float32)
    mo = np.concatenate([m for _, m in spec.objects])
    out = {}
    for i, v in enumerate(verts.astype(np.float64)):
        m = spec.materials[int(mo[i])]
        es = (float(np.float32(m[2][0])) + float(np.float32(m[2][1]))) + float(np.float32(m[2][2]))
        area = 0.5 * np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0]))
        if m[6] == 3 and es > 0 and area > 0:
            out[i] = area * es
    return out, verts


def lights_spec(tris, mats_of, extra_mats=(), per_object=False):
    """a scene of the emitting triangles `tris` (material 1 + mats_of[i]) over one diffuse floor triangle; per_object: one object per
    triangle (an object may not hold more than six triangles that share a centroid)"""
    from opencl_path_tracer_amd import scenes
    mats = [((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),
            ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),
            ((0, 0, 0), (0, 0, 0), (0.5, 0.25, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3)] + list(extra_mats)
    v = [((-50.0, -5.0, -50.0), (50.0, -5.0, -50.0), (0.0, -5.0, 80.0))] + [tuple(map(tuple, t)) for t in tris]
    mo = [0] + [1 + int(m) for m in mats_of]
    spec = scenes.SceneSpec(materials=mats, name="lights")
    v, mo = np.asarray(v, dtype=np.float32).reshape(-1, 3, 3), np.asarray(mo, dtype=np.uint16)
    if per_object:
        spec.objects += [(v[i:i + 1], mo[i:i + 1]) for i in range(len(v))]
    else:
        spec.objects.append((v, mo))
    return spec


def random_lights(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10.0, 10.0, size=(n, 1, 3))
    return c + rng.uniform(-0.5, 0.5, size=(n, 3, 3)), rng.integers(0, 2, size=n)


def checked_tree(api, spec):
    sc = host_scene(api, spec)
    nodes, tri = sc.debug_light_tree()
    phi, verts = phi_of_spec(spec)
    depth = LT.check_invariants(nodes, tri, verts, phi)
    assert sc.stat("light_tree_depth") == depth and sc.stat("light_tree_nodes") == len(nodes)
    assert sorted(tri.tolist()) == sorted(sc.debug_light_table()[0].tolist())          # the table's lights, which keeps its own order
    nodes2, tri2 = host_scene(api, spec).debug_light_tree()                            # a second build: the same bytes
    assert nodes.tobytes() == nodes2.tobytes() and tri.tobytes() == tri2.tobytes()
    return sc, nodes, tri, depth


def test_option_and_symbols(api):
    from opencl_path_tracer_amd import scenes
    sc = host_scene(api, scenes.many_lights(4))
    sc.set_option("light_tree", 1)                 # PT_EINVAL ("unknown option") before the hierarchy existed
    sc.set_option("light_tree", 0)
    with pytest.raises(api.PtError) as e:
        sc.set_option("light_tree", 2)
    assert e.value.code == api.PT_EINVAL and "light_tree" in str(e.value)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pt_api.h")).read()
    hpp = open(os.path.join(root, "include", "pt_scene.hpp")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name) and name + "(" in header and name[3:] + "(" in hpp
    assert "typedef struct pt_light_tree_eval {" in header
    assert api.LIGHT_TREE_NODE.itemsize == 32 and api.LIGHT_TREE_EVAL.itemsize == 16


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 257])
def test_tree_invariants_by_count(api, n):
    tris, mo = random_lights(n, 100 + n)
    sc, nodes, tri, depth = checked_tree(api, lights_spec(tris, mo))
    assert len(tri) == n and len(nodes) == max(2 * n - 1, 0)
    if n:
        assert depth >= int(np.ceil(np.log2(n)))
    # the picks of an empty table and of a table of one light
    ev = sc.debug_light_tree_eval([(0, 0, 0)], [(0, 1, 0)], [0.5], [1])
    if n == 0:
        assert ev["tri"][0] == -1 and ev["p"][0] == 0.0 and ev["p_weight"][0] == 0.0
    if n == 1:
        assert ev["tri"][0] == 1 and ev["p"][0] == 1.0 and ev["p_weight"][0] == 1.0


def test_tree_invariants_degenerate_sets(api):
    one = np.array([(1.0, 2.0, 3.0), (2.0, 2.0, 3.0), (1.0, 2.0, 4.5)])
    # 70 copies of one triangle: every centroid coincides, the median leaves a side empty at every node: equal counts, depth 7
    _, _, _, depth = checked_tree(api, lights_spec([one] * 70, [0] * 70, per_object=True))
    assert depth == 7
    # one huge emitter among tiny ones
    tris, mo = random_lights(40, 7)
    tris = np.concatenate([tris * 0.01, [np.array([(-400.0, 30.0, -400.0), (400.0, 30.0, -400.0), (0.0, 30.0, 600.0)])]])
    checked_tree(api, lights_spec(tris, list(mo) + [0]))
    # black and zero-area emitters, which the table leaves out
    black = ((0, 0, 0), (0, 0, 0), (0.0, 0.0, 0.0), (0, 0, 0), (0, 0, 0), 0.0, 3)
    tris, mo = random_lights(9, 8)
    tris[4] = np.array([(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)])          # zero area
    mo = list(mo)
    mo[2] = mo[6] = 2                                                               # the black material (index 3)
    sc, _, tri, _ = checked_tree(api, lights_spec(tris, mo, [black]))
    assert len(tri) == 6 and not {1 + 2, 1 + 4, 1 + 6} & set(tri.tolist())
    # centroids in geometric progression along x: the spatial median peels one light off per level, so the depth rule has to take over
    n = 90
    tris = [[(1000.0 * 2.0 ** -i, 0.0, 0.0), (1000.0 * 2.0 ** -i, 1.0, 0.0), (1000.0 * 2.0 ** -i, 0.0, 1.0)] for i in range(n)]
    _, _, _, depth = checked_tree(api, lights_spec(tris, [0] * n))
    assert 58 <= depth <= 64


# ------------------------------------------------------------------ the walks on many_lights(16)
N_LAMPS = 16


@pytest.fixture(scope="module")
def corridor(api):
    from opencl_path_tracer_amd import scenes
    spec = scenes.many_lights(N_LAMPS)
    sc, nodes, tri, depth = checked_tree(api, spec)
    assert len(tri) == 2 * N_LAMPS
    rng = np.random.default_rng(5)
    z1 = 3.0 * N_LAMPS + 2.0
    pts, nrm = [], []
    for _ in range(24):                                                             # the floor
        pts.append((rng.uniform(-1.9, 1.9), -1.499, rng.uniform(-0.9, z1 - 0.1)))
        nrm.append((0.0, 1.0, 0.0))
    for k in range(24):                                                             # the two walls
        s = 1.0 if k % 2 else -1.0
        pts.append((-1.999 * s, rng.uniform(-1.4, 1.4), rng.uniform(-0.9, z1 - 0.1)))
        nrm.append((s, 0.0, 0.0))
    for k in range(16):                                                             # mid-air: a random normal, or none (a scatter vertex)
        pts.append((rng.uniform(-1.9, 1.9), rng.uniform(-1.4, 1.4), rng.uniform(-0.9, z1 - 0.1)))
        g = rng.normal(size=3)
        nrm.append(tuple(g / np.linalg.norm(g)) if k % 2 else (0.0, 0.0, 0.0))
    return dict(sc=sc, spec=spec, tree=LT.Tree(nodes, tri), tri=tri, depth=depth, pts=np.asarray(pts, dtype=np.float32),
                nrm=np.asarray(nrm, dtype=np.float32))


def all_weights(c, pts, nrm):
    """the weight walk's P of every light (tree order) at every point: (len(pts), lights) float32"""
    nl = len(c["tri"])
    ev = c["sc"].debug_light_tree_eval(np.repeat(pts, nl, axis=0), np.repeat(nrm, nl, axis=0), np.zeros(len(pts) * nl), np.tile(c["tri"], len(pts)))
    return ev["p_weight"].reshape(len(pts), nl)


def test_weights_sum_to_one(corridor):
    # one rounding of 1 - pL and one of the product per level, 2^-24 each at most in absolute terms, with a factor 2 of margin
    P = all_weights(corridor, corridor["pts"], corridor["nrm"]).astype(np.float64)
    assert np.abs(P.sum(axis=1) - 1.0).max() <= corridor["depth"] * 2.0 ** -22


def test_pick_probability_is_the_weight_walks(corridor):
    c = corridor
    rng = np.random.default_rng(6)
    k = 64
    pts, nrm = np.repeat(c["pts"], k, axis=0), np.repeat(c["nrm"], k, axis=0)
    u0 = (rng.integers(0, 1 << 24, size=len(pts)) * 2.0 ** -24).astype(np.float32)
    a = c["sc"].debug_light_tree_eval(pts, nrm, u0, np.zeros(len(pts)))
    assert (a["tri"] >= 0).all() and (c["tri"][a["slot"]] == a["tri"]).all()
    b = c["sc"].debug_light_tree_eval(pts, nrm, u0, a["tri"])
    assert np.array_equal(a["p"].view(np.uint32), b["p_weight"].view(np.uint32))
    assert (a["p"] > 0).all()
    assert c["sc"].debug_light_tree_eval(pts[:4], nrm[:4], u0[:4], [2 * N_LAMPS, 2 * N_LAMPS + 3, -1, 10 ** 6])["p_weight"].tolist() == [0.0] * 4   # no lights


def test_stratified_u0_reaches_each_light_in_proportion(corridor):
    # the u0 that reach a leaf form an interval, so the count of the 2^16 strata in it is off by at most one at each end
    c = corridor
    m = 1 << 16
    u0 = ((np.arange(m) + 0.5) / m).astype(np.float32)
    P = all_weights(c, c["pts"], c["nrm"]).astype(np.float64)
    nl = len(c["tri"])
    worst = 0.0
    for i in range(len(c["pts"])):
        ev = c["sc"].debug_light_tree_eval(np.tile(c["pts"][i], (m, 1)), np.tile(c["nrm"][i], (m, 1)), u0, np.zeros(m))
        share = np.bincount(ev["slot"], minlength=nl) / m
        worst = max(worst, float(np.abs(share - P[i]).max()))
    assert worst <= 2.0 / m, worst


def test_horizon_cull(corridor):
    c = corridor
    below = [2 * (N_LAMPS // 2), 2 * (N_LAMPS // 2) + 1]                # the lamp under the floor
    slots = [int(np.nonzero(c["tri"] == t)[0][0]) for t in below]
    floor = c["pts"][:24]
    P = all_weights(c, floor, c["nrm"][:24])
    assert (P[:, slots] == 0.0).all()                                   # culled while other lamps are above the horizon
    others = np.delete(P, slots, axis=1)
    assert (others > 0.0).all()
    P0 = all_weights(c, floor, np.zeros_like(floor))                    # G = 0: nothing is culled
    assert (P0 > 0.0).all()
    # every lamp below the horizon: the probabilities are the phi shares
    phi, _ = phi_of_spec(c["spec"])
    share = np.array([phi[int(t)] for t in c["tri"]])
    share /= share.sum()
    Pf = all_weights(c, np.array([(0.0, 1000.0, 20.0)], dtype=np.float32), np.array([(0.0, 1.0, 0.0)], dtype=np.float32))[0]
    assert np.abs(Pf.astype(np.float64) - share).max() <= c["depth"] * 2.0 ** -22


def test_float64_model_agrees_with_the_host_walk(corridor):
    c = corridor
    rng = np.random.default_rng(9)
    k = 64
    pts, nrm = np.repeat(c["pts"], k, axis=0), np.repeat(c["nrm"], k, axis=0)
    u0 = (rng.integers(0, 1 << 24, size=len(pts)) * 2.0 ** -24).astype(np.float32)
    want = [c["tree"].pick(pts[i].astype(np.float64), nrm[i].astype(np.float64), float(u0[i])) for i in range(len(pts))]
    near = np.array([w[2] for w in want])
    assert near.mean() <= 0.01                                          # the model alone: the cases left out stay under the cap
    got = c["sc"].debug_light_tree_eval(pts, nrm, u0, np.zeros(len(pts)))
    keep = ~near
    assert np.array_equal(got["slot"][keep], np.array([w[0] for w in want])[keep])
    # about 20 float32 operations of half an ulp per level
    assert np.abs(got["p"][keep].astype(np.float64) - np.array([w[1] for w in want])[keep]).max() <= c["depth"] * 2e-6
    # and the weight walk of the model is its pick's P
    for i in range(0, len(pts), 97):
        assert c["tree"].weight(pts[i].astype(np.float64), nrm[i].astype(np.float64), want[i][0]) == pytest.approx(want[i][1], rel=1e-12)
    assert c["tree"].depth() == c["depth"]
