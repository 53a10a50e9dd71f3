"""-m "not gpu": the scenes of builder_scenes.py on host-only contexts and in the oracle, so that no comparison of
test_gpu_device_builders.py is vacuous: every generator gives the tree and the list it promises, the host builder's trees of
all three leaf policies are valid, the on-device column of the case table follows from the host builder alone, and the oracle's
two searches agree on the fixed rays and hit often enough."""
import numpy as np
import pytest

import builder_scenes as bs
import bvh_check

HOST_POLICIES = (0, 2, 3)          # the trees bvh_policy 5 / 2 / 3 name (pt_builder.cpp tree_policy)


def host_scene(api, case, spec, policy, wide=0):
    sc = case.configure(api.Scene(32, 24, device=None))
    sc.set_option("bvh_policy", policy)
    sc.set_option("wide_nodes", wide)
    return sc.load(spec)


@pytest.fixture(scope="module")
def specs():
    return {c.id: c.spec() for c in bs.CASES}


@pytest.mark.parametrize("case", bs.CASES, ids=bs.CASE_IDS)
def test_generator_gives_the_tree_and_the_list(api, specs, case):
    spec = specs[case.id]
    assert spec.ntris == case.n + case.listed + case.dropped
    assert sum(int((m == 0).sum() + (m == 1).sum()) for _, m in spec.objects) >= 2, "no emitter"
    sc = host_scene(api, case, spec, 0)
    nf = int(sc.stat("flat_triangles"))
    assert nf == case.listed and sc.stat("triangles") - nf == case.n
    if case.geometry == "soup":
        assert nf == 0
    _, _, _, orig = sc.debug_bvh()
    verts = np.concatenate([o[0] for o in spec.objects])
    assert np.isfinite(verts[orig]).all() and len(set(orig.tolist())) == len(orig)
    c = bs.box_centres(verts[orig[nf:]])
    ext = c.max(axis=0) - c.min(axis=0)
    for a in range(3):
        assert (ext[a] == 0) == (a in case.zero_axes), "axis %d: centroid extent %g" % (a, ext[a])
    if case.geometry == "duplicates":
        w = verts.view(np.uint32).reshape(-1, 9)
        assert np.array_equal(w[0:case.n - 1:2], w[1:case.n:2])
    if case.geometry == "zero_area":
        e1, e2 = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
        thin = np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1) < 0.05
        assert thin.sum() == len(range(2, case.n, 3))


@pytest.mark.parametrize("case", bs.CASES, ids=bs.CASE_IDS)
def test_host_trees_are_valid(api, specs, case):
    for policy in HOST_POLICIES:
        sc = host_scene(api, case, specs[case.id], policy, wide=2)
        nodes, tris, meta, orig = sc.debug_bvh()
        nf = int(sc.stat("flat_triangles"))
        depth = bvh_check.validate_structure(nodes, tris, len(orig), nf)
        assert depth <= sc.stat("bvh_depth")
        bs.check_node_boxes(nodes, tris)
        wide = sc.debug_wide_nodes()
        assert len(wide) > 0
        assert bvh_check.validate_wide(nodes, wide, len(orig), nf) == sc.stat("wide_pending")


@pytest.mark.parametrize("case", bs.CASES, ids=bs.CASE_IDS)
def test_expected_column_follows_from_the_host_builder(api, specs, case):
    spec = specs[case.id]
    finite = all(np.isfinite(o[0]).all() for o in spec.objects)
    assert finite == (case.dropped == 0)
    for policy in HOST_POLICIES + (4,):
        sc = host_scene(api, case, spec, policy)
        assert sc.stat("bvh_on_device") == 0
        n_tree = sc.stat("triangles") - sc.stat("flat_triangles")
        medians = sc.stat("bvh_median_splits")
        rule = 0 if (n_tree <= 8 or not finite or (policy != 4 and medians > 0)) else 1
        assert case.expected(policy if policy else 5) == rule, "policy %d: %d median splits" % (policy, medians)


@pytest.mark.parametrize("case", bs.CASES, ids=bs.CASE_IDS)
def test_oracle_searches_agree_and_hit(oracle, specs, case):
    """orc_kd_intersect mode 2 is the exhaustive search, mode 0 the oracle's own traversal of the reference's tree"""
    spec = specs[case.id]
    rays = bs.rays(case, spec)
    assert rays.shape == (bs.N_RAYS,) and np.isfinite(rays["P"]).all() and np.isfinite(rays["D"]).all()
    osc = oracle.load_scene(spec)
    brute = osc.closest_hit(rays.view(oracle.RAY), mode=2)
    own = osc.closest_hit(rays.view(oracle.RAY), mode=0)
    hits = int((brute["t"] > 0).sum())
    print("%s: %d of %d rays hit (%d of the random half)" % (case.id, hits, bs.N_RAYS, int((brute["t"][:bs.N_RAYS // 2] > 0).sum())))
    assert hits >= bs.N_RAYS // 4
    assert np.array_equal(brute["t"].view(np.uint32), own["t"].view(np.uint32))
    assert np.array_equal(brute["N"].view(np.uint32), own["N"].view(np.uint32)) and np.array_equal(brute["mati"], own["mati"])
    # ... and the frame the GPU tests render is not empty: some camera ray hits a triangle and goes on
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, 32, 24)
    assert oracle.OracleFrame(32, 24).render(osc, cam, 6, 0, 3, mode=2, nthreads=4) > 32 * 24 * 3
