"""-m gpu: the device BVH builders (pt_lbvh.hip, pt_sahdev.hip) and the device 4-wide collapse (pt_widedev.hip) on the small and
degenerate scenes of builder_scenes.py: tree sizes on either side of a wave, a block, two blocks and PLOC's tile; zero-area
triangles, flat meshes, coincident box centres, exact duplicates, clusters 1e4 diameters apart, huge and non-finite coordinates,
and a big-triangle list in front of a very small tree.

The closest hit does not depend on the tree, so every comparison is a bit equality: the SAH builder
against the host builder's tree, node for node; every device-built tree against the oracle's exhaustive search on the case's
2,048 fixed rays and against the host-built context's render.  Where a case must be built (1: on the device, 0: handed back to the
host) is the case table's column, which test_builder_scenes_host.py derives from the host builder; a build that ends up elsewhere
fails here."""
import numpy as np
import pytest

import builder_scenes as bs
import bvh_check

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 32, 24, 3, 6
SAH_GRAINS = (8, 64, 4096)          # (almost) everything through the level-synchronous top phase ... everything in one bottom wave
LBVH_CONFIGS = [(ploc, cluster) for ploc in (0, 8, 16, 32) for cluster in (0, 8, 64)]


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class CaseData:
    """a case's scene as triangle records, its rays and what the oracle's exhaustive search (orc_kd_intersect mode 2) finds"""

    def __init__(self, api, oracle, case):
        self.case, self.spec = case, case.spec()
        self.records = [api.triangles_from_vertices(v, m) for v, m in self.spec.objects]
        self.tris = np.concatenate(self.records)
        self.rays = bs.rays(case, self.spec)
        osc = oracle.load_scene(self.spec)
        hit = osc.closest_hit(self.rays.view(oracle.RAY), mode=2)
        self.t = np.where(hit["t"] > 0, hit["t"], np.float32(-1))
        self.hit = self.t > 0
        self.N, self.mati = hit["N"][:, :3], hit["mati"]
        # among triangles that are the same bit for bit the oracle's tie goes to the one the reference meets first
        corners = np.ascontiguousarray(np.stack([self.tris["r1"], self.tris["r2"], self.tris["r3"]], 1)).view(np.uint32).reshape(len(self.tris), -1)
        _, group = np.unique(corners, axis=0, return_inverse=True)
        rank = osc.encounter_rank()
        first = np.full(group.max() + 1, np.iinfo(np.int32).max, dtype=np.int64)
        np.minimum.at(first, group.reshape(-1), rank)
        self.meets_first = rank == first[group.reshape(-1)]

    def scene(self, api, **options):
        sc = self.case.configure(api.Scene(W, H))
        for k, v in options.items():
            sc.set_option(k, v)
        for m in self.spec.materials:
            sc.add_Material(*m)
        for r in self.records:
            sc.add_Triangles(r)
            sc.end_Obj()
        sc.upload_Triangles()
        sc.upload_Materials()
        sc.set_view(self.spec.fov, self.spec.yaw, self.spec.pitch, self.spec.shift)
        return sc

    def check_hits(self, sc, mode, what):
        assert sc.stat("node_mode") == mode, what
        t, tri = sc.debug_closest_hit(self.rays)
        assert np.array_equal(words(t), words(self.t)), "%s, node mode %d: t differs on %d rays" % (what, mode, int((words(t) != words(self.t)).sum()))
        assert np.array_equal(tri >= 0, self.hit)
        got = self.tris[tri[self.hit]]
        assert np.array_equal(words(got["N"][:, :3]), words(self.N[self.hit])) and np.array_equal(got["mati"], self.mati[self.hit]), what
        assert self.meets_first[tri[self.hit]].all(), "%s: a later copy of a duplicated triangle won the tie" % what


_DATA = {}


@pytest.fixture
def data(api, oracle, request):
    case = request.getfixturevalue("case")
    if case.id not in _DATA:
        _DATA.clear()                      # (cases come grouped: one at a time is kept)
        _DATA[case.id] = CaseData(api, oracle, case)
    return _DATA[case.id]


def snapshot(sc):
    return dict(stats={k: sc.stat(k) for k in ("bvh_nodes", "bvh_depth", "flat_triangles", "wide_pending", "triangles")}, bvh=sc.debug_bvh(),
                wide=sc.debug_wide_nodes().tobytes())


def assert_same_scene(got, ref, what):
    assert got["stats"] == ref["stats"], what
    (an, at, am, ao), (bn, bt, bm, bo) = ref["bvh"], got["bvh"]
    assert np.array_equal(ao, bo), "%s: packed triangle order" % what
    assert an.shape == bn.shape and np.array_equal(words(an), words(bn)), "%s: nodes" % what
    assert np.array_equal(words(at), words(bt)) and np.array_equal(am, bm), "%s: packets / meta" % what
    assert got["wide"] == ref["wide"], "%s: 4-wide nodes" % what


def render(sc):
    sc.iterations = BOUNCES
    sc.render(SPP)
    return sc.read_colors().copy(), sc.stat("segments")


@pytest.fixture
def host(api, data):
    """the host builder's contexts of the three SAH trees (4-wide nodes built: wide_nodes 2), and the frame all builds must render"""
    out = {}
    for tp in (0, 2, 3):
        sc = data.scene(api, bvh_device=0, bvh_policy=tp, wide_nodes=2)
        assert sc.stat("bvh_on_device") == 0
        out[tp] = snapshot(sc)
        if tp == 0:
            data.check_hits(sc, 3, "host builder")
            out["colors"], out["segments"] = render(sc)
            assert np.isfinite(out["colors"]).all() and out["segments"] > W * H * SPP, "no ray of the reference frame hits anything"
    return out


def check_modes_and_render(api, data, host, what, **options):
    """a build's closest hits in node modes 3 (the context given: wide_nodes 2), 0 and 1 (a second build without 4-wide nodes), its frame"""
    sc = data.scene(api, wide_nodes=2, **options)
    data.check_hits(sc, 3, what)
    colors, segments = render(sc)
    assert np.array_equal(words(colors), words(host["colors"])), "%s: the frame differs from the host-built context's" % what
    assert segments == host["segments"], what
    flat = data.scene(api, wide_nodes=0, **options)
    assert flat.stat("bvh_on_device") == sc.stat("bvh_on_device")
    data.check_hits(flat, 0, what)                     # (every tree here fits LDS)
    flat.set_option("lds_scene", 0)
    data.check_hits(flat, 1, what)
    return sc


@pytest.mark.parametrize("case", bs.CASES, ids=bs.CASE_IDS)
def test_sah_builder(api, data, host, case):
    """bvh_policy 5 / 2 / 3 with bvh_device 1 at three grains: the host builder's tree node for node, its 4-wide nodes byte for byte
    whether they are collapsed on the device or on the host -- or, where the table says so, handed back"""
    for policy in bs.SAH_POLICIES:
        ref = host[0 if policy == 5 else policy]
        for grain in SAH_GRAINS:
            what = "%s policy %d grain %d" % (case.id, policy, grain)
            opts = dict(bvh_policy=policy, bvh_device=1, sah_grain=grain)
            sc = check_modes_and_render(api, data, host, what, **opts)
            assert sc.stat("bvh_on_device") == case.expected(policy), what
            assert_same_scene(snapshot(sc), ref, what)
            other = data.scene(api, wide_nodes=2, wide_on_device=0, **opts)
            assert other.stat("bvh_on_device") == case.expected(policy), what
            assert_same_scene(snapshot(other), ref, what + " wide_on_device 0")


@pytest.mark.parametrize("case", bs.CASES, ids=bs.CASE_IDS)
def test_lbvh_builder(api, data, host, case):
    """bvh_policy 4: Karras' radix tree and PLOC at every radius, with and without the SAH top over clusters: a valid tree over all
    triangles, valid 4-wide nodes -- or, where the table says so, the host's scene"""
    for ploc, cluster in LBVH_CONFIGS:
        what = "%s lbvh_ploc %d lbvh_cluster %d" % (case.id, ploc, cluster)
        sc = check_modes_and_render(api, data, host, what, bvh_policy=4, lbvh_ploc=ploc, lbvh_cluster=cluster)
        assert sc.stat("bvh_on_device") == case.lbvh, what
        if not case.lbvh:
            assert_same_scene(snapshot(sc), host[0], what)
            continue
        nodes, tris, meta, orig = sc.debug_bvh()
        ntris = case.n + case.listed
        nf = int(sc.stat("flat_triangles"))
        assert nf == case.listed and len(orig) == ntris, what
        finite = np.nonzero(np.isfinite(np.stack([data.tris["r1"], data.tris["r2"], data.tris["r3"]], 1)).all(axis=(1, 2)))[0]
        assert sorted(orig.tolist()) == finite.tolist(), "%s: orig is not a permutation of the triangles" % what
        assert np.array_equal(words(tris[:, 0:3]), words(data.tris["r1"][orig][:, :3])) and np.array_equal(meta[:, 1], data.tris["mati"][orig]), what
        depth = bvh_check.validate_structure(nodes, tris, ntris, nf)
        assert depth <= sc.stat("bvh_depth"), what
        bs.check_node_boxes(nodes, tris)
        wide = sc.debug_wide_nodes()
        assert len(wide) > 0 and bvh_check.validate_wide(nodes, wide, ntris, nf) == sc.stat("wide_pending"), what
