"""The table of k_nee instances and its scenes on host-only contexts (tests/nee_instances.py; the GPU side is
tests/test_gpu_nee_instances.py): no device needed."""

import numpy as np
import pytest

import nee_instances as I


def test_cells_hold_each_of_the_144_instances_once():
    keys = [(c.family, c.form, c.mode) for c in I.CELLS]
    assert len(keys) == 144 and len(set(keys)) == 144
    assert set(keys) == {(f, form, mode) for f in range(9) for form in range(4) for mode in range(4)}
    assert len(I.FAMILIES) == 9 and len(I.FORMS) == 4 and len(I.CONFIGS) == 10
    for c in I.CELLS:
        assert c.scenes and set(c.scenes) <= set(I.PLACEMENTS)
        for s in c.scenes:                          # (that the placement reaches the mode: test_every_placement_reaches_its_node_mode)
            assert c.mode in {m for _, _, m in I.PLACEMENTS[s].values()}
        assert c.block == {0: 512, 1: 256, 3: 256}.get(c.mode, c.block)
    # the treelet column, against launch_nee read by eye: plain has no 512-thread form, smooth one (_env_tiles), tex two (_env and
    # _env_tiles), every family from glossy on all four
    treelet = {(c.family, c.form): c.block for c in I.CELLS if c.mode == 2}
    assert [treelet[(0, f)] for f in range(4)] == [1024, 1024, 1024, 1024]
    assert [treelet[(1, f)] for f in range(4)] == [1024, 1024, 1024, 512]
    assert [treelet[(2, f)] for f in range(4)] == [1024, 512, 1024, 512]
    assert all(treelet[(fam, f)] == 512 for fam in range(3, 9) for f in range(4))
    # every configuration selects its family's features, and the chain of "differs from the one below" reaches plain
    assert [I.family_of(c) for c in I.CONFIGS] == list(range(9)) + [8]
    assert I.features("plain") == () and I.features("medium") == I.FEATURES and I.features("medium_alone") == ("medium",)
    assert [I.below(c) for c in I.CONFIGS] == [None] + list(I.FAMILIES[:8]) + ["plain"]


def test_the_specs_are_well_formed(api):
    from opencl_path_tracer_amd import scenes
    small, mesh, anchor = I.small_spec(), I.mesh_spec(), I.mesh_spec(rich=False)
    assert small.ntris == 1932 and small.ntris < 4096 < mesh.ntris == anchor.ntris == 6062

    def types_used(spec):
        mo = np.concatenate([m for _, m in spec.objects])
        return {int(spec.materials[int(m)][6]) for m in np.unique(mo)}
    assert types_used(small) == {0, 1, 2, 3, 4, 5, 6} and types_used(mesh) == {0, 1, 2, 3, 4, 5, 6} and types_used(anchor) == {0, 1, 2, 3, 4}
    for spec in (small, mesh, anchor):
        mo = np.concatenate([m for _, m in spec.objects])
        assert mo.dtype == np.uint16 and int(mo.max()) < len(spec.materials)
    # the bands of the mesh are of equal size, in face order
    band = mesh.objects[1][1]
    assert (np.diff(np.nonzero(np.diff(band.astype(int)))[0]) >= 6050 // 6).all() and len(np.unique(band)) == 6
    # normals and uvs, per object, in the shape Scene.load takes
    assert len(small.normals) == 3 and small.normals[0] is None
    for k in (1, 2):
        assert small.normals[k].shape == small.objects[k][0].shape and small.normals[k].dtype == np.float32
    assert small.uvs[0].shape == (12, 3, 2) and np.isfinite(small.uvs[0][-2:]).all() and np.isnan(small.uvs[0][:-2]).all()
    assert mesh.uvs[0] is None and mesh.uvs[1].shape == (6050, 3, 2) and mesh.uvs[1].dtype == np.float32
    # (x, z) / 1000 of a grid over x in [0, 1000], z in [-600, 800]: v wraps below 0, as the Cornell floor's uvs do
    assert mesh.uvs[1].min() == np.float32(-0.6) and mesh.uvs[1].max() == 1.0 and mesh.material_textures == {scenes.WHITE_DIFFUSE: 0}
    assert mesh.textures[0][1] == dict(filter=1, srgb=0) and small.textures[0][1]["filter"] == 0
    assert not anchor.uvs and not anchor.textures
    # what a configuration without a feature loads has none of its data
    bare = I.scene_spec("small", False, False)
    assert not bare.normals and not bare.uvs and not bare.textures and not bare.material_textures
    assert I.scene_spec("mesh", True, False).uvs == [] and len(I.scene_spec("mesh", False, True).uvs) == 2
    # on a context: the mesh's computed normals cover the mesh and only it; the uvs arrive
    sc, _ = I.build(api, "mesh", "medium", "treelet", sky=True, device=None)
    vn, has = sc.debug_vertex_normals()
    assert vn.shape == (6062, 3, 3) and has[12:].all() and not has[:12].any()
    sc, _ = I.build(api, "small", "medium", "lds", device=None)
    assert sc.debug_vertex_normals()[1].sum() == 1920
    sc, _ = I.build(api, "small", "medium_alone", "lds", device=None)
    assert sc.debug_vertex_normals()[1].sum() == 0 and sc.medium()["sigma_t"] > 0


@pytest.mark.parametrize("scene,placement", [(s, p) for s in sorted(I.PLACEMENTS) for p in sorted(I.PLACEMENTS[s])])
def test_every_placement_reaches_its_node_mode(api, scene, placement):
    """with the options the GPU test sets, for the poorest and the richest configuration (what a configuration adds is authoring data
    and options that do not move nodes)"""
    for config in ("plain", "medium"):
        sc, mode = I.build(api, scene, config, placement, device=None)
        assert sc.stat("node_mode") == mode, config
        if placement == "treelet":
            assert sc.stat("treelet_nodes") == 40
        if placement == "wide_overflow":          # wide_stack_entries(pending): ((pending + 4) + 1) & ~1 entries, of which 6 stay in LDS
            assert ((int(sc.stat("wide_pending")) + 5) & ~1) > I.OVERFLOW_LDS_ENTRIES
    sc, mode = I.build_anchor(api, "treelet", True, device=None)[:2]
    assert sc.stat("node_mode") == mode == 2 and sc.debug_lights()["P_ana"] == I.ANCHOR["select"]


def test_the_new_stats_read_minus_one_on_a_fresh_context(api):
    sc, _ = I.build(api, "small", "medium", "lds", device=None)
    assert [sc.stat(k) for k in ("nee_family", "nee_form", "nee_block")] == [-1.0, -1.0, -1.0]
    sc.iterations = 4
    with pytest.raises(api.PtError) as e:           # a refused launch records nothing
        sc.render_nee(1, "mis")
    assert e.value.code == api.PT_ENODEVICE
    assert [sc.stat(k) for k in ("nee_family", "nee_form", "nee_block")] == [-1.0, -1.0, -1.0]
