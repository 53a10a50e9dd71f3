"""-m "not gpu": which triangles of the big-triangle list the host pairs for the one-evaluation test of Trav::flat_pass
(pt_builder.cpp plan_flat_pairs), read through pt_debug_flat_list on host-only contexts, and that pairing leaves the packed
scene alone: packets, ranks, meta and order equal the lists frozen in tests/golden/wallpair_lists.npz (wallpair_scenes.py)."""
import numpy as np
import pytest

import wallpair_scenes as ws


@pytest.fixture(scope="module")
def cases(api, cb_spec):
    out = {}
    for name, (spec, pert) in ws.host_cases(cb_spec).items():
        sc = ws.load_host_only(api, spec, pert)
        out[name] = (sc, ws.packed_list(sc), sc.debug_flat_list())
    return out


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def heads(mask):
    return [i for i in range(32) if mask >> i & 1]


def check_pairs(listed, packed, mask):
    """every marked pair: neighbours, same N words, same r1 words; every listed triangle: its packet with the corners rotated"""
    hs = heads(mask)
    for a, b in zip(hs, hs[1:]):
        assert b >= a + 2, "a triangle in two pairs"
    for i in hs:
        assert i + 1 < listed.shape[0]
        assert np.array_equal(words(listed[i, 9:12]), words(listed[i + 1, 9:12])), "N words of pair %d" % i
        assert np.array_equal(words(listed[i, 0:3]), words(listed[i + 1, 0:3])), "r1 words of pair %d" % i
    for k in range(listed.shape[0]):
        c, p = listed[k, :9].reshape(3, 3), packed[k, :9].reshape(3, 3)
        assert any(np.array_equal(words(c), words(np.roll(p, -r, axis=0))) for r in range(3)), "triangle %d is not a rotation of its packet" % k
        assert np.array_equal(listed[k, 9:12], packed[k, 9:12]), "N of triangle %d" % k           # (== : the sign of a zero may differ)
        if not any(k in (i, i + 1) for i in hs):
            assert np.array_equal(words(listed[k]), words(packed[k])), "unpaired triangle %d is not as packed" % k


def test_cornell_box_walls_form_six_pairs(cases):
    sc, packed, (listed, mask) = cases["cornell"]
    assert sc.stat("flat_triangles") == 12 and sc.stat("flat_boxes") == 6
    assert heads(mask) == [0, 2, 4, 6, 8, 10]
    check_pairs(listed, packed["tris"], mask)


def test_swapped_halves_pair_too(cases):
    sc, packed, (listed, mask) = cases["swapped"]
    assert heads(mask) == [0, 2, 4, 6, 8, 10]
    check_pairs(listed, packed["tris"], mask)


def test_tilted_wall_stays_unpaired(cases):
    """its halves share the diagonal but not r1, and on a plane that is not axis-aligned no other corner may stand in for r1"""
    sc, packed, (listed, mask) = cases["tilted"]
    assert sc.stat("flat_triangles") == 12 and sc.stat("flat_boxes") == 6
    assert heads(mask) == [0, 4, 6, 8, 10]
    check_pairs(listed, packed["tris"], mask)


def test_one_ulp_in_a_normal_unpairs_a_quad(cases):
    sc, packed, (listed, mask) = cases["quad"]
    assert np.array_equal(packed["orig"][:2], [0, 1]) and heads(mask) == [0]
    check_pairs(listed, packed["tris"], mask)
    sc, packed, (listed, mask) = cases["quad_ulp"]
    assert np.array_equal(packed["orig"][:2], [0, 1]) and mask == 0
    assert np.array_equal(words(listed), words(packed["tris"]))


def test_lone_big_triangle_has_no_pair(cases):
    sc, packed, (listed, mask) = cases["lone"]
    assert packed["orig"][0] == 0 and sc.stat("flat_triangles") >= 1 and mask == 0
    assert np.array_equal(words(listed), words(packed["tris"]))


@pytest.mark.parametrize("name", ["cornell", "tilted", "swapped", "quad", "quad_ulp", "lone"])
def test_packed_scene_is_what_it_was_before_pairing(cases, name):
    """packets of the list, ranks and meta of every triangle, packed order: the frozen lists"""
    g = np.load(ws.GOLDEN)
    _, packed, _ = cases[name]
    assert int(packed["n_flat"]) == int(g[name + "_n_flat"])
    assert np.array_equal(words(packed["tris"]), words(g[name + "_tris"]))
    assert np.array_equal(packed["meta"], g[name + "_meta"]) and np.array_equal(packed["orig"], g[name + "_orig"])
