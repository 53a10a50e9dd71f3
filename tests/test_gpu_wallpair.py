"""-m gpu: the big-triangle list with its coplanar pairs tested in one evaluation (Trav::flat_pass, tri_test_pair) against
the CPU oracle: colors and final LCG state bit for bit, and the segment count, at 64x64, 4 bounces, 4 spp -- the paired
path under every schedule and in the wavefront variant, a wall that stays unpaired next to paired ones, a wall whose
halves come in the other order (a hit on the diagonal ties between them: the lower encounter rank must win, as in the
oracle), and a two-tile frame."""
import os

import numpy as np
import pytest

import wallpair_scenes as ws

pytestmark = pytest.mark.gpu

W = H = 64
BOUNCES, SPP = 4, 4


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_frame(oracle, osc, spec, w, h):
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, w, h)
    fr = oracle.OracleFrame(w, h)
    segs = fr.render(osc, cam, BOUNCES, 0, SPP, nthreads=16)
    return fr.colors()[:, :3].copy(), fr.rnds().copy(), int(segs)


@pytest.fixture(scope="module")
def refs(oracle, cb_spec, cb_oracle_scene):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "cb_64x64_b4_s4.npz"))
    out = {"cornell": (cb_spec, (g["colors"], g["rnds"], int(g["segments"])))}
    for name, spec in (("tilted", ws.tilted_wall(cb_spec)), ("swapped", ws.swapped_halves(cb_spec))):
        out[name] = (spec, oracle_frame(oracle, oracle.load_scene(spec), spec, W, H))
    out["two_tiles"] = (cb_spec, oracle_frame(oracle, cb_oracle_scene, cb_spec, 16, 8))
    return out


def render_and_check(api, spec, ref, w, h, pairs, **options):
    sc = api.Scene(w, h)
    for k, v in options.items():
        sc.set_option(k, v)
    sc.load(spec)
    assert sc.stat("node_mode") == 0                       # the whole tree in LDS: the path that tests pairs
    assert bin(sc.debug_flat_list()[1]).count("1") == pairs
    sc.iterations = BOUNCES
    sc.render(SPP)
    cols, rnds, segs = ref
    assert np.array_equal(sc.read_rnds(), rnds), "%d pixels consumed a different number of draws" % int((sc.read_rnds() != rnds).sum())
    assert np.array_equal(words(sc.read_colors()[:, :3]), words(cols)), "colors differ in bits"
    assert sc.stat("segments") == segs and sc.stat("samples") == w * h * SPP


@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_cornell_box_paired_walls(api, refs, schedule):
    spec, ref = refs["cornell"]
    render_and_check(api, spec, ref, W, H, 6, schedule=schedule)


def test_unpaired_wall_next_to_paired_ones(api, refs):
    spec, ref = refs["tilted"]
    render_and_check(api, spec, ref, W, H, 5)


def test_halves_in_swapped_order(api, refs):
    spec, ref = refs["swapped"]
    render_and_check(api, spec, ref, W, H, 6)


def test_two_tile_frame_migrating_schedule(api, refs):
    spec, ref = refs["two_tiles"]
    render_and_check(api, spec, ref, 16, 8, 6, schedule=2)


def test_wavefront_variant(api, refs):
    spec, ref = refs["cornell"]
    render_and_check(api, spec, ref, W, H, 6, variant=1)
