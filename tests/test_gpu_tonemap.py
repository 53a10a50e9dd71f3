"""-m gpu: the tone maps and the 8-bit writer on authored frames.  In one child process (torch next to the library) torch tensors
are bound as the context's frame buffer (bind_framebuffer), filled with the frames of tests/tonemap_inputs.py, and resolve_ldr(0) / resolve_ldr(1) are compared with the
oracle's reinhard_tone_map per pixel and its filt_im on a frame of the same colours -- on bits, NaN equal to NaN at the same positions;
write_ppm's bytes are compared with the numpy restatement of the quantiser.  Sizes: no interior, one interior pixel, both sides of
k_filt_im's 32 x 8 block edge.  tests/test_tonemap_host.py holds the guards of the frames."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_inputs as S
import tonemap_inputs as T
from test_tonemap_host import oracle_filt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(what, got, want):
    g, w = S.bits(got), S.bits(want)
    bad = ((g != w) & ~(np.isnan(got) & np.isnan(want))).any(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d pixels differ, first pixel %d: device %s, oracle %s" % (
            what, int(bad.sum()), bad.size, i, " ".join("%08x" % v for v in g[i]), " ".join("%08x" % v for v in w[i])))


_CHILD = r"""
import sys, time
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np, torch
torch.cuda.init()
from opencl_path_tracer_amd import api
import spec_inputs as S, tonemap_inputs as T
res = {}
for w, h in T.SIZES:
    for which, frame in ((0, T.reinhard_frame(w, h)), (1, T.median_frame(w, h))):
        t0 = time.perf_counter()
        sc = api.Scene(w, h, device=0)
        assert sc.local_pixels == w * h
        colors = torch.zeros((sc.slab_pixels, 4), dtype=torch.float32, device="cuda:0")
        rnds = torch.zeros((sc.slab_pixels,), dtype=torch.int32, device="cuda:0")
        sc.bind_framebuffer(colors.data_ptr(), rnds.data_ptr())
        assert sc.device_colors() == colors.data_ptr()
        colors[:w * h].copy_(torch.from_numpy(frame))
        torch.cuda.synchronize()
        assert np.array_equal(S.bits(sc.read_colors()), S.bits(frame))
        res["ldr_%%d_%%d_%%d" %% (which, w, h)] = sc.resolve_ldr(which)
        path = %(tmp)r + "/%%d_%%d_%%d.ppm" %% (which, w, h)
        sc.write_ppm(path, which)
        sc.close()
        torch.cuda.synchronize()
        print("[tonemap] %%s %%dx%%d: device side %%.3f s" %% (("reinhard", "filt_im")[which], w, h, time.perf_counter() - t0))
np.savez(%(tmp)r + "/ldr.npz", **res)
print("TONEMAP_CHILD_OK")
"""


@pytest.fixture(scope="module")
def device_side(tmp_path_factory):
    """One child process for every size and both maps, as the other tests that put torch next to the library do: the resolves as an
    .npz and the PPM files, in a directory of their own."""
    tmp = str(tmp_path_factory.mktemp("tonemap"))
    out = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "tmp": tmp}], capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert "TONEMAP_CHILD_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return tmp, np.load(os.path.join(tmp, "ldr.npz"))


def ppm_body(path, w, h):
    raw = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert raw[:len(head)] == head
    return raw[len(head):]


@pytest.mark.timeout(360, method="thread")
@pytest.mark.parametrize("w,h", T.SIZES)
def test_reinhard_map_on_authored_values(oracle, device_side, w, h):
    tmp, ldr = device_side
    want = oracle.reinhard_n(T.reinhard_frame(w, h))
    same_bits("resolve_ldr(0) %dx%d" % (w, h), ldr["ldr_0_%d_%d" % (w, h)], want)
    assert ppm_body(os.path.join(tmp, "0_%d_%d.ppm" % (w, h)), w, h) == T.quantise(want, w, h)


@pytest.mark.timeout(360, method="thread")
@pytest.mark.parametrize("w,h", T.SIZES)
def test_median_filter_on_authored_ties(oracle, device_side, w, h):
    tmp, ldr = device_side
    want = oracle_filt(oracle, T.median_frame(w, h), w, h)
    got = ldr["ldr_1_%d_%d" % (w, h)]
    same_bits("resolve_ldr(1) %dx%d" % (w, h), got, want)
    border = np.ones((h, w), dtype=bool)
    border[1:h - 1, 1:w - 1] = False
    assert (S.bits(got).reshape(h, w, 4)[border] == 0).all()                                        # border pixels read 0
    assert ppm_body(os.path.join(tmp, "1_%d_%d.ppm" % (w, h)), w, h) == T.quantise(want, w, h)
