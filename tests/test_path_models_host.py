"""The float64 path models against their recording (tests/golden/path_models.npz, written by tests/golden/make_path_model_golden.py from
the class tower that tests/path_ref.py's PathModel replaced): every class name of the family, in every configuration the suite constructs
it in, rebuilt through the same builders on a host-only context, must return the recorded colour bits, LCG states, near-tie masks and
per-pixel event counts.  Equal, not close: the class names are configurations of one path loop, and a change to that loop that moves one
bit of one of them is a change to the reference every test_gpu_* replay is held to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_path_model_golden as MG          # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with np.load(MG.PATH) as f:
        return {k: f[k] for k in f.files}


def test_the_recording_holds_exactly_the_cases(recorded):
    assert {k.split("/")[0] for k in recorded} == set(MG.CASES)


@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_model_reproduces_its_recording(api, recorded, name):
    got = MG.record(api, name)
    want = {k: v for k, v in recorded.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        same = got[k] == want[k]
        assert same.all(), "%s: %d of %d entries differ" % (k, int((~same).sum()), same.size)
    MG.check_events(name, got)
