"""-m gpu: the IEEE divide / sqrt cores of pt_device.hpp (div_rn, sqrt_rn, rsqrt_rn) give the same bits as the
compiler's correctly rounded expansions wherever their windows admit an input, the windows admit no zero, denormal,
inf or NaN, and the wave-level functions (core or expansion, whichever their wave took) match on every input
(pt_debug_math).  Each enumeration has its own time limit (pytest-timeout, thread method: a hung launch ends the run), and
each call is also held to a wall-clock budget below that limit, which a slow enumeration would miss."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(api):
    return api.Scene(8, 8, device=0)


def _run(api, sc, fn, first, n, budget_s):
    t0 = time.monotonic()
    miss, inside, bad = sc.debug_math(fn, first, n)
    dt = time.monotonic() - t0
    assert dt < budget_s, "enumeration %d took %.1f s, over its %.0f s budget" % (fn, dt, budget_s)
    assert miss == 0, "%d mismatches, first inputs (bits): %s" % (miss, [tuple("%08x" % v for v in row) for row in bad])
    return inside


@pytest.mark.timeout(120, method="thread")
def test_sqrt_all_non_negative_floats(api, sc):
    # every x in [+0, +inf] and every positive NaN: 2^31 inputs
    inside = _run(api, sc, api.PT_MATH_SQRT, 0, 1 << 31, 60.0)
    assert inside == 0x7f800000 - 0x0f800000 + 1       # [2^-96, +inf]


@pytest.mark.timeout(60, method="thread")
def test_sqrt_negative_floats_take_the_expansion(api, sc):
    assert _run(api, sc, api.PT_MATH_SQRT, 1 << 31, 1 << 24, 30.0) == 0
    assert _run(api, sc, api.PT_MATH_SQRT, (1 << 32) - (1 << 24), 1 << 24, 30.0) == 0


@pytest.mark.timeout(120, method="thread")
def test_rsqrt_all_non_negative_floats(api, sc):
    inside = _run(api, sc, api.PT_MATH_RSQRT, 0, 1 << 31, 60.0)
    assert inside == 0x7f800000 - 0x0f800000         # [2^-96, FLT_MAX]


@pytest.mark.timeout(120, method="thread")
def test_div_every_exponent_pair(api, sc):
    # 256 x 256 exponent pairs (zeros, denormals, inf and NaN included) x 8 x 8 mantissas at the edges and hashed x 4 signs
    inside = _run(api, sc, api.PT_MATH_DIV_GRID, 0, 1 << 24, 60.0)
    assert inside > 0


@pytest.mark.timeout(120, method="thread")
def test_div_random_bit_patterns(api, sc):
    inside = _run(api, sc, api.PT_MATH_DIV_RANDOM, 0, 1 << 28, 60.0)
    assert inside > 0


@pytest.mark.timeout(240, method="thread")
def test_div_random_normal_pairs(api, sc):
    # 10^9 normal pairs with exponents -63 .. 63: a third or so inside the window, the rest around and outside its edges
    n = 10 ** 9
    inside = _run(api, sc, api.PT_MATH_DIV_NORMAL, 0, n, 120.0)
    assert inside > n // 10


@pytest.mark.timeout(60, method="thread")
def test_div_window_edges_pinned(api, sc):
    # the window as pt_device.hpp states it, on powers of two: |b|, |1/b| and the quotient within [2^-40, 2^40]
    k = lambda ea, eb, ia, ib, sg: ea | eb << 8 | ia << 16 | ib << 19 | sg << 22
    for ea, eb, want in [(127, 127, 1), (127 + 40, 127, 1), (127 + 41, 127, 0), (127 - 40, 127, 1), (127 - 41, 127, 0),
                         (127, 127 + 40, 1), (127, 127 + 41, 0), (127, 127 - 40, 1), (127, 127 - 41, 0), (0, 127, 0), (127, 0, 0),
                         (255, 127, 0), (127, 255, 0)]:
        assert _run(api, sc, api.PT_MATH_DIV_GRID, k(ea, eb, 0, 0, 0), 1, 10.0) == want, (ea, eb)
