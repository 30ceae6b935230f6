"""The host conversion of the association's double thresholds (plane_tol MO:1662, min_s MO:1679) to the fp32 value the kernels
compare against (lio_threshold_f32 in lio-slam_amd/csrc/lio_types.h, through the exported helper lio_debug_threshold_f32): t_f is
the largest float not above t, and for every float v

    (double)v > t   ==   v > t_f

checked on t_f itself and its neighbours on both sides, where the two comparisons could part.  No GPU needed."""
import importlib

import numpy as np
import pytest

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
DENORM = float(np.finfo(np.float32).smallest_subnormal)


@pytest.fixture(scope="module")
def tf():
    return importlib.import_module("lio-slam_amd.api").debug_threshold_f32


def _around(f):
    """f and four floats on either side of it (fewer at an infinity), plus the zeros, the extremes and the infinities."""
    out = {float(f), 0.0, -0.0, FLT_MAX, -FLT_MAX, float("inf"), float("-inf"), DENORM, -DENORM}
    for direction in (np.inf, -np.inf):
        v = F(f)
        for _ in range(4):
            v = np.nextafter(v, F(direction))
            out.add(float(v))
    return [F(v) for v in out]


def _check(tf, t):
    t_f = tf(t)
    assert isinstance(t_f, np.float32)
    if np.isnan(t):
        assert np.isnan(t_f)
        return
    # the largest float not above t
    assert float(t_f) <= t, (t, t_f)
    if np.isfinite(t_f) or t_f < 0:
        up = np.nextafter(t_f, F(np.inf))
        assert float(up) > t or (up == t_f), (t, t_f, up)
    with np.errstate(all="ignore"):
        for v in _around(t_f) + [F(np.nan)]:
            assert (float(v) > t) == bool(v > t_f), (t, t_f, v)


CASES = [0.2, 0.1,                                   # the shipped plane_tol and min_s
         0.25, 0.5,                                  # exactly representable
         0.0, -0.0, -0.2, -0.1, -0.25, -1.0, -3.7e5,
         FLT_MIN / 3, -FLT_MIN / 3, DENORM / 2, -DENORM / 2, DENORM * 0.75, 1e-50, -1e-50, 5e-324, -5e-324, DENORM, FLT_MIN,
         FLT_MAX, -FLT_MAX, FLT_MAX * (1 + 2.0 ** -30), -FLT_MAX * (1 + 2.0 ** -30), 2.0 ** 128, -2.0 ** 128, 1e300, -1e300,
         float("inf"), float("-inf"), float("nan")]


@pytest.mark.parametrize("t", CASES, ids=[repr(c) for c in CASES])
def test_threshold_cases(tf, t):
    _check(tf, t)


def test_shipped_thresholds_are_one_step_below_the_rounded_literals(tf):
    # float(0.2) and float(0.1) round UP from the double literal: the threshold is the float below
    assert tf(0.2) == np.nextafter(F(0.2), F(0)) and float(F(0.2)) > 0.2
    assert tf(0.1) == np.nextafter(F(0.1), F(0)) and float(F(0.1)) > 0.1
    assert tf(0.25) == F(0.25) and tf(0.5) == F(0.5)


def test_random_doubles(tf):
    rng = np.random.default_rng(5)
    n = 100_000
    # a quarter each: around the shipped values, wide magnitudes of either sign, exact floats, floats +- half an ulp and a bit
    a = rng.uniform(0.0, 1.0, n // 4)
    b = rng.choice([-1.0, 1.0], n // 4) * 10.0 ** rng.uniform(-50, 40, n // 4)
    with np.errstate(invalid="ignore"):                    # (signalling NaN patterns, dropped below)
        c = rng.integers(0, 1 << 32, n // 4, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)
        base = rng.integers(0, 1 << 32, n // 4, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)
    c = c[np.isfinite(c)]
    base = base[np.isfinite(base)]
    with np.errstate(all="ignore"):
        d = base * (1.0 + rng.choice([-1.0, 1.0], len(base)) * 2.0 ** rng.integers(-52, -22, len(base)))
    ts = np.concatenate([a, b, c, d])
    assert len(ts) > 99_000
    t_f = np.array([tf(float(t)) for t in ts], np.float32)
    with np.errstate(all="ignore"):
        # the largest float not above t (every t here is finite; beyond FLT_MAX the answer is FLT_MAX, below -FLT_MAX it is -inf)
        assert np.all(t_f.astype(np.float64) <= ts)
        assert np.all(np.nextafter(t_f, F(np.inf)).astype(np.float64) > ts)
        # the two comparisons agree on t_f and on four floats to either side
        for direction in (np.inf, -np.inf):
            v = t_f.copy()
            for _ in range(5):
                bad = np.flatnonzero((v.astype(np.float64) > ts) != (v > t_f))
                assert len(bad) == 0, (ts[bad[:3]], t_f[bad[:3]], v[bad[:3]])
                v = np.nextafter(v, F(direction))
