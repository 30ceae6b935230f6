"""The layer sampling without a GPU: the numpy restatement of GridMap::atPosition (tests/grid_sample_restate.py) against the
values the reference's own tests hold (GridMapTest.cpp:448-494), against the seven analytic surfaces of its cubic tests at
their own bound of 1e-3, and, for the linear method, against scipy; then the header the kernel runs
(lio-slam_amd/csrc/lio_gridsample.h over the geometry of lio_gridmath.h, through tools/grid_sample_host_check.cpp) against the
restatement, bit for bit."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_restate as R                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


def types_map():
    """GridMapTest.cpp:450-461"""
    layer = np.array([[0.5, 3.8, 2.0], [2.1, 1.0, 2.0], [1.0, 2.0, 2.0]], f32)
    return R.Geometry(3, 3, 1.0), R.Layer(layer)


def test_reference_held_values():
    g, layer = types_map()
    v, m = R.at_position(g, layer, (1.35, -0.4))
    assert float(v) == float(f32(3.8)) and m == R.NEAREST
    v, m = R.at_position(g, layer, (-0.3, 0.0))
    assert float(v) == 1.0 and m == R.NEAREST
    v, m = R.at_position(g, layer, (-0.5, -1.2), R.LINEAR)     # close to the border: reverting to nearest
    assert float(v) == 2.0 and m == R.NEAREST
    v, m = R.at_position(g, layer, (-0.5, 0.0), R.LINEAR)
    assert float(v) == 1.5 and m == R.LINEAR
    v, m = R.at_position(g, layer, (0.69, 0.38), R.LINEAR)
    print("linear (0.69, 0.38)", float(v))
    assert abs(float(v) - 2.19632) <= 1e-7 and m == R.LINEAR


def test_edges_outside_and_the_labelled_deviations():
    g, layer = types_map()
    # the high edge is inside, the low edge is not; nothing is read outside
    for p, want in (((1.5, 1.5), R.NEAREST), ((1.5, 0.0), R.NEAREST), ((-1.5, 0.0), R.OUTSIDE), ((0.0, -1.5), R.OUTSIDE), ((1.6, 0.0), R.OUTSIDE),
                    ((float("nan"), 0.0), R.OUTSIDE), ((0.0, float("inf")), R.OUTSIDE)):
        for method in range(4):
            v, m = R.at_position(g, layer, p, method)
            if want == R.OUTSIDE:
                assert m == R.OUTSIDE and np.array([v], f32).view(u32)[0] == R.QNAN_BITS, (p, method)
            else:
                assert m != R.OUTSIDE, (p, method)
    # cell (0, 2), up and to the right of its centre: the taps are (0, 2), (-1, 2) -> linear index 5, (0, 3) -> 9 = rows * cols,
    # (-1, 3) -> 8.  The reference lets 9 pass and reads past the buffer; here the query falls back to nearest
    v, m = R.at_position(g, layer, (1.2, -1.2), R.LINEAR)
    assert m == R.NEAREST and float(v) == 2.0
    # the wrap that stays inside the buffer: cell (2, 0) below its centre reads (3, 0) -> linear index 3 = cell (0, 1)
    v, m = R.at_position(g, layer, (-1.2, 1.2), R.LINEAR)
    assert m == R.NEAREST                                      # (its column neighbour (2, -1) is negative: fails)
    v, m = R.at_position(g, layer, (-1.2, 0.8), R.LINEAR)      # taps (2, 0), (3, 0) -> (0, 1), (2, 1), (3, 1) -> (0, 2)
    assert m == R.LINEAR
    # tap 0 is (3, 1): outside the grid, so `point` stays the centre of (2, 0) = (-1, 1) and t = (-0.2, -0.2)
    taps = [2.0, 2.0, float(f32(3.8)), 1.0]                    # (0, 2), (2, 1), (0, 1), (2, 0) in idxShift order 3, 2, 1, 0
    tx = ty = (-1.2 - -1.0) / 1.0
    want = taps[0] * (1 - tx) * (1 - ty) + taps[1] * tx * (1 - ty) + taps[2] * (1 - tx) * ty + taps[3] * tx * ty
    assert float(v) == float(f32(want)), (float(v), want)
    # the clamped border mode never wraps and never fails
    v, m = R.at_position(g, layer, (1.2, -1.2), R.LINEAR, border=1)
    assert m == R.LINEAR and float(v) == 2.0                   # all four taps are cell (0, 2)


WORLD_ERRORS = {}


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", list(R.WORLDS))
def test_analytic_worlds(kind, seed):
    """CubicInterpolationTest.cpp and CubicConvolutionInterpolationTest.cpp: both cubic methods within the reference's own
    maxAbsErrorValue of the analytic surface, 1000 points at least 3 cells from the edges"""
    g, layer, f, pts = R.analytic_world(kind, seed)
    truth = f(pts[:, 0], pts[:, 1])
    for method in (R.CUBIC_CONVOLUTION, R.CUBIC):
        vals, used, _ = R.sample(g, [layer], pts, method)
        err = float(np.abs(vals[0].astype(np.float64) - truth).max())
        WORLD_ERRORS[(kind, seed, method)] = err
        print(kind, "seed", seed, "method", method, "max abs error", err)
        assert (used == method).all()
        assert err <= R.MAX_ABS_ERROR, (kind, seed, method, err)


def test_linear_against_scipy():
    from scipy.interpolate import RegularGridInterpolator
    rng = np.random.default_rng(5)
    g = R.Geometry(12, 9, 0.2, (0.7, -1.3))
    layer = rng.uniform(-2.0, 2.0, g.size).astype(f32)
    xs = np.array([R.position_from_index(g, (i, 0))[0] for i in range(12)])
    ys = np.array([R.position_from_index(g, (0, j))[1] for j in range(9)])
    interp = RegularGridInterpolator((xs[::-1], ys[::-1]), layer[::-1, ::-1].astype(np.float64))
    pts = np.c_[rng.uniform(xs[-1] + 1e-9, xs[0] - 1e-9, 2000), rng.uniform(ys[-1] + 1e-9, ys[0] - 1e-9, 2000)]      # between the outermost centres
    vals, used, _ = R.sample(g, [layer], pts, R.LINEAR)
    err = float(np.abs(vals[0] - interp(pts)).max())
    print("linear against scipy, max abs difference", err)
    assert (used == R.LINEAR).all() and err <= 1e-6


def holes_layer(rows, cols, seed):
    rng = np.random.default_rng(seed)
    a = (1.0 + np.arange(rows * cols).reshape(rows, cols) * 0.37 + rng.uniform(0, 0.1, (rows, cols))).astype(f32)
    k = a.size
    a.flat[1 % k] = np.nan
    a.flat[k // 2] = np.inf
    a.flat[k - 2] = -np.inf
    a.view(u32).flat[3 % k] = 0xffc01234                        # a NaN with a payload
    return a


def test_fall_back_chain_on_holes():
    g = R.Geometry(12, 9, 0.2)
    layer = R.Layer(holes_layer(12, 9, 3))
    pts = R.border_lattice(g)
    for method in (R.CUBIC_CONVOLUTION, R.CUBIC):
        vals, used, info = R.sample(g, [layer], pts, method)
        inside = used != R.OUTSIDE
        assert set(np.unique(used[inside])) == {R.NEAREST, R.LINEAR, method}
        assert np.isfinite(vals[used == method]).all()         # a cubic result is finite or it is not used
        assert info["n_outside"] + sum(info["n_method"]) == len(pts)
    vals, used, _ = R.sample(g, [layer], pts, R.NEAREST)
    hit = vals.view(u32) == 0xffc01234
    assert hit.any() and (used[hit] == R.NEAREST).all()        # the payload comes through


def test_header_on_the_host_equals_the_restatement():
    """tools/grid_sample_host_check.cpp runs csrc/lio_gridsample.h and lio_gridmath.h -- the text the kernel runs -- on the host: its own run
    counts no read outside a layer, and its `dump` mode equals the restatement on the border lattice, for every method and both
    border modes, values as words (NaN for NaN where a method computed it) and method bytes"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grid_sample_host_check")
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                               os.path.join(ROOT, "tools", "grid_sample_host_check.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        print(out.stdout[-600:])
        assert out.returncode == 0 and "out-of-range accesses: 0, inconsistencies: 0" in out.stdout
        cases = [(1, 1, 0.2, (0.0, 0.0), False), (2, 2, 0.2, (0.0, 0.0), False), (1, 7, 0.2, (0.0, 0.0), False), (5, 4, 0.2, (0.0, 0.0), False),
                 (4, 5, 0.2, (0.0, 0.0), False), (5, 4, 0.2, (0.0, 0.0), True), (12, 9, 0.2, (1e4, -3e4), True), (3, 3, 1.0, (0.0, 0.0), False),
                 (5, 4, 0.25, (0.25, -0.125), False)]
        for rows, cols, res, pos, holes in cases:
            g = R.Geometry(rows, cols, res, pos)
            a = holes_layer(rows, cols, rows * 10 + cols) if holes else (1.0 + np.arange(rows * cols).reshape(rows, cols) * 0.37).astype(f32)
            pts = R.border_lattice(g)
            a.ravel(order="F").tofile(os.path.join(d, "layer"))
            pts.tofile(os.path.join(d, "pos"))
            layer = R.Layer(a)
            for method in range(4):
                for border in (0, 1):
                    subprocess.check_call([exe, "dump", str(rows), str(cols), repr(res), repr(pos[0]), repr(pos[1]), str(method), str(border),
                                           os.path.join(d, "layer"), os.path.join(d, "pos"), str(len(pts)), os.path.join(d, "out")],
                                          stdout=subprocess.DEVNULL)
                    raw = open(os.path.join(d, "out"), "rb").read()
                    got_v = np.frombuffer(raw[:4 * len(pts)], f32)
                    got_m = np.frombuffer(raw[4 * len(pts):], np.uint8)
                    vals, used, _ = R.sample(g, [layer], pts, method, border)
                    what = (rows, cols, method, border)
                    assert np.array_equal(got_m, used[0]), what
                    same = (got_v.view(u32) == vals[0].view(u32)) | (np.isnan(got_v) & np.isnan(vals[0]) & (used[0] != R.NEAREST) & (used[0] != R.OUTSIDE))
                    assert same.all(), (what, "first at", int(np.argmin(same)), pts[int(np.argmin(same))])
