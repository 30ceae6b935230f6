"""tests/sdf_restate.py (the fp32 restatement of grid_map_sdf that the GPU tests compare bits with) against the brute-force
definition written from the formula in fp64, on the shapes of grid_map_sdf/test/ and with its tolerance: 1e-4
(testSignedDistance2d.cpp, testSignedDistance3d.cpp).  No GPU."""
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdf_restate as R                                        # noqa: E402

f32 = np.float32
TOL = 1e-4                                                     # the reference's own


def random_map(seed, rows=20, cols=30):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, cols)).astype(f32)          # Matrix::Random


def check_3d(elev, h, res):
    got = R.signed_distance_at_height(elev, h, res, elev.min(), elev.max())
    ok, dev = R.is_equal_sdf(got, R.brute_force_at_height(elev, h, res), TOL)
    assert ok, (h, dev)
    return dev


def check_2d(occ, res):
    got = R.signed_distance_from_occupancy(occ, res)
    ok, dev = R.is_equal_sdf(got, R.brute_force_occupancy(occ, res), TOL)
    assert ok, dev
    return dev


def test_pixel_border_distance():
    """testPixelBorderDistance.cpp: the distance itself, and the equidistance point solves its defining equation"""
    assert R.pixel_border_distance(0, 0) == 0 and R.pixel_border_distance(0, 1) == 0.5 and R.pixel_border_distance(3, 0) == 2.5
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(2000):
        p, q = rng.integers(0, 40, 2)
        if p == q:
            continue
        fp, fq = f32(rng.uniform(0, 30)), f32(rng.uniform(0, 30))
        s = float(R.equidistance_point(f32(q), fq, f32(p), fp))
        dp = max(abs(s - p) - 0.5, 0.0) ** 2 + float(fp)
        dq = max(abs(s - q) - 0.5, 0.0) ** 2 + float(fq)
        worst = max(worst, abs(dp - dq) / max(dp, 1.0))
    assert worst < 1e-4, worst
    assert R.equidistance_point(f32(3), f32(2), f32(7), f32(2)) == 5.0                       # equal offsets: the midpoint
    # INF flows through: a finite bound against an infinite one
    assert R.equidistance_point(f32(5), f32(0), f32(2), R.INF) == -np.inf
    assert R.equidistance_point(f32(5), R.INF, f32(2), f32(0)) == np.inf


def test_flat_terrain():
    elev = np.full((3, 4), 0.5, f32)
    for h in (3.0, -3.0):
        check_3d(elev, h, 0.1)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_terrain(seed):
    elev = random_map(seed)
    worst = 0.0
    h = f32(-1.0) - f32(0.1)
    while h < f32(1.0) + f32(0.1):                             # the reference's float loop: 23 heights
        worst = max(worst, check_3d(elev, h, 0.1))
        h = f32(h + f32(0.1))
    print(f"  random 20 x 30, seed {seed}: worst deviation from the definition {worst:.2e}")


def test_step_terrain():
    """plateaus: many equal offsets (the fp == fq branch), res 0.2, sizes astride a wave"""
    r, c = np.mgrid[0:33, 0:65]
    elev = (0.4 * ((r // 7 + c // 11) % 3)).astype(f32)
    for h in (-0.1, 0.0, 0.2, 0.4, 0.5, 0.8, 1.0):
        check_3d(elev, h, 0.2)


def test_occupancy():
    assert (R.signed_distance_from_occupancy(np.zeros((3, 4), bool), 0.1) == np.inf).all()
    assert (R.signed_distance_from_occupancy(np.ones((3, 4), bool), 0.1) == -np.inf).all()
    check_2d(np.array([[0, 1, 1], [0, 0, 1]], bool), 1.0)
    one = np.zeros((20, 30), bool)
    one[10, 15] = True
    check_2d(one, 0.1)
    check_2d(~one, 0.1)
    check_2d(np.array([[1, 1, 1], [0, 1, 1], [1, 1, 0]], bool), 1.0)                          # the "debugcase"
    elev = random_map(5)
    h = f32(-1.1)
    while h < f32(1.1):
        occ = elev > h
        got = R.signed_distance_from_occupancy(occ, 1.0)
        if occ.any() and not occ.all():
            ok, dev = R.is_equal_sdf(got, R.brute_force_occupancy(occ, 1.0), TOL)
            assert ok, (h, dev)
        else:
            assert (got == (-np.inf if occ.all() else np.inf)).all()
        h = f32(h + f32(0.1))


def test_three_branches_differ_in_the_sign_of_zero_only():
    """below the minimum and above the maximum the shortcut is one transform alone: the same numbers as the mixed form"""
    elev = random_map(8, 9, 7)
    for h, mode in ((-1.5, R.ALL_OBSTACLE), (1.5, R.ALL_FREE)):
        assert R.layer_mode(h, elev.min(), elev.max()) == mode
        short = R.signed_distance_at_height(elev, h, 0.1, elev.min(), elev.max())
        mixed = R.signed_distance_at_height(elev, h, 0.1, -np.inf, np.inf)
        assert np.array_equal(short, mixed)


def test_field_and_derivatives():
    """testSignedDistance3d randomTerrainDerivative: 10 x 20, the value at every node and the three differences against
    differences of the brute-force layers, one-sided at the borders"""
    rows, cols, res = 10, 20, 0.1
    elev = random_map(11, rows, cols)
    F = R.Field(elev, res, (rows * res, cols * res), (0.0, 0.0))
    assert F.layers == max(math.ceil((float(elev.max()) - float(elev.min())) / res), 2) and F.nodes.shape == (F.layers, cols, rows, 4)
    naive = [R.brute_force_at_height(elev, h, res) for h in F.heights]
    r = float(f32(res))
    for k in range(F.layers):
        d, dx, dy, dz = (F.nodes[k, :, :, a].T for a in range(4))
        assert np.abs(d - naive[k]).max() < TOL
        n = naive[k]
        ex = np.empty_like(n)
        ex[0], ex[1:-1], ex[-1] = (n[1] - n[0]) / -r, (n[2:] - n[:-2]) / (-2 * r), (n[-1] - n[-2]) / -r
        ey = np.empty_like(n)
        ey[:, 0], ey[:, 1:-1], ey[:, -1] = (n[:, 1] - n[:, 0]) / -r, (n[:, 2:] - n[:, :-2]) / (-2 * r), (n[:, -1] - n[:, -2]) / -r
        if k == 0:
            ez = (naive[1] - naive[0]) / r
        elif k == F.layers - 1:
            ez = (naive[k] - naive[k - 1]) / r
        else:
            ez = (naive[k + 1] - naive[k - 1]) / (2 * r)
        # a difference of two values that each sit within e of the definition sits within 2 e / step of its difference;
        # the reference's test asks 1e-4 of the derivative itself
        for got, want in ((dx, ex), (dy, ey), (dz, ez)):
            assert np.abs(got - want).max() < TOL, k


def test_extrapolation_constant_terrain():
    rows, cols, res, h0 = 20, 30, 0.1, 0.5
    elev = np.full((rows, cols), h0, f32)
    F = R.Field(elev, res, (rows * res, cols * res), (0.0, 0.0), float(f32(h0) - f32(res)), float(f32(h0) + f32(res)))
    h = f32(h0 - 1.0)
    while h < f32(h0 + 1.0):
        naive = R.brute_force_at_height(elev, h, res)
        for i in range(rows):
            for j in range(cols):
                p = (F.origin[0] - i * res, F.origin[1] - j * res, float(h))
                v, der = F.value_and_derivative(p)
                assert abs(v - naive[i, j]) < TOL
                assert math.sqrt(der[0] ** 2 + der[1] ** 2 + (der[2] - 1.0) ** 2) < TOL
        h = f32(h + f32(res))


def test_host_program_runs_the_same_bits():
    """tools/sdf_host_check.cpp runs csrc/lio_sdf.h -- the text the kernels run -- on the host; its `dump` mode against the
    restatement, bit for bit, on grids astride a wave in both directions, a band of 40 layers and a filled hole"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(5)
    r, c = np.mgrid[0:65, 0:33]
    holes = rng.uniform(-1, 1, (12, 9)).astype(f32)
    holes[3, 4] = np.nan
    cases = [(rng.uniform(-1, 1, (33, 65)).astype(f32), 0.2, None, None, 0), ((0.4 * ((r // 7 + c // 11) % 3)).astype(f32), 0.2, None, None, 0),
             (rng.uniform(-1, 1, (129, 70)).astype(f32), 0.1, -2.0, 2.0, 0), (holes, 0.1, None, None, 1)]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sdf_host_check")
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", os.path.join(root, "tools", "sdf_host_check.cpp"), "-o", exe])
        for elev, res, lo, hi, policy in cases:
            rows, cols = elev.shape
            elev.T.tofile(os.path.join(d, "in.f32"))                                           # column-major
            band = ["nan" if v is None else repr(v) for v in (lo, hi)]
            out = subprocess.check_output([exe, "dump", str(rows), str(cols), repr(res), *band, str(policy), os.path.join(d, "in.f32"),
                                           os.path.join(d, "out.f32")], text=True).split()
            F = R.Field(elev, res, (rows * res, cols * res), (0.0, 0.0), lo, hi, nan_fill=bool(policy))
            assert (int(out[2]), int(out[3])) == (F.layers, 0)                                 # the layers; no out-of-range access
            got = np.fromfile(os.path.join(d, "out.f32"), f32).reshape(F.nodes.shape)
            assert np.array_equal(got.view(np.uint32), F.nodes.view(np.uint32)), (rows, cols)


def test_nan_fill_reads_as_the_smallest_elevation():
    elev = random_map(13, 8, 9)
    holes = elev.copy()
    holes[2, 3] = np.nan
    holes[7, 0] = np.inf
    filled = holes.copy()
    filled[~np.isfinite(holes)] = holes[np.isfinite(holes)].min()
    a = R.Field(holes, 0.1, (0.8, 0.9), (1.0, 2.0), nan_fill=True)
    b = R.Field(filled, 0.1, (0.8, 0.9), (1.0, 2.0))
    assert a.n_nan == 2 and b.n_nan == 0 and np.array_equal(a.nodes, b.nodes)


def test_lookup():
    """std::round at exact halves, the clamp on all six sides, the linear index, layer heights"""
    assert [R.std_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, -0.49999999999999994)] == [1.0, 2.0, 3.0, -1.0, -2.0, 0.0, -0.0]
    assert R.nearest_index(0.5, 4) == 1 and R.nearest_index(2.5, 4) == 3 and R.nearest_index(-0.5, 4) == 0
    assert R.nearest_index(1e300, 4) == 4 and R.nearest_index(-1e300, 4) == 0 and R.nearest_index(float("nan"), 4) == 0
    assert R.nearest_index(float("inf"), 4) == 4 and R.nearest_index(float("-inf"), 4) == 0
    elev = random_map(17, 4, 5)
    F = R.Field(elev, 0.5, (2.0, 2.5), (10.0, -3.0), -1.0, 1.0)
    assert F.layers == 4 and F.origin == (10.0 + (1.0 - 0.25), -3.0 + (1.25 - 0.25), -1.0)
    ox, oy, oz = F.origin
    assert F.nearest_node((ox, oy, oz)) == (0, 0, 0)
    assert F.nearest_node((ox - 0.25, oy - 0.75, oz + 0.25)) == (1, 2, 1)                     # exact halves go away from zero
    assert F.nearest_node((ox + 99, oy + 99, oz - 99)) == (0, 0, 0)
    assert F.nearest_node((ox - 99, oy - 99, oz + 99)) == (3, 4, 3)
    assert F.nearest_node((ox - 99, oy + 99, oz)) == (3, 0, 0) and F.nearest_node((ox + 99, oy - 99, oz + 99)) == (0, 4, 3)
    assert F.linear_index((1, 2, 3)) == (3 * 5 + 2) * 4 + 1
    node = F.nodes.reshape(-1, 4)[F.linear_index((1, 2, 3))]
    assert node[0] == F.dist[3, 1, 2]
    v, der = F.value_and_derivative((ox - 0.5 + 0.1, oy - 1.0, oz + 1.5 + 0.2))
    assert der == [float(node[1]), float(node[2]), float(node[3])]
    assert v == float(node[0]) + ((der[0] * ((ox - 0.5 + 0.1) - (ox - 0.5)) + der[1] * ((oy - 1.0) - (oy - 1.0))) + der[2] * ((oz + 1.5 + 0.2) - (oz + 1.5)))
    assert R.num_layers(0.0, 0.05, 0.1) == 2 and R.num_layers(0.0, 0.0, 0.1) == 2 and R.num_layers(-1.0, 2.0, 0.2) == 15
    assert [R.layer_height(f32(0.3), f32(0.1), z) for z in range(4)] == [f32(0.3), f32(0.3) + f32(0.1), f32(0.3) + f32(2) * f32(0.1),
                                                                        f32(0.3) + f32(3) * f32(0.1)]
