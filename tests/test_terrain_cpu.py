"""Pins tests/terrain_restate.py, the numpy restatement the device's terrain layers are held against:
closed forms where there are any, LAPACK for the closed-form eigen solver.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_restate as T                                    # noqa: E402

f32 = np.float32

# The closed-form solver's error against LAPACK in units of 2^-53 |sumSquared / n|_F / (l1 - l0), the largest over the
# well-conditioned cells of scene A (seed 5) at positions (0, 0) and (60, -35), radii 0.3 and 0.6: 1.697, measured
# 2026-10-18 (the worst cell is (30, 7) at radius 0.3, next to the spike).  tests/test_gpu_terrain.py holds the device to 8 K.
K_EIGEN = 1.7

# circle members under the fp64 rule on the 9 x 7 grid at resolution 0.25, position (3.7, -12.3): radius in cells ->
# (cell (4, 3), corner (0, 0), the sum over all cells).  At this position no rounding drops a cell at the exact distance.
CIRCLE_COUNTS = {0.5: (1, 1, 63), 1.0: (5, 3, 283), math.sqrt(2.0): (9, 4, 475), 2.0: (13, 6, 663), 2.5: (21, 8, 991)}


def test_circle_membership():
    G = T.Geom(9, 7, 0.25, (3.7, -12.3))
    for cells, want in CIRCLE_COUNTS.items():
        radius = cells * 0.25
        per = [[len(T.circle(G, i, j, radius)) for j in range(7)] for i in range(9)]
        print(f"  radius {cells} cells: centre {per[4][3]}, corner {per[0][0]}, total {sum(map(sum, per))}")
        assert (per[4][3], per[0][0], sum(map(sum, per))) == want, cells
    # the visiting order: rows outermost, the column index fastest; the centre cell is a member of its own circle
    members = T.circle(G, 4, 3, 0.25)
    assert members == [(3, 3), (4, 2), (4, 3), (4, 4), (5, 3)]
    # cell centres: x falls with the row index, one resolution per cell, around the position
    assert T.centre(G, 0, 0) - T.centre(G, 0, 1) == pytest.approx(0.25, abs=1e-12)
    assert 0.5 * (T.centre(G, 0, 0) + T.centre(G, 0, 8)) == pytest.approx(3.7, abs=1e-12)
    assert 0.5 * (T.centre(G, 1, 0) + T.centre(G, 1, 6)) == pytest.approx(-12.3, abs=1e-12)


def plane(G, a, b):
    x = np.array([T.centre(G, 0, i) for i in range(G.rows)])
    y = np.array([T.centre(G, 1, j) for j in range(G.cols)])
    return x, y, (a * x[:, None] + b * y[None, :])


def test_plane_normals():
    # a and b are dyadic and the centres multiples of 1/8: the float grid holds the plane exactly
    G = T.Geom(12, 10, 0.25, (1.0, -2.0))
    a, b = 0.25, -0.5
    _, _, z = plane(G, a, b)
    grid = z.astype(f32)
    assert np.array_equal(grid.astype(np.float64), z)
    want = np.array([-a, -b, 1.0]) / math.sqrt((a * a + b * b) + 1.0)
    (nx, ny, nz), counts = T.normals_raster(grid, G, 2)
    inner = (slice(1, -1), slice(1, -1))
    assert counts["n_normal_cells"] == 10 * 8 and np.isnan(nx[0]).all() and np.isnan(nx[:, -1]).all()
    for got, w in zip((nx, ny, nz), want):
        assert (got[inner] == f32(w)).all()
    # area: the same direction within the solver's bar on a plane (conditioning: l0 = 0)
    (ax, ay, az), counts = T.normals_area(grid, G, 0.6, 2)
    assert counts == dict(n_normal_cells=120, n_few_points=0, n_degenerate=0)
    cond = T.conditioning(grid, G, 0.6)
    worst = 0.0
    for (r, c), (w, v, fro, ev, v0) in cond.items():
        bar = K_EIGEN * 2.0 ** -53 * fro / (w[1] - w[0])
        ang = T.line_angle(v0, want)
        worst = max(worst, ang / bar)
        assert ang <= 8 * bar, (r, c, ang, bar)               # (the plane's own normal, not LAPACK's: the covariance is rounded too)
        assert abs(float(az[r, c]) - want[2]) < 1e-6
    print(f"  area on a plane: worst angle {worst:.2f} bars")
    # the positive axis: with x, a normal whose x component would be negative is flipped
    (fx, fy, fz), _ = T.normals_raster(grid, G, 0)
    assert (fx[inner] == f32(-want[0])).all() and (fz[inner] == f32(-want[2])).all()


def test_smooth_of_a_constant():
    G = T.Geom(7, 9, 0.2, (5.0, 5.0))
    grid = np.full((7, 9), 1.2345, f32)
    grid[3, 4] = np.nan
    sm = T.smooth(grid, G, 0.45)
    assert (sm == f32(1.2345)).all()                           # every cell, the hole too
    assert (T.roughness_of(grid, sm)[~np.isnan(grid)] == 0).all() and np.isnan(T.roughness_of(grid, sm)[3, 4])
    lone = np.full((7, 9), np.nan, f32)
    lone[0, 0] = 2.0
    sm = T.smooth(lone, G, 0.45)
    assert sm[0, 0] == 2.0 and sm[1, 1] == 2.0 and np.isnan(sm[6, 8])   # no finite cell in the circle: NaN


def test_edge_window():
    assert T.edge_window_size(0.5, 0.2) == 3                   # 2.5 -> round 3
    assert T.edge_window_size(0.5, 0.25) == 3                  # 2 -> even -> 3
    assert T.edge_window_size(1.0, 0.25) == 5                  # 4 -> 5
    assert T.edge_window_size(0.05, 0.2) == 1                  # the yaml's length at the loader's resolution: the cell alone
    assert T.edge_window_size(0.0, 0.25, explicit=7) == 7
    with pytest.raises(ValueError):
        T.edge_window_size(0.0, 0.25, explicit=4)
    # a constant (dyadic: its float sums are exact) slope has no edges; a window without slope gives NaN; the crop at the border
    s = np.full((5, 6), 0.25, f32)
    assert (T.edges_of(s, 3) == 0).all()
    s[:, 3:] = np.nan
    e = T.edges_of(s, 3)
    assert (e[:, :4] == 0).all() and np.isnan(e[:, 4:]).all()
    step = np.zeros((1, 4), f32)
    step[0, 2:] = 1.0
    e = T.edges_of(step, 3)                                    # windows (0 0), (0 0 1), (0 1 1), (1 1): the crop at both ends
    assert e[0, 0] == 0 and e[0, 3] == 0
    assert e[0, 1] == pytest.approx(math.sqrt(2.0) / 3.0, rel=1e-6) and e[0, 2] == pytest.approx(math.sqrt(2.0) / 3.0, rel=1e-6)


def test_threshold_quirk():
    slope = np.array([0.0, 0.3, np.nan, 0.3, 2.0, 0.0], f32)
    rough = np.array([0.0, 0.05, 0.05, np.nan, 1.0, -0.5], f32)
    t = T.traversability_of(slope, rough)
    assert t[0] == 1.0 and t[2] == 0.0 and t[3] == 0.0 and t[4] == 0.0 and t[5] == 1.0    # NaN -> 0, below 0 -> 0, above 1 -> 1
    assert t[1] == (f32(0.5) * (f32(1.0) - f32(0.3) / f32(0.6))) + (f32(0.5) * (f32(1.0) - f32(0.05) / f32(0.1)))
    assert not np.isnan(t).any()


def test_eigen_solver_against_lapack():
    """K: the closed-form solver's angle to LAPACK's eigenvector over the well-conditioned cells of scene A, in units of
    2^-53 |sumSquared / n|_F / (l1 - l0).  Also the share of cells left out as ill-conditioned (the GPU test caps it at 5 %)."""
    k_max = 0.0
    for pos in ((0.0, 0.0), (60.0, -35.0)):
        grid = T.scene_a(pos)
        G = T.Geom(grid.shape[0], grid.shape[1], 0.25, pos)
        n_finite = int(np.isfinite(grid).sum())
        for radius in (0.3, 0.6):
            cond = T.conditioning(grid, G, radius)
            ill, k = 0, 0.0
            for (r, c), (w, v, fro, ev, v0) in cond.items():
                assert np.allclose(ev, w, rtol=0, atol=1e-9 * max(1.0, fro))
                if not T.well_conditioned(w):
                    ill += 1
                    continue
                k = max(k, T.line_angle(v0, v) / (2.0 ** -53 * fro / (w[1] - w[0])))
            print(f"  position {pos}, radius {radius}: {len(cond)} cells, {ill} ill-conditioned ({100.0 * ill / n_finite:.2f} %), K {k:.4f}")
            assert ill <= 0.05 * n_finite
            k_max = max(k_max, k)
    print(f"  K = {k_max:.4f}")
    assert k_max <= K_EIGEN
