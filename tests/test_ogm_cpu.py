"""Pins tests/ogm_restate.py, the numpy restatement the GPU tests of the occupancy grid hold the device to: the fp32 counts
against a kd-tree in fp64 on inputs where no pair is near the radius, the tie rule on a lattice, and both rasters against
small grids worked out by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ogm_restate as R                                        # noqa: E402

PARAMS = ((1.0, 3), (1.5, 10), (0.5, 1))                       # (radius, min_neighbors)
KEPT = {257: (112, 59, 79), 513: (420, 424, 242)}


def uniform_clouds():
    """the two clouds of the filter tests, 257 and 513 points: one past a workgroup of 256, one past two"""
    return _clouds()[0]


def raster_cloud():
    """513 points uniform in (-6, 6)^3, the next draw of the same generator"""
    return _clouds()[1]


def _clouds():
    rng = np.random.default_rng(31)
    flt = {n: (rng.uniform(-6, 6, (n, 3)) * [1, 1, 0.2]).astype(np.float32) for n in (257, 513)}
    return flt, rng.uniform(-6, 6, (513, 3)).astype(np.float32)


def lattice():
    """6 x 6 x 2 points of pitch 0.5: every neighbour distance is the radius 0.5 exactly, or more"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * 0.5).astype(np.float32)


def test_counts_equal_a_kdtree_where_the_bracket_is_empty():
    from scipy.spatial import cKDTree
    gaps = []
    for n, pts in uniform_clouds().items():
        p64 = pts.astype(np.float64)
        d2 = ((p64[:, None, :] - p64[None, :, :]) ** 2).sum(axis=2)
        tree = cKDTree(p64)
        for (radius, min_nb), kept in zip(PARAMS, KEPT[n]):
            r2 = float(radius) ** 2
            gap = np.abs(d2 - r2).min() / r2
            gaps.append(gap)
            assert gap > 1e-5, (n, radius, gap)                # no pair within 1e-5 r^2 of the radius: about 300 fp32 roundings of d2
            ref = np.array([len(v) for v in tree.query_ball_point(p64, radius)], np.int32)
            idx, k = R.radius_keep(pts, radius, min_nb)
            assert np.array_equal(k, ref), (n, radius)
            assert len(idx) == kept and 0 < kept < n, (n, radius, len(idx))
            assert np.array_equal(idx, np.nonzero(ref > min_nb)[0])
    assert 7.2e-5 < min(gaps) < 7.4e-5, min(gaps)              # the inputs are the ones the figure was taken on


def test_tie_rule_is_strict():
    pts = lattice()
    k = R.radius_counts(pts, 0.5)
    assert (k == 1).all()                                       # a neighbour AT the radius is not counted: only the point itself
    assert len(R.radius_keep(pts, 0.5, 0)[0]) == len(pts)       # k > 0
    assert len(R.radius_keep(pts, 0.5, 1)[0]) == 0              # k > 1: nothing
    assert (R.radius_counts(pts, np.nextafter(np.float32(0.5), np.float32(1))) > 1).all()


def test_duplicates_count_and_bad_points_take_no_part():
    pts = np.array([[0, 0, 0], [0, 0, 0], [0.3, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [2e15, 0, 0], [5, 5, 5]], np.float32)
    assert R.radius_counts(pts, 0.5).tolist() == [3, 3, 3, -1, -1, -1, 1]


def test_slice_limits_are_inclusive_floats():
    z = np.array([0.2, np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(0)), 2.0, np.nextafter(np.float32(2), np.float32(3)), 1.0,
                  np.nan], np.float32)
    pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
    pts[5, 0] = np.inf                                          # a finite z does not save a point with a bad x
    assert R.slice_z(pts, 0.2, 2.0).tolist() == [0, 1, 3]
    assert R.slice_z(pts, 0.2, 2.0, negative=1).tolist() == [2, 4]     # the outside, still without the non-finite ones


def test_raster_by_hand():
    # box over the first three points: x 0 .. 1, y 0 .. 0.75 at 0.25 m -> 4 x 3 cells; the last point (2, 2) is outside
    pts = np.array([[0, 0, 0], [1.0, 0.75, 0], [0.3, 0.3, 0], [0.6, 0.55, 0], [2, 2, 0]], np.float32)
    grid, w, h, origin, n_binned = R.raster(pts, 0.25)
    assert (w, h, origin) == (4, 3, (0.0, 0.0))
    exp = np.zeros((3, 4), np.int8)
    exp[0, 0] = 100                                             # (0, 0)
    exp[1, 1] = 100                                             # (0.3, 0.3)
    # (1.0, 0.75): i = 4 = width, skipped; (0.6, 0.55): j = 2 = height - 1, the last row is never filled; (2, 2): outside
    assert np.array_equal(grid, exp) and n_binned == 2
    assert not grid[-1].any()
    # the last point as the extreme: the box ignores it as written and includes it with whole_box
    grid_w, w2, h2, origin2, nb2 = R.raster(pts, 0.25, whole_box=1)
    assert (w2, h2, origin2) == (8, 8, (0.0, 0.0))
    exp = np.zeros((8, 8), np.int8)
    for x, y in ((0, 0), (1.0, 0.75), (0.3, 0.3), (0.6, 0.55)):
        exp[int(y / 0.25), int(x / 0.25)] = 100
    assert np.array_equal(grid_w, exp) and nb2 == 4             # (2, 2): i = 8 = width, skipped
    # a last point less than one cell below the minimum lands in column / row 0: (int) truncates toward zero
    pts = np.array([[0, 0, 0], [1, 1, 0], [-0.2, -0.1, 0]], np.float32)
    grid, w, h, origin, n_binned = R.raster(pts, 0.25)
    assert (w, h, n_binned) == (4, 4, 2) and grid[0, 0] == 100 and int((grid == 100).sum()) == 1
    pts[2] = [-0.3, -0.1, 0]                                    # more than a cell below: i = -1
    assert R.raster(pts, 0.25)[4] == 1
    # degenerate clouds: one point is its own box; no extent along x
    assert R.raster(np.array([[1, 2, 3]], np.float32), 0.25)[1:4] == (0, 0, (1.0, 2.0))
    g, w, h, _, nb = R.raster(np.array([[1, 0, 0], [1, 2, 0], [1, 1, 0]], np.float32), 0.25)
    assert (w, h, nb) == (0, 8, 0) and g.shape == (8, 0)
    assert R.raster(np.zeros((0, 3), np.float32), 0.25)[1:3] == (0, 0)


def test_raster_quirks_on_a_random_cloud():
    pts = raster_cloud()
    grid, w, h, _, n_binned = R.raster(pts, 0.25)
    assert (w, h, n_binned) == (47, 47, 483) and not grid[-1].any()
    grid_w, w2, h2, _, nb2 = R.raster(pts, 0.25, whole_box=1)
    assert (w2, h2, nb2) == (47, 47, 496)
    # the 13 further points all fall into the last row, into 9 of its cells; the rows below are the as-written grid's
    assert int((grid_w[-1] == 100).sum()) == 9 and np.array_equal(grid_w[:-1], grid[:-1])


def test_chain_counts_are_consistent():
    pts = uniform_clouds()[513] + np.float32([0, 0, 1.0])
    grid, info = R.occupancy_grid(pts, z_min=0.2, z_max=1.5, radius=1.0, min_neighbors=3, resolution=0.25)
    assert info["n_in"] == 513 and 0 < info["n_inliers"] < info["n_slice"] < 513
    assert 0 < info["n_occupied"] <= info["n_binned"] <= info["n_inliers"]
    assert grid.shape == (info["height"], info["width"]) and set(np.unique(grid)) == {0, 100}
