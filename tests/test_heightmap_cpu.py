"""tests/heightmap_restate.py against closed forms (no GPU): the numpy restatement the device is compared with in
tests/test_gpu_heightmap.py is itself pinned here.  Parity with PCL, Eigen and grid_map is unpinned (none can be built here)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_restate as H   # noqa: E402

f32 = np.float32
NO_FILTER = dict(remove_outliers=0, level_and_ego_filter=0)


def test_tilted_plane_mean_per_cell_is_analytic():
    # z = a x + b y + c sampled on a lattice of 4 x 4 points per 0.5 m cell, all exactly representable: the mean of a cell is
    # the plane at the mean of its points, and every sum is exact in fp64
    a, b, c = 0.25, -0.5, 3.0
    xs = np.arange(0, 6 * 4 + 1) * 0.125                       # 0 .. 3.0
    ys = np.arange(0, 4 * 4 + 1) * 0.125                       # 0 .. 2.0
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), (a * X + b * Y + c).ravel()], 1).astype(f32)
    r = H.height_map(pts, resolution=0.5, **NO_FILTER)
    assert (r["rows"], r["cols"]) == (6, 4) and np.allclose(r["length"], [3.0, 2.0]) and np.allclose(r["position"], [1.5, 1.0])
    # the maximum corner row / column (x = 3.0, y = 2.0) has index 0; the minimum ones (x = 0, y = 0) index == size: dropped
    assert r["n_binned"] == (len(xs) - 1) * (len(ys) - 1) and r["n_valid_cells"] == 24
    for row in range(6):
        for col in range(4):
            # cell (row, col) holds x in (3 - 0.5 (row + 1), 3 - 0.5 row], the 4 lattice points ending at the upper edge
            mx = 3.0 - 0.5 * row - 0.125 * 1.5
            my = 2.0 - 0.5 * col - 0.125 * 1.5
            assert r["grid"][row, col] == f32(a * mx + b * my + c), (row, col)


def test_size_rounds_half_away_from_zero():
    for k in (3, 4):                                            # length / resolution = k + 0.5 exactly (binary fractions)
        pts = np.array([[0.0, 0.0, 0.0], [(k + 0.5) * 0.25, 1.0, 0.0]], f32)
        g = H.geometry(pts, 0.25)
        assert (g["rows"], g["cols"]) == (k + 1, 4) and g["length"][0] == (k + 1) * 0.25
    assert [H.c_round(x) for x in (0.5, 1.5, 2.5, 0.49999999999999994, 2.4999999999999996)] == [1, 2, 3, 0, 2]


def test_points_on_the_extreme_corners():
    pts = np.array([[-1.0, -2.0, 5.0], [1.0, 2.0, 7.0], [0.0, 0.0, 1.0]], f32)
    g = H.geometry(pts, 0.5)
    r, c, inside = H.bin_cells(pts, g)
    assert (g["rows"], g["cols"]) == (4, 8)
    assert inside.tolist() == [False, True, True]               # the minimum corner: index == size on both axes
    assert (r[1], c[1]) == (0, 0) and (r[2], c[2]) == (2, 4)
    out = H.height_map(pts, resolution=0.5, **NO_FILTER)
    assert out["n_binned"] == 2 and out["grid"][0, 0] == f32(7.0) and out["grid"][2, 4] == f32(1.0) and out["n_valid_cells"] == 2


def test_r2_is_not_the_inverse_of_r1():
    R1, R2 = H.rotations(0.3, -0.2)
    P = R2.astype(np.float64) @ R1.astype(np.float64)
    assert np.abs(P - np.eye(3)).max() > 1e-2                   # Rx(r) Ry(p) Rx(-r) Ry(-p) != I
    # ... and each is the textbook product
    def rx(a): return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    def ry(a): return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    r, p = float(f32(0.3)), float(f32(-0.2))
    assert np.abs(R1 - rx(-r) @ ry(-p)).max() < 3e-7 and np.abs(R2 - rx(r) @ ry(p)).max() < 3e-7
    R1z, R2z = H.rotations(0.0, 0.0)
    assert np.array_equal(R1z, np.eye(3, dtype=f32)) and np.array_equal(R2z, np.eye(3, dtype=f32))
    # roll = pitch = 0: the ego filter alone, thresholds exclusive
    pts = np.array([[2.0, 4.0, 0.5], [2.0, 4.0, 1.0], [2.5, 4.0, 1.5], [2.5, 4.0, 2.0], [20.0, 0.0, 9.0], [0.0, 30.0, 9.0], [19.0, 29.0, 2.5]], f32)
    kept, keep = H.level_ego(pts, 0.0, 0.0)
    assert keep.tolist() == [True, False, True, False, True, True, False] and np.array_equal(kept, pts[keep])


def test_components_against_scipy():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(5)
    for n, tol in ((1, 0.3), (40, 0.3), (200, 0.15), (200, 0.4)):
        p = rng.uniform(0, 1.5, (n, 3)).astype(f32)
        d = p[:, None, :] - p[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        adj = d2 <= f32(float(f32(tol)) * float(f32(tol)))
        n_comp, lab = connected_components(csr_matrix(adj), directed=False)
        mine = H.components(p, tol)
        assert len(np.unique(mine)) == n_comp
        for c in range(n_comp):                                 # same partition, and the label is the first member
            members = np.nonzero(lab == c)[0]
            assert (mine[members] == members[0]).all()
    # cluster heights: sizes outside [min, max] drop, min or max of the rest
    cell = np.array([[0, 0, 0.0], [0, 0, 0.1], [0, 0, 0.2], [0, 0, 2.0], [0, 0, 5.0], [0, 0, 5.1], [0, 0, 5.2], [0, 0, 5.3]], f32)
    cfg = dict(H.DEFAULTS, use_cluster=1, cluster_tolerance=0.3, cluster_min_points=3)
    assert H.cell_height(cell, cfg) == H.ordered_mean(cell[:3, 2])
    assert H.cell_height(cell, dict(cfg, use_max_height=1)) == H.ordered_mean(cell[4:, 2])
    assert H.cell_height(cell, dict(cfg, cluster_max_points=3, use_max_height=1)) == H.ordered_mean(cell[:3, 2])
    assert np.isnan(H.cell_height(cell, dict(cfg, cluster_min_points=5)))
    assert H.cell_height(cell, dict(cfg, cluster_tolerance=2.0)) == H.ordered_mean(cell[:4, 2])      # 0 .. 2.0 chain, 5.x apart


def test_fill_cascade_against_a_sort():
    rng = np.random.default_rng(9)
    layer = rng.uniform(-1, 1, (30, 24)).astype(f32)
    layer[rng.uniform(size=layer.shape) < 0.6] = np.nan
    layer[:12, :12] = np.nan                                    # a hole wider than the window
    layer[0, 0] = np.nan
    out, n = H.fill(layer)
    n_ref = 0
    for row, col in zip(*np.nonzero(np.isnan(layer))):
        cand = []                                               # (distance, visiting order): the cascade keeps the earliest of equals
        for i in range(max(row - 5, 0), min(row + 5, 30)):
            for j in range(max(col - 5, 0), min(col + 5, 24)):
                if not np.isnan(layer[i, j]):
                    cand.append((math.sqrt((i - row) ** 2 + (j - col) ** 2), len(cand), float(layer[i, j])))
        cand.sort()
        if len(cand) < 4:
            assert np.isnan(out[row, col])
            continue
        n_ref += 1
        assert out[row, col] == f32((((cand[0][2] + cand[1][2]) + cand[2][2]) + cand[3][2]) / 4.0)
    assert n == n_ref > 0 and np.isnan(out).any()
    valid = ~np.isnan(layer)
    assert np.array_equal(out[valid], layer[valid])
    # the window is asymmetric: a valid cell 5 rows below is out of reach, 5 rows above is in
    one = np.full((12, 1), np.nan, f32)
    one[1:5, 0] = 1.0
    assert np.isnan(H.fill(one)[0][9, 0]) and H.fill(one)[0][6, 0] == f32(1.0)      # rows [1, 11) from 6; [4, 12) from 9


def test_ordered_sum_is_the_input_order():
    z = np.array([1e8, 1.0, -1e8, 1.0], f32)
    assert H.ordered_mean(z) == f32(((1e8 + 1.0 - 1e8) + 1.0) / 4.0)
    rng = np.random.default_rng(2)
    z = (10.0 ** rng.uniform(-6, math.log10(50.0), 2000)).astype(f32)
    acc = 0.0
    for v in z:
        acc += float(v)
    assert H.ordered_mean(z) == f32(acc / 2000.0)
