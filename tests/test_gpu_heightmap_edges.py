"""The planning height map on the device at the edges of its clustering, its cell keys and its fill: every designed input of
tests/heightmap_cases.py through lio_height_map against the restatement (tests/heightmap_restate.py), by check() of
tests/test_gpu_heightmap.py: geometry, all six counts, the NaN mask and every other word bit for bit.  Tolerance 0: the device
does fixed-order fp32 and fp64 arithmetic and the restatement states the same order.  tests/test_heightmap_cases_cpu.py
proves without a GPU that every case holds what it is named for and that the restatement on it differs from the defect it
targets.  Parity with PCL and grid_map themselves stays unpinned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_cases as K                                    # noqa: E402
from test_gpu_heightmap import assert_same_grid, bits, check, small_store   # noqa: E402, F401  (small_store: a fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32


def run(pkg, name):
    pts, cfg = K.case(name)
    return check(pkg, pts, name, **cfg)


# ---- A. clustering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.names("chain_") + K.names("two_chains_"))
def test_chains(pkg, name):
    # a component joined link by link only, in four index orders; cluster_min_points = its size, so a fragment gives NaN
    grid, info, ref = run(pkg, name)
    r, c = K.info(name)["cell"]
    assert info.n_valid_cells == 1 and not np.isnan(grid[r, c])


@pytest.mark.parametrize("name", ["tol_eq_small", "tol_eq_big", "tol_zero"])
def test_tolerance_boundary(pkg, name):
    grid, info, ref = run(pkg, name)
    for rc, want in K.info(name)["want"].items():               # d2 == tol2 joins; one float further does not
        assert np.isnan(grid[rc]) if want is None else grid[rc] == want, rc


@pytest.mark.parametrize("name", ["tile_cells_max0", "tile_cells_max1", "two_long_cells"])
def test_tile_boundary(pkg, name):
    grid, info, ref = run(pkg, name)
    assert info.n_valid_cells == 3 and info.n_binned == info.n_filtered - 1


@pytest.mark.parametrize("name", ["ties_max0", "ties_max1"])
def test_ties(pkg, name):
    grid, info, ref = run(pkg, name)
    for rc, d in K.info(name)["ties"].items():                  # +0.0 against -0.0: the component with the smaller first member
        assert grid[rc] == 0 and bool(np.signbit(grid[rc])) == d["negative_wins"], (rc, d)


@pytest.mark.parametrize("name", ["best_lane_max0", "best_lane_max1"])
def test_best_component_in_a_late_lane(pkg, name):
    grid, info, ref = run(pkg, name)
    for rc, d in K.info(name)["best"].items():
        assert grid[rc] == d["height"], (rc, d)


@pytest.mark.parametrize("name", ["size_limits_max0", "size_limits_max1", "cluster_min_zero", "cell_min_points", "cell_max_points"])
def test_size_limits(pkg, name):
    grid, info, ref = run(pkg, name)
    inf = K.info(name)
    if name.startswith("size_limits"):
        assert np.isnan(grid[0, 1]) and info.n_valid_cells == 2          # every component rejected: NaN, not counted
    if "valid" in inf:
        assert sorted(inf["valid"]) == sorted((int(r), int(c)) for r, c in zip(*np.nonzero(~np.isnan(grid))))


def test_more_cells_than_workgroups(pkg):
    # 4160 cells on 4096 workgroups: a workgroup goes from a global-memory cell to an LDS cell, the reverse, and past a refused cell
    grid, info, ref = run(pkg, "many_cells")
    inf = K.info("many_cells")
    assert info.rows * info.cols > K.HM_GROUPS
    for k in inf["keys"]:
        assert np.isnan(grid[k % 65, k // 65]) == (k == inf["refused"]), k


def test_clusters_from_the_store(pkg, small_store):
    st = small_store
    pose = np.array([0.02, -0.01, 0.4, 2.0, 0.8, 0.1], f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    cloud, lm_ref, rc = st.local_map(pose, lm)
    assert rc == 0 and lm_ref.n_out > 500
    cfg = pkg.height_map_default_config(roll=0.02, pitch=-0.01, resolution=0.5, use_cluster=1, cluster_tolerance=0.3, cluster_min_points=2,
                                        use_max_height=1)
    grid, info, lm_info = st.height_map(pose, lm, cfg)
    direct, info_d = pkg.height_map(cloud[:, :3], cfg)
    print(f"  store, clustered: {info.rows} x {info.cols}, in {info.n_in}, binned {info.n_binned}, valid {info.n_valid_cells}; direct "
          f"{info_d.rows} x {info_d.cols}, {info_d.n_in}, {info_d.n_binned}, {info_d.n_valid_cells}")
    for name, _ in pkg.HeightMapInfo._fields_:
        a, b = getattr(info, name), getattr(info_d, name)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    assert info.n_in == lm_ref.n_out and 0 < info.n_valid_cells < info.rows * info.cols
    assert_same_grid(grid, direct, "store, clustered")
    plain, _, _ = st.height_map(pose, lm, pkg.height_map_default_config(roll=0.02, pitch=-0.01, resolution=0.5))
    assert not np.array_equal(bits(plain), bits(grid))          # clustering changed the layer


# ---- B. cell keys and the sort --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.names("sort_"))
def test_sort_width(pkg, name):
    # n_cells at and next to a power of two, with points on the key behind the last cell
    grid, info, ref = run(pkg, name)
    rows, cols = K.info(name)["shape"]
    assert (info.rows, info.cols) == (rows, cols) and info.n_binned == info.n_filtered - K.info(name)["n_dropped"] < info.n_filtered
    assert not np.isnan(grid[0, 0]) and not np.isnan(grid[rows - 1, cols - 1])


@pytest.mark.parametrize("name", K.names("far_") + K.names("thin_"))
def test_far_and_thin_grids(pkg, name):
    grid, info, ref = run(pkg, name)
    assert info.n_binned > 0
    if name.startswith("thin"):
        assert (info.rows, info.cols) == K.info(name)["shape"]


# ---- C. fill ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.names("fill_"))
def test_fill(pkg, name):
    grid, info, ref = run(pkg, name)
    inf = K.info(name)
    valid = ~np.isnan(inf["values"])
    assert np.array_equal(bits(grid[valid]), bits(inf["values"][valid])) and info.n_valid_cells == int(valid.sum())
    if "filled" in inf:
        assert not np.isnan(grid[inf["filled"]]) and np.isnan(grid[inf["stays"]])
    if "want" in inf:
        assert grid[inf["hole"]] == inf["want"]
    if inf.get("k") == 3:
        assert info.n_filled_cells == 0
