"""grid_map's region iterators on the resident planning layers (lio_grid_region_reduce, lio_grid_region_cells) through the C
ABI: every output word against the restatement (tests/grid_region_restate.py), which tests/test_grid_region_cpu.py holds
against the reference's own sequences and against the header the kernels run.  All grids are 70 x 50 or smaller."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_region_restate as R                                # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
GRIDS = [(8, 5, 1.0, (0.0, 0.0)), (3, 3, 1.0, (0.0, 0.0)), (1, 1, 0.2, (0.0, 0.0)), (70, 50, 0.2, (1e3, -3e3))]


def upload(pkg, g, arrays):
    grid = pkg.Grid()
    grid.set_layers(np.stack(arrays), g.res, g.length, g.pos)
    return grid


def words(stats):
    """the library's records with min and max as their words: the restatement's dtype"""
    return stats.view(R.STAT_DTYPE)


def check_reduce(grid, g, arrays, regions, ids=None, threshold=0.5, what=None):
    ids = list(range(len(arrays))) if ids is None else ids
    stats, n_cells, status, info = grid.region_reduce(regions, ids, threshold=threshold)
    want, w_n, w_status = R.regions_reduce(g, [arrays[k] for k in ids], regions, threshold)
    assert np.array_equal(status, w_status), (what, "status", np.nonzero(status != w_status)[0][:5])
    assert np.array_equal(n_cells, w_n), (what, "n_cells", np.nonzero(n_cells != w_n)[0][:5])
    got = words(stats)
    assert got.shape == want.shape
    for name in ("n_finite", "n_below", "min", "max"):
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5])
    assert np.array_equal(got["sum"].view(np.uint64), want["sum"].view(np.uint64)), (what, "sum", np.argwhere(got["sum"] != want["sum"])[:5])
    assert (info.n_ok, info.n_empty, info.n_invalid) == tuple(int((w_status == s).sum()) for s in (R.OK, R.EMPTY, R.INVALID)), what
    assert info.n_cells == int(w_n.sum()), what
    return stats, n_cells, status, info


def check_cells(grid, g, regions, what=None):
    offsets, cells, status, info = grid.region_cells(regions)
    w_off, w_cells, w_status = R.regions_cells(g, regions)
    assert np.array_equal(status, w_status), (what, "status")
    assert np.array_equal(offsets, w_off), (what, "offsets")
    assert np.array_equal(cells, w_cells), (what, "cells")
    assert info.n_cells == len(w_cells) and info.n_ok + info.n_empty + info.n_invalid == len(regions)
    return offsets, cells


def layers_for(rows, cols, n, holes=True):
    return [R.make_layer(rows, cols, holes and k % 2 == 0, seed=17 * k + rows) for k in range(n)]


def test_reference_sequences(pkg):
    """the reference's own tests on its 8 x 5 map (the literals of tests/test_grid_region_cpu.py), through lio_grid_region_cells"""
    g = R.Geometry(8, 5, 1.0)
    grid = upload(pkg, g, [np.zeros((8, 5), f32)])
    regions = [("polygon", ((-100.0, 100.0), (100.0, 100.0), (100.0, -100.0), (-100.0, -100.0))),          # PolygonIteratorTest.cpp:25-63
               ("polygon", ((99.0, 101.0), (101.0, 101.0), (101.0, 99.0), (99.0, 99.0))),                  # :65-79
               ("polygon", ((-1.0, 1.5), (1.0, 1.5), (1.0, -1.5), (-1.0, -1.5))),                          # :81-125
               ("polygon", ((-40.1, 20.6), (40.1, 20.4), (-40.1, -20.6))),                                 # :127-149
               ("ellipse", 0.0, 0.0, 8.0, 1.0, 0.0),                                                       # EllipseIteratorTest.cpp:23-55
               ("line", 2.0, 2.0, 0.0, 0.0), ("line", 0.0, 0.0, 9.0, 6.0), ("line", -7.0, -9.0, 8.0, 8.0),  # LineIteratorTest.cpp:17-98
               ("line", -8.0, 8.0, 8.0, 8.0)]                                                              # :100-106
    offsets, cells, status, _ = grid.region_cells(regions)
    rc = [[(int(k) % 8, int(k) // 8) for k in cells[offsets[q]:offsets[q + 1]]] for q in range(len(regions))]
    assert rc[0] == [(r, c) for r in range(8) for c in range(5)]
    assert rc[1] == [] and status[1] == R.EMPTY
    assert rc[2] == [(3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3)]
    assert rc[3][:2] == [(0, 0), (1, 0)]
    assert rc[4] == [(r, 2) for r in range(8)]
    assert rc[5] == [(2, 0), (3, 1), (4, 2)]
    assert rc[6][:3] == [(4, 2), (3, 1), (2, 1)] and len(rc[6]) == 5
    assert rc[7][:3] == [(5, 4), (4, 3), (3, 2)] and len(rc[7]) == 5
    assert rc[8] == [] and status[8] == R.EMPTY
    assert list(status[[0, 2, 3, 4, 5, 6, 7]]) == [R.OK] * 7
    check_cells(grid, g, regions, "reference")
    grid.close()


@pytest.mark.parametrize("n_layers", [1, 3, 10])
@pytest.mark.parametrize("grid_case", GRIDS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_lattice(pkg, grid_case, n_layers):
    """the whole CPU lattice (every INVALID cause, the lines' special cases, the 64 / 65 / 256-cell windows) through both
    entry points; 10 layers take three sweeps of four"""
    rows, cols, res, pos = grid_case
    g = R.Geometry(rows, cols, res, pos)
    arrays = layers_for(rows, cols, n_layers)
    grid = upload(pkg, g, arrays)
    regions = R.lattice(g) + R.exact_windows(g)
    before = [grid.layer(k).tobytes() for k in range(n_layers)]
    _, n_cells, status, _ = check_reduce(grid, g, arrays, regions, what=(rows, cols, n_layers))
    assert set(status) == {R.OK, R.EMPTY, R.INVALID}
    if n_layers == 1:
        check_cells(grid, g, regions, (rows, cols))
    if n_layers == 3:                                          # the caller's order of the layers, and a subset
        check_reduce(grid, g, arrays, regions[::3], ids=[2, 0], threshold=0.25, what="ids")
    assert [grid.layer(k).tobytes() for k in range(n_layers)] == before        # the layers are only read
    grid.close()


def test_exact_window_257(pkg):
    """257 cells: five sweeps of a wave, the last with one cell; along a row (strided) and along a column (contiguous)"""
    for rows, cols in ((1, 300), (300, 1)):
        g = R.Geometry(rows, cols, 0.5, (-2.0, 7.0))
        arrays = layers_for(rows, cols, 2)
        grid = upload(pkg, g, arrays)
        regions = R.exact_windows(g)
        _, n_cells, _, _ = check_reduce(grid, g, arrays, regions, threshold=0.25, what=(rows, cols))
        assert 257 in list(n_cells)
        check_cells(grid, g, regions, (rows, cols))
        grid.close()


def test_mixed_batch(pkg):
    """2000 random regions of all four kinds on the 70 x 50 grid with 20 % holes, word for word, through both entry points"""
    g = R.Geometry(70, 50, 0.2, (12.5, -40.0))
    arrays = [R.make_layer(70, 50, True, seed=5), R.make_layer(70, 50, False, seed=6)]
    grid = upload(pkg, g, arrays)
    regions = R.random_regions(g, 2000, 3)
    assert {r[0] for r in regions} == {"line", "circle", "ellipse", "polygon"}
    _, n_cells, status, info = check_reduce(grid, g, arrays, regions, what="mixed")
    assert info.n_ok > 1500 and info.n_empty > 0
    check_cells(grid, g, regions, "mixed")
    grid.close()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_region_counts_that_do_not_fill_a_workgroup(pkg, n):
    g = R.Geometry(70, 50, 0.2)
    arrays = layers_for(70, 50, 3)
    grid = upload(pkg, g, arrays)
    regions = R.random_regions(g, n, 100 + n)
    check_reduce(grid, g, arrays, regions, what=n)
    check_cells(grid, g, regions, n)
    # no regions at all: LIO_OK, nothing written
    stats, n_cells, status, info = grid.region_reduce([], [0])
    assert stats.shape == (1, 0) and info.n_ok == info.n_cells == 0
    offsets, cells, _, _ = grid.region_cells([])
    assert list(offsets) == [0] and len(cells) == 0
    grid.close()


def test_whole_map_and_capacity(pkg):
    """one region covering the whole map; cap_cells one short is LIO_ERR_CAPACITY with the need in offsets[n] and the cells
    untouched, the exact capacity succeeds"""
    g = R.Geometry(70, 50, 0.2, (3.0, 4.0))
    arrays = layers_for(70, 50, 2)
    grid = upload(pkg, g, arrays)
    whole = [("circle", 3.0, 4.0, 100.0), ("polygon", ((20.0, 20.0), (-20.0, 20.0), (-20.0, -20.0), (20.0, -20.0))), ("circle", 3.0, 4.0, 1.0)]
    _, n_cells, _, _ = check_reduce(grid, g, arrays, whole, what="whole")
    assert list(n_cells[:2]) == [3500, 3500]
    w_off, w_cells, _ = R.regions_cells(g, whole)
    lib = pkg.load_library()
    rec, verts = pkg.pack_regions(whole)
    need = int(w_off[-1])
    offsets = np.full(4, -7, np.int64)
    cells = np.full(need, -7, np.int32)
    info = pkg.GridRegionInfo()
    rc = lib.lio_grid_region_cells(grid.h, rec.ctypes.data, 3, verts.ctypes.data, len(verts), offsets.ctypes.data, cells.ctypes.data, need - 1, None, C.byref(info))
    assert rc == -3 and "cap_cells" in lib.lio_last_error().decode()
    assert np.array_equal(offsets, w_off) and (cells == -7).all() and info.n_cells == need
    rc = lib.lio_grid_region_cells(grid.h, rec.ctypes.data, 3, verts.ctypes.data, len(verts), offsets.ctypes.data, cells.ctypes.data, need, None, None)
    assert rc == 0 and np.array_equal(cells, w_cells) and np.array_equal(offsets, w_off)
    grid.close()


def test_second_call_with_fewer_regions_and_memory(pkg):
    """the object's workspace is reused: a smaller call after a larger one returns its own results, and lio_grid_memory grows
    with the first calls and is then stable"""
    g = R.Geometry(70, 50, 0.2)
    arrays = layers_for(70, 50, 2)
    grid = upload(pkg, g, arrays)
    m0 = grid.memory()
    many, few = R.random_regions(g, 300, 21), R.random_regions(g, 7, 22)
    check_reduce(grid, g, arrays, many, what="many")
    check_cells(grid, g, many, "many")
    m1 = grid.memory()
    check_reduce(grid, g, arrays, few, what="few")
    check_cells(grid, g, few, "few")
    check_reduce(grid, g, arrays, many, what="many again")
    check_cells(grid, g, many, "many again")
    assert m0 < m1 == grid.memory()
    grid.close()


def test_refusals_that_need_an_object(pkg):
    grid = pkg.Grid()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # no layers yet
        grid.region_reduce([("circle", 0.0, 0.0, 1.0)])
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        grid.region_cells([("circle", 0.0, 0.0, 1.0)])
    g = R.Geometry(8, 5, 1.0)
    grid.set_layers(np.zeros((2, 8, 5), f32), g.res, g.length, g.pos)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # an absent layer
        grid.region_reduce([("circle", 0.0, 0.0, 1.0)], [0, 2])
    stats, _, _, _ = grid.region_reduce([("circle", 0.0, 0.0, 1.0)], [1, 0])
    assert stats.shape == (2, 1)
    grid.close()


@pytest.fixture(scope="module")
def dense_store(pkg):
    """the scene of tests/test_gpu_grid_sample.py: keyframes on a jittered 0.1 m lattice over 15 m x 15 m around one hole"""
    rng = np.random.default_rng(41)
    st = pkg.KeyframeStore()
    poses = []
    for k in range(3):
        x, y = np.meshgrid(np.arange(-7.5, 7.5, 0.1), np.arange(-7.5, 7.5, 0.1), indexing="ij")
        xy = np.c_[x.ravel(), y.ravel()] + rng.uniform(-0.04, 0.04, (x.size, 2))
        xy = xy[~((xy[:, 0] > 2.0) & (xy[:, 0] < 3.2) & (xy[:, 1] > 1.0) & (xy[:, 1] < 2.0))]
        z = 0.04 * xy[:, 0] + 0.1 * np.sin(xy[:, 1]) + rng.normal(0, 0.01, len(xy))
        st.add(np.c_[xy, z, rng.uniform(0, 255, len(xy))].astype(f32))
        poses.append([0.0, 0.0, 0.0, 0.05 * k, 0.05 * k, 0.0])
    st.set_poses(0, np.array(poses, f32), times=np.arange(3) * 1.0)
    yield st
    st.close()


def test_store_path(pkg, dense_store):
    """layers left by lio_kf_store_planning_grid: vehicle footprints along a straight path on traversability and slope, against
    the restatement on the layers fetched back"""
    st = dense_store
    pose = np.zeros(6, f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(resolution=0.2, fill_holes=0)
    fill = pkg.median_fill_default_config(fill_hole_radius=2.0, num_erode_dilation_iterations=8)
    terrain = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)
    grid = pkg.Grid()
    st.planning_grid(grid, pose, lm, hm, fill, terrain)
    info = grid.info()
    assert info.layer_mask == (1 << 10) - 1 and info.rows > 40 and info.cols > 40
    g = R.Geometry(info.rows, info.cols, info.resolution, tuple(info.position))
    assert g.length == tuple(info.length)
    trav_id = pkg.GRID_LAYER_TERRAIN + pkg.TERRAIN_LAYERS.index("traversability")
    slope_id = pkg.GRID_LAYER_TERRAIN + pkg.TERRAIN_LAYERS.index("slope")
    ids = [trav_id, slope_id, pkg.GRID_LAYER_ELEVATION]
    fetched = {k: grid.layer(k) for k in ids}
    before = {k: v.tobytes() for k, v in fetched.items()}
    t = np.linspace(-9.0, 9.0, 60)                             # from outside the map, through it, and out again
    poses = np.c_[g.pos[0] + t, g.pos[1] + 0.37 * t, np.full_like(t, np.arctan(0.37))]
    rec, verts = pkg.footprint_polygons(poses, 1.1, 0.7)
    stats, n_cells, status, rinfo = grid.region_reduce(rec, ids, vertices=verts, threshold=0.8)
    regions = [("polygon", tuple(map(tuple, verts[4 * q:4 * q + 4]))) for q in range(len(poses))]
    want, w_n, w_status = R.regions_reduce(g, [fetched[k] for k in ids], regions, 0.8)
    got = words(stats)
    assert np.array_equal(status, w_status) and np.array_equal(n_cells, w_n)
    for name in ("n_finite", "n_below", "min", "max"):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["sum"].view(np.uint64), want["sum"].view(np.uint64))
    assert rinfo.n_ok > 30 and rinfo.n_empty > 2 and (stats["n_finite"][0] > 0).sum() > 30
    check_cells(grid, g, regions, "store")
    assert {k: grid.layer(k).tobytes() for k in ids} == before
    grid.close()
