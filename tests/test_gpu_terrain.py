"""The terrain layers on the device (lio_terrain_layers, lio_kf_store_terrain_map) through the C ABI against the numpy
restatement of tests/terrain_restate.py, which tests/test_terrain_cpu.py pins.  The checks are stage-wise: every layer is
compared with the restatement applied to the DEVICE's own preceding layers, so that a one-ulp acosf does not leak into the
checks of later stages.  "Identical" means: the same NaN mask and the same bits.  Parity with grid_map, EigenLab and Eigen
themselves is unpinned (none can be built here)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_restate as T                                    # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

# tests/test_terrain_cpu.py::test_eigen_solver_against_lapack: 1.697 measured 2026-10-18 over the well-conditioned cells of
# scene A (seed 5) at positions (0, 0) and (60, -35), radii 0.3 and 0.6
K_EIGEN = 1.7
# The device's fp64 normal may sit 8 K 2^-53 |sumSquared / n|_F / (l1 - l0) from the restatement's: the margin of 8 covers
# the device's atan2 / cos / sin differing from the host's by a few ulp.  The device stores floats: a component within `bar`
# of the restatement's fp64 component rounds, rounding being monotonic, to a float in [f32(ref - bar), f32(ref + bar)].
AREA_MARGIN = 8.0
# slope against float(arccos(double(normal_z))): no accuracy figure for acosf is in the ROCm installation's documents or
# headers, so this is the project's existing derived 2 fp32 ulp bar, the restatement's rounding included
ACOS_ULPS = 2
TILE_ROWS, TILE_COLS = 32, 8                                   # LIO_TILE_ROWS x LIO_TILE_COLS of csrc/lio_gridtile.h


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_identical(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), (what, "NaN masks differ in", int((nan_g != nan_w).sum()))
    diff = bits(got)[~nan_g] != bits(want)[~nan_w]
    assert not diff.any(), (what, "cells that differ:", int(diff.sum()))


def device(pkg, grid, res, pos, **cfg):
    rows, cols = grid.shape
    return pkg.terrain_layers(grid, res, (rows * res, cols * res), pos, pkg.terrain_default_config(**cfg))


@functools.lru_cache(maxsize=None)
def area_reference(key, pos, res, radius, axis):
    """the restatement's area normals and the conditioning of every cell, once per scene"""
    grid = GRIDS[key]
    G = T.Geom(grid.shape[0], grid.shape[1], res, pos)
    return T.normals_area(grid, G, radius, axis), T.conditioning(grid, G, radius)


GRIDS = {}


def check_area_normals(d, info, key, grid, res, pos, radius, axis, what, max_ill=None):
    (nx, ny, nz), counts = area_reference(key, pos, res, radius, axis)[0]
    cond = area_reference(key, pos, res, radius, axis)[1]
    got = np.stack([d["normal_x"], d["normal_y"], d["normal_z"]], -1)
    ref32 = np.stack([nx, ny, nz], -1)
    assert np.array_equal(np.isnan(got), np.isnan(ref32)), what          # written exactly where the centre is finite
    assert (info.n_normal_cells, info.n_few_points, info.n_degenerate) == (counts["n_normal_cells"], counts["n_few_points"], counts["n_degenerate"]), what
    n_ill, n_well, n_same = 0, 0, 0
    for r, c in zip(*np.nonzero(np.isfinite(grid))):
        if (r, c) not in cond or not cond[(r, c)][3][1] > 1e-8:          # fewer than 3 points or degenerate: UnitZ, flipped
            assert np.array_equal(bits(got[r, c]), bits(ref32[r, c])), (what, r, c)
            continue
        w, v, fro, ev, v0 = cond[(r, c)]
        if not T.well_conditioned(w):
            n_ill += 1
            assert np.isfinite(got[r, c]).all()
            continue
        ref = v0 if v0[axis] >= 0.0 else -v0
        bar = AREA_MARGIN * K_EIGEN * 2.0 ** -53 * fro / (w[1] - w[0])
        lo, hi = (ref - bar).astype(f32), (ref + bar).astype(f32)
        n_well += 1
        n_same += int(np.array_equal(bits(got[r, c]), bits(ref32[r, c])))
        assert (lo <= got[r, c]).all() and (got[r, c] <= hi).all(), (what, r, c, got[r, c], ref, bar)
    n_finite = int(np.isfinite(grid).sum())
    print(f"  {what}: area normals, {n_same} of {n_well} well-conditioned cells bit-equal to the restatement's floats, {n_ill} of {n_finite} "
          f"finite cells ill-conditioned ({100.0 * n_ill / max(n_finite, 1):.2f} %)")
    if max_ill is not None:
        assert n_ill <= max_ill * n_finite, what


def check_stages(pkg, key, grid, res, pos, what="", max_ill=None, **cfg):
    """one call, every stage against the restatement of the device's preceding layers -> (layers, info)"""
    GRIDS[key] = grid
    p = dict(T.DEFAULTS, **cfg)
    G = T.Geom(grid.shape[0], grid.shape[1], res, pos)
    d, info = device(pkg, grid, res, pos, **cfg)
    assert (info.rows, info.cols, info.n_valid_cells) == (G.rows, G.cols, int(np.isfinite(grid).sum())), what
    assert_identical(d["smooth"], T.smooth(grid, G, p["smooth_radius"]), what + " smooth")
    assert_identical(d["roughness"], T.roughness_of(grid, d["smooth"]), what + " roughness")
    fallback = p["normal_method"] == 0 and p["normal_radius"] <= 0
    assert info.normal_method_used == int(fallback)
    if p["normal_method"] == 1 or fallback:
        (nx, ny, nz), counts = T.normals_raster(grid, G, p["normal_axis"])
        for name, want in (("normal_x", nx), ("normal_y", ny), ("normal_z", nz)):
            assert_identical(d[name], want, f"{what} raster {name}")
        assert (info.n_normal_cells, info.n_few_points, info.n_degenerate) == (counts["n_normal_cells"], 0, 0), what
    else:
        check_area_normals(d, info, key, grid, res, tuple(pos), p["normal_radius"], p["normal_axis"], what, max_ill)
    want = T.slope_of(d["normal_z"])
    assert np.array_equal(np.isnan(d["slope"]), np.isnan(want)), what
    m = ~np.isnan(want)
    ulps = np.abs(bits(d["slope"])[m].astype(np.int64) - bits(want)[m].astype(np.int64))      # slopes are not negative
    print(f"  {what}: slope, largest distance to float(arccos(double(normal_z))) {int(ulps.max()) if m.any() else 0} ulp "
          f"({int((ulps > 0).sum())} of {int(m.sum())} cells differ)")
    assert not m.any() or ulps.max() <= ACOS_ULPS, what
    win = T.edge_window_size(p["edge_window_length"], res, p["edge_window_size"])
    assert info.edge_window_size == win, what
    assert_identical(d["edges"], T.edges_of(d["slope"], win), what + " edges")
    assert_identical(d["traversability"], T.traversability_of(d["slope"], d["roughness"], p["slope_critical"], p["roughness_critical"],
                                                               p["slope_weight"], p["roughness_weight"]), what + " traversability")
    return d, info


@pytest.mark.parametrize("pos", [(0.0, 0.0), (60.0, -35.0)])
@pytest.mark.parametrize("radius", [0.3, 0.6])
def test_scene_a(pkg, pos, radius):
    """48 x 36 at 0.25 m: a tilted plane with noise, a box, a spike, 8 % holes and a 4 x 5 hole; the covariance's
    cancellation grows with the coordinates.  Ill-conditioned cells: at most 5 % (1.47 % at radius 0.3, 0 % at 0.6 on the host)."""
    grid = T.scene_a(pos)
    kw = dict(normal_radius=radius, smooth_radius=0.6, edge_window_length=0.75)
    check_stages(pkg, ("A", pos), grid, 0.25, pos, f"scene A {pos} radius {radius}", max_ill=0.05, **kw)
    if radius == 0.3:                                          # the raster normals do not depend on the radius
        check_stages(pkg, ("A", pos), grid, 0.25, pos, f"scene A {pos} raster", normal_method=1, **kw)


def test_circle_edges(pkg):
    """the 9 x 7 grid of the CPU test, radii at which membership is decided by the rounding of the centres, and one circle in
    which another visiting order gives another float"""
    pos, res = (3.7, -12.3), 0.25
    G = T.Geom(9, 7, res, pos)
    rng = np.random.default_rng(9)
    grid = rng.normal(0, 1, (9, 7)).astype(f32)
    assert T.circle(G, 4, 3, res) == [(3, 3), (4, 2), (4, 3), (4, 4), (5, 3)]
    grid[3, 3], grid[4, 2], grid[4, 3], grid[4, 4], grid[5, 3] = 2.0 ** 40, 0.0, 0.0, -2.0 ** 40, 2.0 ** -14
    in_order = f32((((2.0 ** 40 + 0.0) + 0.0) - 2.0 ** 40 + 2.0 ** -14) / 5.0)
    row_fastest = f32((((0.0 + 2.0 ** 40) + 0.0) + 2.0 ** -14 - 2.0 ** 40) / 5.0)           # (4,2) (3,3) (4,3) (5,3) (4,4)
    assert in_order == f32(2.0 ** -14 / 5.0) and row_fastest == 0.0
    for cells in (0.5, 1.0, math.sqrt(2.0), 2.0, 2.5):
        d, info = device(pkg, grid, res, pos, smooth_radius=cells * res, normal_method=1)
        want = T.smooth(grid, G, cells * res)
        assert_identical(d["smooth"], want, f"radius {cells} cells")
        if cells == 1.0:
            assert d["smooth"][4, 3] == in_order


def test_tile_seams(pkg):
    """two tiles and a remainder in both directions, every value distinct, a radius of 3 cells and a 7-cell window"""
    rows, cols, res, pos = 2 * TILE_ROWS + 5, 2 * TILE_COLS + 3, 0.25, (-7.3, 21.9)
    rng = np.random.default_rng(21)
    grid = (rng.permutation(rows * cols).reshape(rows, cols) * 0.001).astype(f32)
    assert len(np.unique(grid)) == rows * cols
    kw = dict(smooth_radius=0.75, normal_radius=0.75, edge_window_size=7)
    d, info = check_stages(pkg, "seams", grid, res, pos, "seams raster", normal_method=1, **kw)
    assert info.edge_window_size == 7 and info.n_normal_cells == (rows - 2) * (cols - 2)
    check_stages(pkg, "seams", grid, res, pos, "seams area", **kw)


@pytest.mark.parametrize("case, cfg", [
    ("a smooth circle of 1 cell under the halo of area normals of 3 cells", dict(smooth_radius=0.25, normal_radius=0.75, edge_window_length=0.75)),
    ("a smooth circle of 32 cells, raster normals: the largest tile", dict(smooth_radius=8.0, normal_method=1, edge_window_length=0.75)),
    ("a window of 65: the largest margin", dict(smooth_radius=0.5, normal_method=1, edge_window_size=65)),
])
def test_smooth_and_edges_are_the_grid_filters_cells(pkg, case, cfg):
    """33 x 9, one row and one column past a tile, with holes and a NaN border column: `smooth` is Grid.filter_radius(GF_MEAN)
    and `edges` is Grid.filter_window(GW_STDDEV, GW_CROP) on the device's slope layer, every word with its NaN payload, and
    every layer is the restatement's under the bars of check_stages"""
    rows, cols, res, pos = TILE_ROWS + 1, TILE_COLS + 1, 0.25, (-7.3, 21.9)
    rng = np.random.default_rng(33)
    x, y = np.meshgrid(np.arange(rows) * res, np.arange(cols) * res, indexing="ij")
    grid = (0.08 * x - 0.05 * y + rng.normal(0, 0.02, x.shape)).astype(f32)
    grid[rng.uniform(size=grid.shape) < 0.1] = np.nan
    grid[:, -1] = np.nan
    d, info = check_stages(pkg, ("33 x 9", case), grid, res, pos, case, **cfg)
    g = pkg.Grid()
    g.set_layers(np.stack([grid, d["slope"]]), res, (rows * res, cols * res), pos)
    g.filter_radius(0, 2, pkg.GF_MEAN, cfg["smooth_radius"])
    assert np.array_equal(bits(g.layer(2)), bits(d["smooth"])), case
    finfo = g.filter_window(1, 3, pkg.GW_STDDEV, pkg.GW_CROP, info.edge_window_size, 0.0)
    assert finfo["window_size"] == info.edge_window_size == cfg.get("edge_window_size", 3)
    assert np.array_equal(bits(g.layer(3)), bits(d["edges"])), case
    g.close()


def test_borders_and_holes(pkg):
    res, pos = 0.2, (1.3, -0.7)
    rng = np.random.default_rng(4)
    kw = dict(smooth_radius=0.45, normal_radius=0.45, edge_window_length=0.6)
    # a NaN centre among valid neighbours
    grid = rng.normal(0, 0.05, (5, 5)).astype(f32)
    grid[2, 2] = np.nan
    d, info = check_stages(pkg, "hole", grid, res, pos, "NaN centre, raster", normal_method=1, **kw)
    assert np.isfinite(d["smooth"][2, 2]) and np.isnan(d["roughness"][2, 2])
    assert np.isfinite(d["normal_z"][2, 2]) and np.isfinite(d["slope"][2, 2])               # case 5 writes a normal
    assert d["traversability"][2, 2] == 0.0                                                 # no roughness: 0, not NaN
    d, info = check_stages(pkg, "hole", grid, res, pos, "NaN centre, area", **kw)
    assert np.isnan(d["normal_z"][2, 2]) and np.isnan(d["slope"][2, 2]) and d["traversability"][2, 2] == 0.0
    assert info.n_normal_cells == 24 and not np.isnan(d["traversability"]).any()
    # windows and circles without a valid cell
    grid = np.full((12, 11), np.nan, f32)
    grid[:3, :4] = rng.normal(0, 0.05, (3, 4))
    d, info = check_stages(pkg, "empty", grid, res, pos, "empty windows", **kw)
    assert np.isnan(d["edges"][8:, 7:]).all() and np.isnan(d["smooth"][8:, 7:]).all() and (d["traversability"][8:, 7:] == 0).all()
    assert np.isfinite(d["edges"][:3, :4]).all()
    # grids without an interior: no raster normal, edges still computed (NaN without slope, finite with the area normals)
    for shape in ((1, 5), (5, 1), (2, 2)):
        grid = rng.normal(0, 0.05, shape).astype(f32)
        d, info = check_stages(pkg, ("thin", shape), grid, res, pos, f"{shape} raster", normal_method=1, **kw)
        assert info.n_normal_cells == 0 and np.isnan(d["normal_z"]).all() and np.isnan(d["edges"]).all()
        d, info = check_stages(pkg, ("thin", shape), grid, res, pos, f"{shape} area", **kw)
        assert info.n_normal_cells == shape[0] * shape[1] and np.isfinite(d["edges"]).all()
    # no cell at all
    for shape in ((0, 6), (6, 0)):
        d, info = device(pkg, np.zeros(shape, f32), res, pos)
        assert (info.rows, info.cols) == shape and all(v.shape == shape for v in d.values()) and len(d) == 8


def test_few_points_and_degenerate(pkg):
    res, pos = 0.25, (0.0, 0.0)
    kw = dict(smooth_radius=0.5, normal_radius=0.5, edge_window_length=0.75)
    # an isolated cell: fewer than 3 points, UnitZ
    grid = np.full((7, 7), np.nan, f32)
    grid[3, 3] = 0.4
    d, info = check_stages(pkg, "isolated", grid, res, pos, "isolated cell", **kw)
    assert (info.n_normal_cells, info.n_few_points, info.n_degenerate) == (1, 1, 0)
    assert (d["normal_x"][3, 3], d["normal_y"][3, 3], d["normal_z"][3, 3]) == (0.0, 0.0, 1.0) and d["slope"][3, 3] == 0.0
    # one valid row of five cells, z linear in x: collinear points, eigenvalue(1) is rounding noise, UnitZ
    grid = np.full((7, 7), np.nan, f32)
    grid[1:6, 3] = 0.5 * np.arange(5)
    d, info = check_stages(pkg, "row", grid, res, pos, "collinear row", **kw)
    assert (info.n_normal_cells, info.n_few_points, info.n_degenerate) == (5, 0, 5)
    assert (d["normal_z"][1:6, 3] == 1.0).all() and (d["normal_x"][1:6, 3] == 0.0).all()
    # normal_axis = 0 on a plane rising with x: the z-up normal has a negative x component and is flipped
    G = T.Geom(8, 9, res, pos)
    x = np.array([T.centre(G, 0, i) for i in range(8)])
    grid = np.repeat((0.5 * x)[:, None], 9, axis=1).astype(f32)
    for method in (0, 1):
        up, _ = check_stages(pkg, "plane", grid, res, pos, f"plane, axis z, method {method}", normal_method=method, **kw)
        dx, _ = check_stages(pkg, "plane", grid, res, pos, f"plane, axis x, method {method}", normal_method=method, normal_axis=0, **kw)
        inner = (slice(1, -1), slice(1, -1))
        assert (up["normal_x"][inner] < 0).all() and (dx["normal_x"][inner] > 0).all() and (dx["normal_z"][inner] < 0).all()
        assert (dx["slope"][inner] > math.pi / 2).all() and (dx["traversability"][inner] == 0).all()


@pytest.fixture(scope="module")
def small_store(pkg):
    rng = np.random.default_rng(37)                            # the store of tests/test_gpu_heightmap.py, its last three keyframes
    st = pkg.KeyframeStore()
    poses = []
    for k in range(3):
        n = 480 + 7 * k
        xy = rng.uniform(-9, 9, (n, 2))
        cloud = np.c_[xy, 0.04 * xy[:, 0] + rng.normal(0, 0.02, n) + (rng.uniform(size=n) < 0.1) * rng.uniform(0, 2.5, n), rng.uniform(0, 255, n)]
        st.add(cloud.astype(f32))
        poses.append([0.01 * k, -0.005 * k, 0.1 * k, 0.5 * k, 0.2 * k, 0.02 * k])
    st.set_poses(0, np.array(poses, f32), times=np.arange(3) * 1.0)
    yield st
    st.close()


def test_from_the_store(pkg, small_store):
    st = small_store
    pose = np.array([0.02, -0.01, 0.4, 2.0, 0.8, 0.1], f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(roll=0.02, pitch=-0.01, resolution=0.2, fill_holes=1)
    scaled = dict(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)            # the yaml's lengths at 0.2 m: times 10
    cfg = pkg.terrain_default_config(**scaled)
    grid_ref, hm_ref, lm_ref = st.height_map(pose, lm, hm)
    grid, layers, info, hm_info, lm_info = st.terrain_map(pose, lm, hm, cfg)
    assert info.rows > 10 and (info.rows, info.cols) == (hm_ref.rows, hm_ref.cols) and grid.tobytes() == grid_ref.tobytes()
    for name, _ in pkg.HeightMapInfo._fields_:
        a, b = getattr(hm_info, name), getattr(hm_ref, name)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    for name, _ in pkg.LocalMapInfo._fields_:
        assert getattr(lm_info, name) == getattr(lm_ref, name), name
    direct, info_d = pkg.terrain_layers(grid_ref, 0.2, hm_ref.length, hm_ref.position, cfg)
    assert list(layers) == list(pkg.TERRAIN_LAYERS) == list(direct)
    for name in pkg.TERRAIN_LAYERS:
        assert layers[name].tobytes() == direct[name].tobytes(), name
    for name, _ in pkg.TerrainInfo._fields_:
        assert getattr(info, name) == getattr(info_d, name), name
    assert info.n_valid_cells == hm_ref.n_valid_cells + hm_ref.n_filled_cells and info.n_normal_cells == info.n_valid_cells
    assert np.isfinite(layers["slope"]).sum() == info.n_normal_cells and not np.isnan(layers["traversability"]).any()
    # a subset of the layers, without the elevation grid; and the whole again
    mask = (1 << 0) | (1 << 4) | (1 << 7)
    none, some, info_s, _, _ = st.terrain_map(pose, lm, hm, pkg.terrain_default_config(layers=mask, **scaled), want_grid=False)
    assert none is None and list(some) == ["smooth", "slope", "traversability"]
    for name in some:
        assert some[name].tobytes() == layers[name].tobytes(), name
    grid2, layers2, info2, _, _ = st.terrain_map(pose, lm, hm, cfg)
    assert grid2.tobytes() == grid.tobytes() and all(layers2[n].tobytes() == layers[n].tobytes() for n in layers)
    # the height map alone still gives the same bytes; an empty store gives no grid
    again, _, _ = st.height_map(pose, lm, hm)
    assert again.tobytes() == grid_ref.tobytes()
    empty = pkg.KeyframeStore()
    g, l, i, h, m = empty.terrain_map(pose)
    assert g.shape == (0, 0) and (i.rows, i.cols, h.n_in, m.n_summed) == (0, 0, 0, 0) and all(v.shape == (0, 0) for v in l.values())
    empty.close()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.terrain_map(pose, lm, hm, pkg.terrain_default_config(edge_window_size=2))
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.terrain_map(pose, lm, pkg.height_map_default_config(fill_holes=2), cfg)


def test_arguments(pkg):
    lib = pkg.load_library()
    res, pos = 0.25, (2.0, 3.0)
    grid = T.scene_a(pos)[:20, :14].copy()
    # refused, never clamped
    nan, inf = float("nan"), float("inf")
    for kw in (dict(normal_radius=nan), dict(normal_radius=-0.1), dict(smooth_radius=inf), dict(smooth_radius=-1.0), dict(edge_window_length=nan),
               dict(edge_window_length=-0.5), dict(slope_critical=nan), dict(slope_critical=-0.6), dict(roughness_critical=inf),
               dict(roughness_critical=-0.1), dict(slope_weight=-0.5), dict(slope_weight=inf), dict(roughness_weight=nan), dict(roughness_weight=-1.0),
               dict(normal_method=-1), dict(normal_method=2), dict(normal_axis=-1), dict(normal_axis=3), dict(edge_window_size=4), dict(edge_window_size=-3),
               dict(smooth_radius=32.5 * res), dict(normal_radius=33 * res), dict(edge_window_size=67), dict(edge_window_length=70 * res),
               dict(layers=0x100)):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            device(pkg, grid, res, pos, **kw)
    cfg = pkg.terrain_default_config()
    for bad_res in (5e-5, nan):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            pkg.terrain_layers(grid, bad_res, (20 * res, 14 * res), pos, cfg)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        pkg.terrain_layers(grid, res, (20 * res, 15 * res), pos, cfg)                      # a length that is not size * resolution
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        pkg.terrain_layers(grid, res, (20 * res, 14 * res), (nan, 0.0), cfg)
    # the limits themselves are served: a radius of 32 cells, a window of 65
    small = grid[:6, :5].copy()
    check_stages(pkg, "limit", small, res, pos, "32 cells", smooth_radius=32 * res, normal_radius=32 * res, edge_window_size=65)
    # area with a radius of 0 falls back to raster, as the reference does
    d, info = check_stages(pkg, "fallback", grid, res, pos, "fallback", normal_radius=0.0, smooth_radius=0.5)
    r, info_r = device(pkg, grid, res, pos, normal_method=1, normal_radius=0.0, smooth_radius=0.5)
    assert info.normal_method_used == 1 and info_r.normal_method_used == 0
    assert all(d[n].tobytes() == r[n].tobytes() for n in d)
    # too small a buffer: refused with the size, nothing written; a subset needs less
    g = np.asfortranarray(grid)
    ln, ps = (C.c_double * 2)(20 * res, 14 * res), (C.c_double * 2)(*pos)
    out = np.full(8 * g.size, 7.0, f32)
    info = pkg.TerrainInfo()
    call = lambda c, cap: lib.lio_terrain_layers(0, g.ctypes.data, 20, 14, res, ln, ps, C.byref(c), out.ctypes.data, cap, C.byref(info))
    assert call(cfg, 8 * g.size - 1) == -1 and (info.rows, info.cols) == (20, 14) and (out == 7.0).all()
    two = pkg.terrain_default_config(layers=(1 << 1) | (1 << 6), smooth_radius=0.5, normal_radius=0.5)
    assert call(two, 2 * g.size - 1) == -1 and call(two, 2 * g.size) == 0 and (out[2 * g.size:] == 7.0).all()
    full, _ = device(pkg, grid, res, pos, smooth_radius=0.5, normal_radius=0.5)
    assert out[:g.size].tobytes() == np.asfortranarray(full["normal_x"]).tobytes(order="F")
    assert out[g.size:2 * g.size].tobytes() == np.asfortranarray(full["edges"]).tobytes(order="F")
    assert lib.lio_terrain_layers(0, g.ctypes.data, 20, 14, res, ln, ps, None, out.ctypes.data, out.size, C.byref(info)) == -1
    check_stages(pkg, "after", grid, res, pos, "after the refusals", smooth_radius=0.5, normal_radius=0.5)
