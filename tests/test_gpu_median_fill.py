"""The median fill on the device (lio_median_fill, lio_kf_store_planning_map) through the C ABI against the numpy restatement
of grid_map_filters' MedianFillFilter (tests/median_fill_restate.py, pinned by tests/test_median_fill_cpu.py): the filled grid
as uint32 words (NaN payloads included), both masks and every count -- every comparison is an equality.  The shapes are the
smallest at which the kernels can still go wrong: below, at and just above the 32 x 8 tile, several tiles with a seam, single
rows and columns, and an 80 x 70 grid on which a 32-cell window is clamped on every side."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_fill_restate as R                                # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
RES = 0.2
COUNTS = ("fill_radius_cells", "existing_radius_cells", "n_nan_in", "n_mask", "n_filled", "n_filtered", "n_nan_out")


def same_words(got, want, what):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(u32) != want.view(u32)
    assert not diff.any(), (what, "words that differ:", int(diff.sum()), "first at", tuple(np.argwhere(diff)[0]))


@functools.lru_cache(maxsize=None)
def grid_of(rows, cols):
    g = R.make_grid(rows, cols, seed=rows * 100 + cols)
    g.setflags(write=False)
    return g


def radius_m(cells):
    """a radius that truncates to `cells`"""
    return (cells + 0.5) * RES


def check(pkg, grid, res, mask_in=None, **cfg):
    want = R.median_fill(grid, res, mask_in=mask_in, **cfg)
    filled, mask, cleaned, info = pkg.median_fill(grid, res, pkg.median_fill_default_config(**cfg), mask_in=mask_in, want_cleaned_mask=True)
    what = (grid.shape, cfg)
    assert (info.rows, info.cols) == grid.shape, what
    for name in COUNTS:
        print(name, getattr(info, name), want[name])
        assert getattr(info, name) == want[name], (what, name)
    same_words(mask, want["fill_mask"], (what, "fill mask"))
    if mask_in is None:
        same_words(cleaned, want["cleaned_mask"], (what, "cleaned mask"))
    else:
        assert cleaned is None
    same_words(filled, want["filled"], (what, "filled"))
    return want, info


def test_the_reference_test_case(pkg):
    """grid_map_filters/test/median_fill_filter_test.cpp"""
    g = np.ones((20, 20), f32)
    g[15:, 15:] = np.nan
    for r, c in ((0, 0), (10, 5), (2, 4), (6, 3), (11, 8), (3, 15), (10, 10)):
        g[r, c] = np.nan
    want, info = check(pkg, g, 0.02, fill_hole_radius=0.02, existing_value_radius=0.02, filter_existing_values=1, num_erode_dilation_iterations=4)
    assert (info.n_nan_in, info.n_filled, info.n_nan_out) == (32, 7, 25)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 40), (40, 1), (2, 2), (32, 8), (33, 9), (69, 19)])
def test_grid_sizes(pkg, rows, cols):
    check(pkg, grid_of(rows, cols), RES, fill_hole_radius=radius_m(2))


@pytest.mark.parametrize("n", [0, 1, 4, 15])
@pytest.mark.parametrize("rows,cols", [(33, 9), (69, 19)])
def test_iterations(pkg, rows, cols, n):
    check(pkg, grid_of(rows, cols), RES, fill_hole_radius=radius_m(2), num_erode_dilation_iterations=n)


@pytest.mark.parametrize("cells", [0, 1, 2, 5])
def test_radii(pkg, cells):
    want, info = check(pkg, grid_of(69, 19), RES, fill_hole_radius=radius_m(cells), num_erode_dilation_iterations=15)
    if cells == 0:                                             # a masked hole has an empty window: the canonical NaN
        holes = ~np.isfinite(grid_of(69, 19)) & (want["fill_mask"] != 0)
        assert holes.any() and info.n_filled == 0 and (want["filled"].view(u32)[holes] == R.QNAN_BITS).all()


def test_radius_of_32_cells_clamped_on_every_side(pkg):
    check(pkg, grid_of(80, 70), RES, fill_hole_radius=radius_m(32))
    check(pkg, grid_of(80, 70), RES, fill_hole_radius=radius_m(1), existing_value_radius=radius_m(32), filter_existing_values=1,
          num_erode_dilation_iterations=1)


@pytest.mark.parametrize("rows,cols", [(33, 9), (69, 19)])
def test_filter_existing_values(pkg, rows, cols):
    want, info = check(pkg, grid_of(rows, cols), RES, fill_hole_radius=radius_m(1), existing_value_radius=radius_m(2), filter_existing_values=1)
    assert info.n_filtered > 0


def test_truncated_radii_reach_the_kernels(pkg):
    want, info = check(pkg, grid_of(33, 9), 0.2, fill_hole_radius=0.6)
    assert info.fill_radius_cells == 2
    want, info = check(pkg, grid_of(33, 9), 0.1, fill_hole_radius=0.3, existing_value_radius=0.3, filter_existing_values=1)
    assert (info.fill_radius_cells, info.existing_radius_cells) == (2, 2)


def test_zeros_of_both_signs_even_counts_infinities_payloads(pkg):
    nan, inf = np.nan, np.inf
    g = np.array([[nan, -0.0, 0.0, nan, 0.0, -0.0, -0.0, nan, 1.0, inf, 2.0, -inf, 3.0, 3.0, nan, 3.0, 5.0, 4.0]], f32)
    g = np.vstack([g, g[:, ::-1], g]).copy()
    g.view(u32)[1, 4] = 0xffc00001
    ones = np.ones(g.shape, f32)
    for cells in (1, 2, 3):
        check(pkg, g, 1.0, mask_in=ones, fill_hole_radius=cells, existing_value_radius=1.0, filter_existing_values=cells == 2)
    want, _ = check(pkg, g, 1.0, mask_in=np.zeros(g.shape, f32), fill_hole_radius=2.0)
    same_words(want["filled"], g, "an all-zero mask copies the input")


def test_mask_of_a_previous_run(pkg):
    g = grid_of(33, 9)
    rng = np.random.default_rng(17)
    for m in (np.ones(g.shape, f32), np.zeros(g.shape, f32), (rng.uniform(size=g.shape) < 0.5).astype(f32) * f32(2.5)):
        want, info = check(pkg, g, RES, mask_in=m, fill_hole_radius=radius_m(2), existing_value_radius=radius_m(1), filter_existing_values=1)
        assert info.n_mask == int((m != 0).sum())
    want, _ = check(pkg, g, RES, mask_in=np.zeros(g.shape, f32), fill_hole_radius=radius_m(2))
    same_words(want["filled"], g, "an all-zero mask copies the input")
    nan_mask = np.zeros(g.shape, f32)
    nan_mask[0, 0] = np.nan                                    # NaN != 0.0f: fill
    want, info = check(pkg, g, RES, mask_in=nan_mask, fill_hole_radius=radius_m(2))
    assert info.n_mask == 1


def test_outputs_one_at_a_time(pkg):
    lib = pkg.load_library()
    g = np.asfortranarray(grid_of(69, 19))
    cfg = pkg.median_fill_default_config(fill_hole_radius=radius_m(2))
    want = R.median_fill(g, RES, fill_hole_radius=radius_m(2))
    for which in ("none", "fill_mask", "cleaned_mask"):
        filled, other = np.empty(g.shape, f32, order="F"), np.empty(g.shape, f32, order="F")
        info = pkg.MedianFillInfo()
        rc = lib.lio_median_fill(0, g.ctypes.data, 69, 19, RES, C.byref(cfg), None, filled.ctypes.data,
                                 other.ctypes.data if which == "fill_mask" else None, other.ctypes.data if which == "cleaned_mask" else None,
                                 C.byref(info))
        assert rc == 0, which
        same_words(filled, want["filled"], which)
        if which != "none":
            same_words(other, want[which], which)
        assert info.n_nan_out == want["n_nan_out"]


# ---- the one chain ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_store(pkg):
    """three keyframes on a jittered 0.1 m lattice over 15 m x 15 m, a dozen points in every 0.2 m cell, around one hole"""
    rng = np.random.default_rng(41)
    st = pkg.KeyframeStore()
    poses = []
    for k in range(3):
        x, y = np.meshgrid(np.arange(-7.5, 7.5, 0.1), np.arange(-7.5, 7.5, 0.1), indexing="ij")
        xy = np.c_[x.ravel(), y.ravel()] + rng.uniform(-0.04, 0.04, (x.size, 2))
        xy = xy[~((xy[:, 0] > 2.0) & (xy[:, 0] < 3.2) & (xy[:, 1] > 1.0) & (xy[:, 1] < 2.0))]       # a hole some 5 x 4 cells wide
        z = 0.04 * xy[:, 0] + 0.1 * np.sin(xy[:, 1]) + rng.normal(0, 0.01, len(xy))
        st.add(np.c_[xy, z, rng.uniform(0, 255, len(xy))].astype(f32))
        poses.append([0.0, 0.0, 0.0, 0.05 * k, 0.05 * k, 0.0])
    st.set_poses(0, np.array(poses, f32), times=np.arange(3) * 1.0)
    yield st
    st.close()


def same_struct(a, b, what):
    for name, _ in type(a)._fields_:
        x, y = getattr(a, name), getattr(b, name)
        x, y = (list(x), list(y)) if hasattr(x, "__len__") else (x, y)
        same = x == y or (isinstance(x, float) and x != x and y != y)
        assert same, (what, name, x, y)


def test_planning_map_is_the_steps_one_after_the_other(pkg, dense_store):
    """lio_kf_store_planning_map = lio_kf_store_height_map, lio_median_fill, then lio_terrain_layers and lio_sdf_build on the
    filled grid: every output and every info field.  The store is dense enough for the restatement to leave no hole, so the
    field under nan_policy = 0 is built from a height map with fill_holes = 0 -- which no call could do before."""
    st = dense_store
    pose = np.zeros(6, f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(resolution=RES, fill_holes=0)
    fill_kw = dict(fill_hole_radius=2.0, num_erode_dilation_iterations=8)
    fill = pkg.median_fill_default_config(**fill_kw)
    terrain = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)
    sdf_cfg = pkg.sdf_default_config(nan_policy=0)
    raw, hm_ref, lm_ref = st.height_map(pose, lm, hm)
    assert hm_ref.rows > 40 and hm_ref.cols > 40
    want = R.median_fill(raw, RES, **fill_kw)
    print("holes in the height map", want["n_nan_in"], "left by the restatement", want["n_nan_out"])
    assert want["n_nan_in"] > 0 and want["n_nan_out"] == 0     # the restatement decides: the hole is there and none is left
    chained = pkg.Sdf()
    out = st.planning_map(pose, lm, hm, fill, terrain, chained, sdf_cfg)
    # the steps
    filled, mask, _, fill_ref = pkg.median_fill(raw, RES, fill)
    layers_ref, terrain_ref = pkg.terrain_layers(filled, RES, hm_ref.length, hm_ref.position, terrain)
    direct = pkg.Sdf()
    sdf_ref = direct.build(filled, RES, hm_ref.length, hm_ref.position, sdf_cfg)
    assert out["grid"].tobytes() == raw.tobytes()
    same_words(out["filled"], want["filled"], "filled against the restatement")
    same_words(out["filled"], filled, "filled")
    same_words(out["fill_mask"], mask, "fill mask")
    same_struct(out["lm_info"], lm_ref, "lm_info")
    same_struct(out["hm_info"], hm_ref, "hm_info")
    same_struct(out["fill_info"], fill_ref, "fill_info")
    same_struct(out["terrain_info"], terrain_ref, "terrain_info")
    same_struct(out["sdf_info"], sdf_ref, "sdf_info")
    assert out["sdf_info"].n_nan == 0 and out["sdf_info"].layers >= 2
    for name in pkg.TERRAIN_LAYERS:
        same_words(out["layers"][name], layers_ref[name], name)
    nodes_ref = direct.nodes().tobytes()
    assert chained.nodes().tobytes() == nodes_ref
    # today's calls on the same store: the field is refused for the holes the height map has (none could be built), unless the
    # height map itself is extended
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.sdf_map(direct, pose, lm, hm, sdf_cfg)
    # each optional stage absent
    alone = st.planning_map(pose, lm, hm)
    assert alone["grid"].tobytes() == raw.tobytes() and alone["filled"] is None and alone["layers"] is None
    same_struct(alone["hm_info"], hm_ref, "hm_info, no stage")
    only_fill = st.planning_map(pose, lm, hm, fill, want_grid=False, want_fill_mask=False)
    assert only_fill["grid"] is None and only_fill["fill_mask"] is None
    same_words(only_fill["filled"], filled, "fill alone")
    same_struct(only_fill["fill_info"], fill_ref, "fill_info, fill alone")
    no_fill = st.planning_map(pose, lm, hm, None, terrain, chained, pkg.sdf_default_config(nan_policy=1))
    layers_raw, terrain_raw = pkg.terrain_layers(raw, RES, hm_ref.length, hm_ref.position, terrain)
    for name in pkg.TERRAIN_LAYERS:
        same_words(no_fill["layers"][name], layers_raw[name], name + " on the raw grid")
    same_struct(no_fill["terrain_info"], terrain_raw, "terrain_info on the raw grid")
    assert no_fill["sdf_info"].n_nan == want["n_nan_in"]
    no_sdf = st.planning_map(pose, lm, hm, fill, terrain)
    for name in pkg.TERRAIN_LAYERS:
        same_words(no_sdf["layers"][name], layers_ref[name], name + " without the field")
    no_terrain = st.planning_map(pose, lm, hm, fill, None, chained, sdf_cfg, want_filled=False)
    assert no_terrain["layers"] is None and chained.nodes().tobytes() == nodes_ref
    direct.close()
    chained.close()


def test_planning_map_with_holes_left_and_refusals(pkg, dense_store):
    """a pose turned by 0.4 rad looks past the corners of the mapped square: triangles the closing does not reach stay NaN"""
    st = dense_store
    pose = np.array([0.0, 0.0, 0.4, 0.0, 0.0, 0.0], f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(resolution=RES, fill_holes=0)
    fill_kw = dict(fill_hole_radius=0.4, num_erode_dilation_iterations=1)
    fill = pkg.median_fill_default_config(**fill_kw)
    raw, hm_ref, _ = st.height_map(pose, lm, hm)
    want = R.median_fill(raw, RES, **fill_kw)
    print("holes in the height map", want["n_nan_in"], "left by the restatement", want["n_nan_out"])
    assert want["n_nan_out"] > 0                               # the restatement decides: this pose leaves holes
    sdf = pkg.Sdf()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.planning_map(pose, lm, hm, fill, None, sdf, pkg.sdf_default_config(nan_policy=0))
    assert sdf.info.n_nan == want["n_nan_out"]
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # refused: the object holds no field
        sdf.nodes()
    out = st.planning_map(pose, lm, hm, fill, None, sdf, pkg.sdf_default_config(nan_policy=1))
    same_words(out["filled"], want["filled"], "filled")
    same_words(out["fill_mask"], want["fill_mask"], "fill mask")
    for name in COUNTS:
        assert getattr(out["fill_info"], name) == want[name], name
    assert out["sdf_info"].n_nan == want["n_nan_out"]
    direct = pkg.Sdf()
    direct.build(want["filled"], RES, hm_ref.length, hm_ref.position, pkg.sdf_default_config(nan_policy=1))
    assert sdf.nodes().tobytes() == direct.nodes().tobytes()
    direct.close()
    # refusals in the order of the existing chained calls
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.planning_map(pose, lm, pkg.height_map_default_config(fill_holes=2), fill)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.planning_map(pose, lm, hm, pkg.median_fill_default_config(num_erode_dilation_iterations=16))
    empty = pkg.KeyframeStore()
    e = empty.planning_map(pose, lm, hm, fill, pkg.terrain_default_config(), sdf, pkg.sdf_default_config())
    assert e["grid"].shape == (0, 0) and (e["hm_info"].rows, e["fill_info"].rows, e["terrain_info"].cols, e["sdf_info"].layers) == (0, 0, 0, 0)
    empty.close()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # an empty local map leaves no field
        sdf.nodes()
    sdf.close()


def test_the_older_store_entries_are_the_chain_with_one_stage(pkg, dense_store):
    """lio_kf_store_height_map, lio_kf_store_terrain_map and lio_kf_store_sdf against lio_kf_store_planning_map with only their
    stage requested: the bytes of the grid, of every layer and of the nodes, and every info field; the same on an empty store and
    without the grid; a grid buffer of one float is refused by both with rows and cols filled in."""
    pose = np.zeros(6, f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(resolution=RES, fill_holes=0)
    terrain = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)
    sdf_cfg = pkg.sdf_default_config(nan_policy=1)
    own, chained = pkg.Sdf(), pkg.Sdf()
    empty = pkg.KeyframeStore()

    def same_grid(a, b, what):
        assert (a is None) == (b is None), what
        if a is not None:
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), what

    for st, want_grid in ((dense_store, True), (dense_store, False), (empty, True), (empty, False)):
        what = ("empty store" if st is empty else "dense store", "grid" if want_grid else "no grid")
        grid, hm_info, lm_info = st.height_map(pose, lm, hm, want_grid=want_grid)
        out = st.planning_map(pose, lm, hm, want_grid=want_grid)
        same_grid(grid, out["grid"], (what, "height_map"))
        same_struct(hm_info, out["hm_info"], (what, "height_map, hm_info"))
        same_struct(lm_info, out["lm_info"], (what, "height_map, lm_info"))
        assert (hm_info.rows > 40 and hm_info.cols > 40) if st is dense_store else (hm_info.rows, hm_info.cols) == (0, 0), what

        grid, layers, info, hm_info, lm_info = st.terrain_map(pose, lm, hm, terrain, want_grid=want_grid)
        out = st.planning_map(pose, lm, hm, None, terrain, want_grid=want_grid)
        same_grid(grid, out["grid"], (what, "terrain_map"))
        for name in pkg.TERRAIN_LAYERS:
            same_grid(layers[name], out["layers"][name], (what, name))
        same_struct(info, out["terrain_info"], (what, "terrain_info"))
        same_struct(hm_info, out["hm_info"], (what, "terrain_map, hm_info"))
        same_struct(lm_info, out["lm_info"], (what, "terrain_map, lm_info"))
        assert (info.rows, info.cols) == (hm_info.rows, hm_info.cols), what

        grid, info, hm_info, lm_info = st.sdf_map(own, pose, lm, hm, sdf_cfg, want_grid=want_grid)
        out = st.planning_map(pose, lm, hm, None, None, chained, sdf_cfg, want_grid=want_grid)
        same_grid(grid, out["grid"], (what, "sdf_map"))
        same_struct(info, out["sdf_info"], (what, "sdf_info"))
        same_struct(hm_info, out["hm_info"], (what, "sdf_map, hm_info"))
        same_struct(lm_info, out["lm_info"], (what, "sdf_map, lm_info"))
        if st is dense_store:
            assert info.layers >= 2 and own.nodes().tobytes() == chained.nodes().tobytes(), what
        else:                                                  # an empty local map leaves no field in either object
            for sdf in (own, chained):
                with pytest.raises(pkg.LioError, match="ERR_ARG"):
                    sdf.nodes()
    empty.close()

    # a grid buffer of one float: refused, with rows x cols in the height map's info and in the stage's
    st, lib = dense_store, pkg.load_library()
    _, hm_ref, _ = st.height_map(pose, lm, hm)
    one = np.zeros(1, f32)
    layers = np.zeros(8 * hm_ref.rows * hm_ref.cols, f32)
    p = pose.ctypes.data_as(C.POINTER(C.c_float))
    lm_info, hm_info, t_info, s_info = pkg.LocalMapInfo(), pkg.HeightMapInfo(), pkg.TerrainInfo(), pkg.SdfInfo()
    rc = lib.lio_kf_store_terrain_map(st.h, C.byref(lm), p, C.byref(hm), C.byref(terrain), one.ctypes.data, one.size, layers.ctypes.data, layers.size,
                                      C.byref(lm_info), C.byref(hm_info), C.byref(t_info))
    assert rc == -1 and b"grid holds fewer cells" in lib.lio_last_error()
    assert (hm_info.rows, hm_info.cols) == (t_info.rows, t_info.cols) == (hm_ref.rows, hm_ref.cols)
    hm_info = pkg.HeightMapInfo()
    rc = lib.lio_kf_store_sdf(st.h, C.byref(lm), p, C.byref(hm), C.byref(sdf_cfg), one.ctypes.data, one.size, own.h, C.byref(lm_info),
                              C.byref(hm_info), C.byref(s_info))
    assert rc == -1 and b"grid holds fewer cells" in lib.lio_last_error()
    assert (hm_info.rows, hm_info.cols) == (s_info.rows, s_info.cols) == (hm_ref.rows, hm_ref.cols)
    own.close()
    chained.close()
