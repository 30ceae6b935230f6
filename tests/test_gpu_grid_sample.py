"""The resident planning layers and their sampling on the device (lio_grid_*, lio_kf_store_planning_grid) through the C ABI
against the restatement of GridMap::atPosition (tests/grid_sample_restate.py, pinned by tests/test_grid_sample_cpu.py): the
values as uint32 words (NaN for NaN only where an interpolating method computed it), the method bytes and the counts.  The
shapes are the smallest at which the index work can still go wrong: 1 x 1 up to 5 x 4 grids on which every tap leaves the
grid somewhere, non-square so that a row / column swap shows; n up to 100 003 so that the last wave and block are partial."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_restate as R                                # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
METHODS = (R.NEAREST, R.LINEAR, R.CUBIC_CONVOLUTION, R.CUBIC)


def same_values(got_v, got_m, want_v, want_m, what):
    assert got_v.shape == want_v.shape and got_m.shape == want_m.shape, what
    diff_m = got_m != want_m
    assert not diff_m.any(), (what, "method bytes that differ:", int(diff_m.sum()), "first at", tuple(np.argwhere(diff_m)[0]))
    computed = (want_m != R.NEAREST) & (want_m != R.OUTSIDE)
    same = (got_v.view(u32) == want_v.view(u32)) | (computed & np.isnan(got_v) & np.isnan(want_v))
    assert same.all(), (what, "words that differ:", int((~same).sum()), "first at", tuple(np.argwhere(~same)[0]))


def check(grid, g, layers, pts, method, border=0, ids=None, what=None):
    ids = list(range(len(layers))) if ids is None else ids
    vals, used, info = grid.sample(pts, ids, method=method, border_mode=border)
    want_v, want_m, want_info = R.sample(g, [layers[k] for k in ids], pts, method, border)
    what = (what, g.size, "method", method, "border", border)
    same_values(vals, used, want_v, want_m, what)
    print(what, "outside", info.n_outside, "per method", list(info.n_method))
    assert info.n_outside == want_info["n_outside"] and list(info.n_method) == want_info["n_method"], what
    return vals, used, info


def upload(pkg, g, arrays):
    grid = pkg.Grid()
    grid.set_layers(np.stack(arrays), g.res, g.length, g.pos)
    return grid


def plain_layer(rows, cols):
    return (1.0 + np.arange(rows * cols).reshape(rows, cols) * 0.37).astype(f32)         # distinct values


def holes_layer(rows, cols, seed):
    rng = np.random.default_rng(seed)
    a = (plain_layer(rows, cols) + rng.uniform(0, 0.1, (rows, cols))).astype(f32)
    k = a.size
    a.flat[1 % k] = np.nan
    a.flat[k // 2] = np.inf
    a.flat[k - 2] = -np.inf
    a.view(u32).flat[3 % k] = 0xffc01234                        # a NaN with a payload
    return a


# ---- 1
def test_reference_held_values(pkg):
    """GridMapTest.cpp:448-494, from the device"""
    g = R.Geometry(3, 3, 1.0)
    grid = upload(pkg, g, [np.array([[0.5, 3.8, 2.0], [2.1, 1.0, 2.0], [1.0, 2.0, 2.0]], f32)])
    v, m, _ = grid.sample([(1.35, -0.4), (-0.3, 0.0)])
    assert [float(x) for x in v[0]] == [float(f32(3.8)), 1.0] and list(m[0]) == [R.NEAREST, R.NEAREST]
    v, m, info = grid.sample([(-0.5, -1.2), (-0.5, 0.0), (0.69, 0.38)], method=R.LINEAR)
    print("linear", v[0].tolist(), m[0].tolist())
    assert float(v[0, 0]) == 2.0 and m[0, 0] == R.NEAREST      # close to the border: reverting to nearest
    assert float(v[0, 1]) == 1.5 and m[0, 1] == R.LINEAR
    assert abs(float(v[0, 2]) - 2.19632) <= 1e-7 and m[0, 2] == R.LINEAR
    assert (info.n_outside, list(info.n_method)) == (0, [1, 2, 0, 0])
    grid.close()


# ---- 2
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", ["flat", "saddle", "poly", "sine"])
def test_analytic_worlds(pkg, kind, seed):
    """the 20 x 20 and 30 x 30 maps and one 300 x 300: the device's own values within the reference's 1e-3 of the analytic
    surface, and the same values bit-identical to the restatement"""
    g, layer, f, pts = R.analytic_world(kind, seed, n_points=400)
    truth = f(pts[:, 0], pts[:, 1])
    grid = upload(pkg, g, [layer])
    layers = [R.Layer(layer)]
    for method in (R.CUBIC_CONVOLUTION, R.CUBIC):
        vals, used, _ = check(grid, g, layers, pts, method, what=kind)
        err = float(np.abs(vals[0].astype(np.float64) - truth).max())
        print(kind, "seed", seed, "method", method, "max abs error on the device", err)
        assert (used == method).all() and err <= R.MAX_ABS_ERROR
    grid.close()


# ---- 3
@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 2), (1, 7), (5, 4), (4, 5)])
def test_border_lattice(pkg, rows, cols):
    """every cell centre, edge, corner and quadrant, both map edges and one step beyond them, all methods, both border modes:
    the linear wraps, the unsigned wraps of both cubic methods, the exclusive low and inclusive high edge, LIO_GRID_OUTSIDE"""
    g = R.Geometry(rows, cols, 0.25, (0.25, -0.125))          # binary fractions: the lattice's edges are the cells' edges exactly
    a = plain_layer(rows, cols)
    grid = upload(pkg, g, [a])
    layers = [R.Layer(a)]
    pts = R.border_lattice(g)
    for method in METHODS:
        for border in (0, 1):
            vals, used, info = check(grid, g, layers, pts, method, border)
            assert info.n_outside > 0 and (used != R.OUTSIDE).any()
            if border == 1 and method != R.NEAREST:
                assert info.n_method[R.NEAREST] == 0           # clamped: nothing fails
    # the labelled deviation: in cell (0, cols - 1), up and right of its centre, tap (0, cols) has the linear index rows x cols,
    # which the reference lets pass; here the query falls back to nearest
    x, y = R.position_from_index(g, (0, cols - 1))
    v, m, _ = grid.sample([(x + 0.05, y - 0.05)], method=R.LINEAR)
    assert m[0, 0] == R.NEAREST and v[0, 0] == a[0, cols - 1]
    # the edges themselves
    hi = (g.pos[0] + 0.5 * g.length[0], g.pos[1] + 0.5 * g.length[1])
    lo = (g.pos[0] - 0.5 * g.length[0], g.pos[1] - 0.5 * g.length[1])
    v, m, _ = grid.sample([hi, lo, (hi[0], lo[1]), (lo[0], hi[1])])
    assert m[0].tolist() == [R.NEAREST, R.OUTSIDE, R.OUTSIDE, R.OUTSIDE] and v[0, 0] == a[0, 0]
    assert (v[0, 1:].view(u32) == R.QNAN_BITS).all()
    grid.close()


# ---- 4
@pytest.mark.parametrize("rows,cols", [(5, 4), (12, 9)])
def test_holes(pkg, rows, cols):
    """NaN, +inf, -inf and a NaN with a payload: the fall-back chains and method bytes as the restatement says"""
    g = R.Geometry(rows, cols, 0.2)
    a = holes_layer(rows, cols, 7)
    grid = upload(pkg, g, [a])
    layers = [R.Layer(a)]
    pts = R.border_lattice(g)
    for method in METHODS:
        for border in (0, 1):
            vals, used, info = check(grid, g, layers, pts, method, border)
            if method >= R.CUBIC_CONVOLUTION and (rows, cols) == (12, 9):
                assert info.n_method[method] > 0 and info.n_method[R.LINEAR] > 0          # some cubic taps touch a hole, some do not
                assert np.isfinite(vals[used == method]).all()
    vals, used, _ = grid.sample(pts)
    assert (vals.view(u32) == 0xffc01234).any()                # nearest: the cell's bits
    grid.close()


# ---- 5
def test_far_from_the_origin(pkg):
    g = R.Geometry(12, 9, 0.2, (1e4, -3e4))
    rng = np.random.default_rng(11)
    a = rng.uniform(-5, 5, g.size).astype(f32)
    grid = upload(pkg, g, [a])
    layers = [R.Layer(a)]
    pts = np.r_[R.border_lattice(g), np.c_[rng.uniform(1e4 - 1.3, 1e4 + 1.3, 300), rng.uniform(-3e4 - 1.0, -3e4 + 1.0, 300)]]
    for method in METHODS:
        check(grid, g, layers, pts, method)
    check(grid, g, layers, pts, R.CUBIC, 1)
    grid.close()


# ---- 6
def test_several_layers(pkg):
    g = R.Geometry(12, 9, 0.2)
    arrays = [holes_layer(12, 9, 1), plain_layer(12, 9), holes_layer(12, 9, 2)[::-1].copy()]
    grid = upload(pkg, g, arrays)
    layers = [R.Layer(a) for a in arrays]
    assert grid.info().layer_mask == 0b111
    pts = R.border_lattice(g)
    for method in (R.LINEAR, R.CUBIC_CONVOLUTION, R.CUBIC):
        together, used, info = check(grid, g, layers, pts, method, ids=[2, 0, 1])          # a permuted order
        total = np.zeros(5, np.int64)
        for k, layer_id in enumerate([2, 0, 1]):
            v1, m1, i1 = grid.sample(pts, [layer_id], method=method)
            assert v1.tobytes() == together[k:k + 1].tobytes() and m1.tobytes() == used[k:k + 1].tobytes()
            total += np.array([i1.n_outside, *i1.n_method])
        assert total.tolist() == [info.n_outside, *info.n_method]
    for ids in ([0, 0], [1, 2, 1], [3], [0, 16], [-1]):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            grid.sample(pts[:4], ids)
    grid.close()


# ---- 7
@functools.lru_cache(maxsize=None)
def sizes_case():
    g = R.Geometry(12, 9, 0.2)
    a = holes_layer(12, 9, 5)
    rng = np.random.default_rng(3)
    pts = np.c_[rng.uniform(-1.3, 1.3, 257), rng.uniform(-1.0, 1.0, 257)]
    want = {m: R.sample(g, [R.Layer(a)], pts, m) for m in METHODS}
    return g, a, pts, want


@pytest.mark.parametrize("n", [0, 1, 64, 65, 257, 100003])
def test_sizes(pkg, n):
    """the last wave and the last block partial; 100 003 positions repeat the 257 of the shared reference"""
    g, a, pts257, want = sizes_case()
    grid = upload(pkg, g, [a])
    pts = np.tile(pts257, ((n + 256) // 257, 1))[:n]
    for method in METHODS:
        vals, used, info = grid.sample(pts, method=method)
        assert vals.shape == (1, n) and used.shape == (1, n)
        wv, wm, _ = want[method]
        reps = (n + 256) // 257
        wv, wm = np.tile(wv, (1, reps))[:, :n], np.tile(wm, (1, reps))[:, :n]
        same_values(vals, used, wv, wm, ("n", n, "method", method))
        assert info.n_outside == int((wm == R.OUTSIDE).sum()) and list(info.n_method) == [int((wm == m).sum()) for m in range(4)]
    grid.close()


# ---- 8
def test_lifecycle(pkg):
    grid = pkg.Grid()
    assert grid.info().layer_mask == 0 and (grid.info().rows, grid.info().cols) == (0, 0)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # no layers yet
        grid.sample([(0.0, 0.0)])
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        grid.layer(0)
    rng = np.random.default_rng(9)
    memory = []
    for rows, cols, n_layers in ((5, 4, 1), (40, 33, 3), (4, 5, 2)):          # growing, then shrinking
        g = R.Geometry(rows, cols, 0.2, (1.0, 2.0))
        arrays = [rng.uniform(-1, 1, (rows, cols)).astype(f32) for _ in range(n_layers)]
        grid.set_layers(np.stack(arrays), g.res, g.length, g.pos)
        i = grid.info()
        assert (i.rows, i.cols, i.resolution, list(i.length), list(i.position), i.layer_mask) == (rows, cols, 0.2, list(g.length), [1.0, 2.0], (1 << n_layers) - 1)
        for k, a in enumerate(arrays):
            assert grid.layer(k).tobytes() == np.asfortranarray(a).tobytes() and np.array_equal(grid.layer(k), a)
        with pytest.raises(pkg.LioError, match="ERR_ARG"):     # what the object held is replaced: no layer beyond the upload's
            grid.layer(n_layers)
        check(grid, g, [R.Layer(a) for a in arrays], R.border_lattice(g), R.CUBIC)
        memory.append(grid.memory())
    assert memory[0] < memory[1] == memory[2]                  # grows and never shrinks
    # non-finite positions are outside
    nan, inf = np.nan, np.inf
    v, m, info = grid.sample([(nan, 2.0), (1.0, nan), (inf, 2.0), (1.0, -inf), (nan, nan), (1.0, 2.0)], [0, 1], method=R.CUBIC_CONVOLUTION)
    assert (m[:, :5] == R.OUTSIDE).all() and (v[:, :5].view(u32) == R.QNAN_BITS).all() and (m[:, 5] == R.CUBIC_CONVOLUTION).all()
    assert info.n_outside == 10 and list(info.n_method) == [0, 0, 2, 0]
    # a refused upload leaves the object as it was; a short buffer is refused
    lib = pkg.load_library()
    out = np.zeros(19, f32)
    assert lib.lio_grid_get_layer(grid.h, 0, out.ctypes.data, 19) == -1
    v, m, _ = grid.sample([(1.0, 2.0)], want_method=False)
    assert m is None and v.shape == (1, 1)
    grid.close()
    grid.close()


# ---- 9: the store path, on the scene of tests/test_gpu_median_fill.py
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


def same_outputs(a, b, what):
    for k in ("grid", "filled", "fill_mask"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape, (what, k)
    assert (a["layers"] is None) == (b["layers"] is None), what
    for name in (a["layers"] or {}):
        assert a["layers"][name].tobytes() == b["layers"][name].tobytes(), (what, name)
    for k in ("lm_info", "hm_info", "fill_info", "terrain_info", "sdf_info"):
        same_struct(a[k], b[k], (what, k))


def test_store_path(pkg, dense_store):
    st = dense_store
    pose = np.zeros(6, f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(resolution=0.2, fill_holes=0)
    fill = pkg.median_fill_default_config(fill_hole_radius=2.0, num_erode_dilation_iterations=8)
    terrain = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)
    sdf_a, sdf_b = pkg.Sdf(), pkg.Sdf()
    sdf_cfg = pkg.sdf_default_config(nan_policy=1)
    want = st.planning_map(pose, lm, hm, fill, terrain, sdf_a, sdf_cfg)
    grid = pkg.Grid()
    got = st.planning_grid(grid, pose, lm, hm, fill, terrain, sdf_b, sdf_cfg)
    same_outputs(got, want, "with a grid")
    assert sdf_a.nodes().tobytes() == sdf_b.nodes().tobytes()
    info, hm_info = grid.info(), want["hm_info"]
    assert hm_info.rows > 40 and hm_info.cols > 40
    assert (info.rows, info.cols, info.resolution, list(info.length), list(info.position)) == (hm_info.rows, hm_info.cols, 0.2, list(hm_info.length),
                                                                                                list(hm_info.position))
    assert info.layer_mask == (1 << 10) - 1
    assert grid.layer(pkg.GRID_LAYER_ELEVATION).tobytes() == want["grid"].tobytes()
    assert grid.layer(pkg.GRID_LAYER_FILLED).tobytes() == want["filled"].tobytes()
    for k, name in enumerate(pkg.TERRAIN_LAYERS):
        assert grid.layer(pkg.GRID_LAYER_TERRAIN + k).tobytes() == want["layers"][name].tobytes(), name
    # the terrain layers arrive whatever the mask copies to the host
    few = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5, layers=0b10000001)
    got_few = st.planning_grid(grid, pose, lm, hm, fill, few)
    same_outputs(got_few, st.planning_map(pose, lm, hm, fill, few), "two layers to the host")
    assert sorted(got_few["layers"]) == ["smooth", "traversability"] and grid.info().layer_mask == (1 << 10) - 1
    for k, name in enumerate(pkg.TERRAIN_LAYERS):
        assert grid.layer(pkg.GRID_LAYER_TERRAIN + k).tobytes() == want["layers"][name].tobytes(), name
    # sampling traversability and the filled elevation: the restatement on the read-back layers
    trav_id = pkg.GRID_LAYER_TERRAIN + pkg.TERRAIN_LAYERS.index("traversability")
    g = R.Geometry(info.rows, info.cols, info.resolution, tuple(info.position))
    assert g.length == tuple(info.length)
    layers = {trav_id: R.Layer(grid.layer(trav_id)), pkg.GRID_LAYER_FILLED: R.Layer(grid.layer(pkg.GRID_LAYER_FILLED))}
    rng = np.random.default_rng(2)
    half = (0.5 * g.length[0] + 0.3, 0.5 * g.length[1] + 0.3)
    pts = np.c_[rng.uniform(g.pos[0] - half[0], g.pos[0] + half[0], 1000), rng.uniform(g.pos[1] - half[1], g.pos[1] + half[1], 1000)]
    for method in (R.LINEAR, R.CUBIC_CONVOLUTION, R.CUBIC):
        vals, used, sinfo = check(grid, g, layers, pts, method, ids=[trav_id, pkg.GRID_LAYER_FILLED], what="store")
        assert 0 < sinfo.n_outside < 2000
    # without a grid the call is lio_kf_store_planning_map
    none = st.planning_grid(None, pose, lm, hm, fill, terrain, sdf_b, sdf_cfg)
    same_outputs(none, want, "grid_out = NULL")
    # neither fill nor terrain: only the raw grid
    alone = st.planning_grid(grid, pose, lm, hm)
    same_outputs(alone, st.planning_map(pose, lm, hm), "no stage")
    assert grid.info().layer_mask == 1 and grid.layer(0).tobytes() == want["grid"].tobytes()
    only_fill = st.planning_grid(grid, pose, lm, hm, fill, want_grid=False, want_filled=False, want_fill_mask=False)
    assert only_fill["grid"] is None and grid.info().layer_mask == 0b11 and grid.layer(1).tobytes() == want["filled"].tobytes()
    only_terrain = st.planning_grid(grid, pose, lm, hm, None, terrain)
    assert grid.info().layer_mask == ((1 << 10) - 1) & ~0b10
    same_outputs(only_terrain, st.planning_map(pose, lm, hm, None, terrain), "terrain on the raw grid")
    # an empty store leaves the object without layers
    empty = pkg.KeyframeStore()
    e = empty.planning_grid(grid, pose, lm, hm, fill, terrain)
    assert e["grid"].shape == (0, 0) and grid.info().layer_mask == 0
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        grid.sample([(0.0, 0.0)])
    empty.close()
    grid.close(); sdf_a.close(); sdf_b.close()
