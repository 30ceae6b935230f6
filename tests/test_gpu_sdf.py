"""The signed distance field on the device (lio_sdf_build, lio_sdf_nodes, lio_sdf_query, lio_occupancy_sdf, lio_kf_store_sdf)
through the C ABI against the fp32 restatement of tests/sdf_restate.py, which tests/test_sdf_cpu.py pins against the
brute-force definition: uint32 / uint64 bit patterns, NaN for NaN only.  On the 20 x 30 cases the brute-force definition is
also applied to the device's own result at the reference's 1e-4, so the check does not rest on the restatement alone."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdf_restate as R                                        # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 1e-4                                                     # grid_map_sdf/test's own


def assert_identical(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), (what, "NaN masks differ in", int((nan_g != nan_w).sum()))
    diff = got.view(u)[~nan_g] != want.view(u)[~nan_w]
    assert not diff.any(), (what, "values that differ:", int(diff.sum()), "of", diff.size)


@pytest.fixture(scope="module")
def sdf(pkg):
    s = pkg.Sdf()
    yield s
    s.close()


def terrain(kind, rows, cols, seed=0):
    r, c = np.mgrid[0:rows, 0:cols]
    if kind == "random":
        return np.random.default_rng(100 + seed).uniform(-1.0, 1.0, (rows, cols)).astype(f32)
    if kind == "low":                                          # less than one cell of relief: the minimum of 2 layers
        return np.random.default_rng(200 + seed).uniform(-0.04, 0.04, (rows, cols)).astype(f32)
    if kind == "constant":
        return np.full((rows, cols), 0.5, f32)
    if kind == "steps":                                        # plateaus: many equal offsets, the fp == fq branch
        return (0.4 * ((r // 7 + c // 11) % 3)).astype(f32)
    if kind in ("spike", "pit"):
        e = np.zeros((rows, cols), f32)
        e[rows // 2, cols // 3] = 1.5 if kind == "spike" else -1.5
        return e
    if kind == "ramp_x":
        return (0.05 * r).astype(f32)
    if kind == "ramp_y":
        return (0.03 * c).astype(f32)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, cols, res, band, pos=(0.0, 0.0), nan_fill=False, seed=0):
    elev = terrain(kind, rows, cols, seed)
    if nan_fill:
        elev = with_holes(elev)
    return R.Field(elev, res, (rows * res, cols * res), pos, band[0], band[1], nan_fill=nan_fill)


def with_holes(elev):
    e = elev.copy()
    e[1, 2] = np.nan
    e[-1, 0] = np.inf
    e[e.shape[0] // 2, e.shape[1] // 2] = -np.inf
    return e


def check_field(pkg, sdf, kind, rows, cols, res, band=(None, None), pos=(0.0, 0.0), definition=False, seed=0):
    F = reference(kind, rows, cols, res, band, pos, False, seed)
    elev = terrain(kind, rows, cols, seed)
    nan = float("nan")
    cfg = pkg.sdf_default_config(min_height=nan if band[0] is None else band[0], max_height=nan if band[1] is None else band[1])
    info = sdf.build(elev, res, (rows * res, cols * res), pos, cfg)
    assert (info.rows, info.cols, info.layers, info.n_nan) == (rows, cols, F.layers, 0)
    assert tuple(info.origin) == F.origin and info.resolution == res
    assert (info.layer_min, info.layer_max) == (F.e_min, F.e_max)
    assert (info.n_all_obstacle, info.n_all_free, info.n_mixed) == tuple(F.modes.count(m) for m in (R.ALL_OBSTACLE, R.ALL_FREE, R.MIXED))
    nodes = sdf.nodes()
    assert_identical(nodes, F.nodes, f"{kind} {rows} x {cols} x {F.layers}")
    if definition:
        worst = 0.0
        for z, h in enumerate(F.heights):
            ok, dev = R.is_equal_sdf(nodes[z, :, :, 0].T, R.brute_force_at_height(elev, h, res), TOL)
            assert ok, (kind, z, dev)
            worst = max(worst, dev)
        print(f"  {kind} {rows} x {cols} x {F.layers}: the device's distances within {worst:.2e} of the definition")
    return F, info, nodes


@pytest.mark.parametrize("kind,rows,cols,res", [("low", 2, 2, 0.1), ("random", 3, 4, 0.1), ("random", 64, 64, 0.1), ("random", 33, 65, 0.2),
                                                ("random", 65, 33, 0.2), ("steps", 33, 65, 0.2), ("steps", 65, 33, 0.2)])
def test_shapes(pkg, sdf, kind, rows, cols, res):
    """the minimum (2 x 2 with 2 layers), odd sizes, a full wave and tile, and one row / column past them in both passes"""
    F, info, _ = check_field(pkg, sdf, kind, rows, cols, res, pos=(3.7, -12.3))
    if kind == "low":
        assert info.layers == 2


@pytest.mark.parametrize("kind", ["random", "constant", "steps", "spike", "pit", "ramp_x", "ramp_y"])
def test_terrains_20x30(pkg, sdf, kind):
    F, info, _ = check_field(pkg, sdf, kind, 20, 30, 0.1, definition=True)
    if kind == "constant":                                     # h == e, then a layer above everything
        assert (info.layers, info.n_mixed, info.n_all_free) == (2, 1, 1)


@pytest.mark.parametrize("band,what", [((1.5, 2.0), "above"), ((-2.0, -1.5), "below"), ((-1.5, 1.5), "around")])
def test_bands(pkg, sdf, band, what):
    """a band entirely above and one entirely below the terrain: every layer takes a shortcut branch"""
    F, info, nodes = check_field(pkg, sdf, "random", 20, 30, 0.1, band=band, definition=True)
    if what == "above":
        assert info.n_all_free == info.layers >= 5 and (nodes[..., 0] > 0).all()
    if what == "below":
        assert info.n_all_obstacle == info.layers >= 5 and (nodes[..., 0] < 0).all()
    if what == "around":
        assert info.n_all_obstacle > 0 and info.n_all_free > 0 and info.n_mixed > 0


def test_layer_heights_on_elevation_values(pkg, sdf):
    """steps of 0.4 at res 0.2 from 0: layers 0, 0.2, 0.4 .. lie on the plateaus (height == elevation: the cell is an obstacle)"""
    F, info, nodes = check_field(pkg, sdf, "steps", 20, 30, 0.2, band=(0.0, 1.0), definition=True)
    assert F.heights[0] == 0.0 and F.heights[2] == f32(0.4) and info.layers >= 5
    assert (nodes[0, :, :, 0] <= 0).all()                      # at the terrain's minimum every cell is an obstacle: distance <= 0


@pytest.mark.parametrize("band,lo,hi", [((-1.15, 1.15), 22, 24), ((-2.0, 2.0), 39, 41)])
def test_129x70(pkg, sdf, band, lo, hi):
    """more than one row tile and wave in both passes; about 23 layers, and about 40, which span two slabs of 32"""
    F, info, _ = check_field(pkg, sdf, "random", 129, 70, 0.1, band=band, pos=(-40.0, 25.0))
    assert lo <= info.layers <= hi


@pytest.mark.parametrize("rows,cols", [(600, 3), (3, 600)])
def test_corridors_and_the_workspace_bound(pkg, rows, cols):
    """grids far from square, both ways: the same bits, and the workspace of a fresh object is what the header states,
    24 bytes x cells x slab (8 of intermediate, 16 of lower bounds) -- not a figure that grows with the longer side's square"""
    one = pkg.Sdf()
    F, info, _ = check_field(pkg, one, "random", rows, cols, 0.1, band=(-2.0, 2.0))
    slab = min(32, info.layers)
    field, work = one.memory()
    cells = rows * cols
    assert info.layers > 32 and 24 * cells * slab <= work <= 24 * cells * slab + 4 * 64 + 8 * 64                # (64 elements of pad a buffer)
    assert 20 * cells * info.layers <= field <= 20 * cells * info.layers + 20 * 64
    one.close()


def test_nan_policy(pkg, sdf):
    elev = with_holes(terrain("random", 20, 30))
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        sdf.build(elev, 0.1, (20 * 0.1, 30 * 0.1), (0.0, 0.0))
    assert sdf.info.n_nan == 3 and (sdf.info.rows, sdf.info.cols) == (20, 30)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # the refused build left no field
        sdf.nodes()
    F = reference("random", 20, 30, 0.1, (None, None), (0.0, 0.0), True)
    info = sdf.build(elev, 0.1, (20 * 0.1, 30 * 0.1), (0.0, 0.0), pkg.sdf_default_config(nan_policy=1))
    assert info.n_nan == 3 and info.layers == F.layers and (info.layer_min, info.layer_max) == (F.e_min, F.e_max)
    assert_identical(sdf.nodes(), F.nodes, "nan_policy 1")
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        sdf.build(np.full((4, 5), np.nan, f32), 0.1, (0.4, 0.5), (0.0, 0.0), pkg.sdf_default_config(nan_policy=1))
    with pytest.raises(pkg.LioError, match="ERR_CAPACITY"):    # 600 cells x 60000 layers
        sdf.build(terrain("random", 20, 30), 0.1, (20 * 0.1, 30 * 0.1), (0.0, 0.0), pkg.sdf_default_config(min_height=0.0, max_height=6000.0))
    assert sdf.info.layers == R.num_layers(0.0, 6000.0, 0.1) >= 59999


def check_occupancy(pkg, grid, res, occupied_min=100):
    """grid: [height, width] int8 as the message; the matrix the reference sees is its transpose"""
    got = pkg.occupancy_sdf(grid, res, occupied_min)
    want = R.signed_distance_from_occupancy((grid.astype(np.int32) >= occupied_min).T, res).T
    assert_identical(got, want, f"occupancy {grid.shape}")
    return got


def test_occupancy(pkg):
    res = 0.1
    assert (check_occupancy(pkg, np.zeros((4, 3), np.int8), res) == np.inf).all()
    assert (check_occupancy(pkg, np.full((4, 3), 100, np.int8), res) == -np.inf).all()
    check_occupancy(pkg, (np.array([[0, 1, 1], [0, 0, 1]]).T * 100).astype(np.int8), 1.0)
    one = np.zeros((30, 20), np.int8)
    one[15, 10] = 100
    got = check_occupancy(pkg, one, res)
    ok, dev = R.is_equal_sdf(got.T, R.brute_force_occupancy((one >= 100).T, res), TOL)
    assert ok, dev
    check_occupancy(pkg, (100 - one).astype(np.int8), res)
    check_occupancy(pkg, (np.array([[1, 1, 1], [0, 1, 1], [1, 1, 0]]).T * 100).astype(np.int8), 1.0)         # the "debugcase"
    rnd = np.random.default_rng(7).uniform(-1, 1, (30, 20))
    for h in (-0.9, -0.3, 0.0, 0.4, 0.95):
        got = check_occupancy(pkg, ((rnd > h) * 100).astype(np.int8), 1.0)
        ok, dev = R.is_equal_sdf(got.T, R.brute_force_occupancy((rnd > h).T, 1.0), TOL)
        assert ok, (h, dev)
    corners = np.zeros((33, 65), np.int8)                      # width 65, height 33: one obstacle in each corner
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 100
    check_occupancy(pkg, corners, 0.05)
    check_occupancy(pkg, corners.T.copy(), 0.05)
    values = np.random.default_rng(8).choice(np.array([0, 1, 50, 100, 127, -1], np.int8), (65, 33))
    for occupied_min in (1, 100, 101):
        check_occupancy(pkg, values, 0.25, occupied_min)


def test_query(pkg, sdf):
    """1000 seeded positions: node centres, exact half-cells (res 0.25: the halves are exact in double), far outside on every
    side, and random ones; n = 0; derivative NULL"""
    rows, cols, res, pos = 20, 30, 0.25, (2.0, -1.0)
    F, info, _ = check_field(pkg, sdf, "random", rows, cols, res, band=(-1.0, 1.0), pos=pos)
    rng = np.random.default_rng(12)
    ox, oy, oz = F.origin
    idx = np.c_[rng.integers(0, rows, 300), rng.integers(0, cols, 300), rng.integers(0, F.layers, 300)]
    centres = np.c_[ox - idx[:, 0] * res, oy - idx[:, 1] * res, oz + idx[:, 2] * res]
    halves = centres[:200] + rng.choice([-0.5, 0.5], (200, 3)) * res
    inside = np.c_[rng.uniform(ox - rows * res, ox + res, 300), rng.uniform(oy - cols * res, oy + res, 300), rng.uniform(oz - res, oz + F.layers * res, 300)]
    far = centres[:200].copy()
    side = rng.integers(0, 6, 200)
    side[:6] = np.arange(6)
    for k, s in enumerate(side):
        far[k, s // 2] += (1.0 if s % 2 else -1.0) * rng.uniform(50.0, 1e6)
    p = np.ascontiguousarray(np.r_[centres, halves, inside, far])
    assert len(p) == 1000
    val, der = sdf.query(p)
    want = [F.value_and_derivative(tuple(q)) for q in p]
    assert_identical(val, np.array([w[0] for w in want]), "value")
    assert_identical(der, np.array([w[1] for w in want]), "derivative")
    flat = F.nodes.reshape(-1, 4)
    assert all(F.nearest_node(tuple(q)) == tuple(i) for q, i in zip(centres, idx))
    assert np.array_equal(val[:300], np.array([flat[F.linear_index(tuple(i))][0] for i in idx], np.float64))      # a node centre returns the node
    only, none = sdf.query(p, want_derivative=False)
    assert none is None and only.tobytes() == val.tobytes()
    v0, d0 = sdf.query(np.zeros((0, 3)))
    assert v0.shape == (0,) and d0.shape == (0, 3)
    assert pkg.load_library().lio_sdf_query(sdf.h, None, 0, None, None) == 0


def test_rebuild_into_the_same_object(pkg, sdf):
    """a smaller and then a larger grid into one object: the same bits as a fresh object gives"""
    fresh = {}
    for shape in ((20, 30), (3, 4), (64, 64)):
        one = pkg.Sdf()
        one.build(terrain("random", *shape), 0.1, (shape[0] * 0.1, shape[1] * 0.1), (0.0, 0.0))
        fresh[shape] = one.nodes()
        one.close()
    for shape in ((20, 30), (3, 4), (64, 64), (3, 4)):
        sdf.build(terrain("random", *shape), 0.1, (shape[0] * 0.1, shape[1] * 0.1), (0.0, 0.0))
        assert sdf.nodes().tobytes() == fresh[shape].tobytes(), shape
    lib = pkg.load_library()
    small = np.zeros(4 * 3 * 4 * sdf.info.layers - 1, f32)
    assert lib.lio_sdf_nodes(sdf.h, small.ctypes.data, small.size) == -1


@pytest.fixture(scope="module")
def small_store(pkg):
    rng = np.random.default_rng(37)                            # the store tests/test_gpu_terrain.py builds
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


def test_from_the_store(pkg, sdf, small_store):
    """lio_kf_store_sdf = lio_kf_store_height_map followed by lio_sdf_build on its grid, bit for bit, with the same grid bytes"""
    st = small_store
    pose = np.array([0.02, -0.01, 0.4, 2.0, 0.8, 0.1], f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    hm = pkg.height_map_default_config(roll=0.02, pitch=-0.01, resolution=0.2, fill_holes=1)
    cfg = pkg.sdf_default_config(nan_policy=1, min_height=-0.5, max_height=2.5)
    grid_ref, hm_ref, lm_ref = st.height_map(pose, lm, hm)
    grid, info, hm_info, lm_info = st.sdf_map(sdf, pose, lm, hm, cfg)
    assert info.rows > 10 and (info.rows, info.cols) == (hm_ref.rows, hm_ref.cols) and grid.tobytes() == grid_ref.tobytes()
    assert info.layers == R.num_layers(-0.5, 2.5, 0.2) and info.n_nan == int((~np.isfinite(grid_ref)).sum())
    for name, _ in pkg.HeightMapInfo._fields_:
        a, b = getattr(hm_info, name), getattr(hm_ref, name)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    for name, _ in pkg.LocalMapInfo._fields_:
        assert getattr(lm_info, name) == getattr(lm_ref, name), name
    chained = sdf.nodes()
    direct = pkg.Sdf()
    info_d = direct.build(grid_ref, 0.2, hm_ref.length, hm_ref.position, cfg)
    for name, _ in pkg.SdfInfo._fields_:
        a, b = getattr(info, name), getattr(info_d, name)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
    assert chained.tobytes() == direct.nodes().tobytes()
    p = np.random.default_rng(3).uniform(-8, 8, (50, 3))
    assert sdf.query(p)[0].tobytes() == direct.query(p)[0].tobytes()
    direct.close()
    # without the elevation grid; the height map alone still gives the same bytes
    none, info2, _, _ = st.sdf_map(sdf, pose, lm, hm, cfg, want_grid=False)
    assert none is None and info2.layers == info.layers and sdf.nodes().tobytes() == chained.tobytes()
    again, _, _ = st.height_map(pose, lm, hm)
    assert again.tobytes() == grid_ref.tobytes()
    if info.n_nan:                                             # the grid has holes: refused as it stands, with their count
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.sdf_map(sdf, pose, lm, hm, pkg.sdf_default_config())
        assert sdf.info.n_nan == info.n_nan
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.sdf_map(sdf, pose, lm, hm, pkg.sdf_default_config(min_height=1.0, max_height=0.0))
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.sdf_map(sdf, pose, lm, pkg.height_map_default_config(fill_holes=2), cfg)
    empty = pkg.KeyframeStore()
    g, i, h, m = empty.sdf_map(sdf, pose)
    assert g.shape == (0, 0) and (i.rows, i.cols, i.layers, h.n_in, m.n_summed) == (0, 0, 0, 0, 0)
    empty.close()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):         # an empty local map leaves no field
        sdf.nodes()
