"""The planner's occupancy grid on the device against tests/ogm_restate.py (which tests/test_ogm_cpu.py pins): the radius
outlier filter, the draft's chain on a host cloud, and the same chain on the map the store exports.  Every output is an
integer or a byte: every bar is "identical".  DESIGN.md section 4h."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ogm_restate as R                                        # noqa: E402
from test_ogm_cpu import PARAMS, lattice, raster_cloud, uniform_clouds   # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32


def _xyzi(xyz):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=f32)[:, None] * f32(0.5) + f32(1)], axis=1)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def _isolated():
    rng = np.random.default_rng(5)
    slab = rng.uniform([-10, -10, 0], [10, 10, 0.5], (3000, 3))
    r = np.linspace(100.0, 1000.0, 20)
    a = 0.7 * np.arange(20)
    far = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-50, 50, 20)], axis=1)
    return np.concatenate([slab, far]).astype(f32)


def _cell_border(radius):
    """two corner points fix the box at (0, 0, 0) .. (8, 8, 8), so the search grid's edge is the float below; points at exact
    multiples of it from the origin, one float below them, and pairs closer than the radius on either side of such a border"""
    e = f32(f32(radius) * f32(1.001)) + f32(1.0e-5) * f32(8.0)
    pts = [[0, 0, 0], [8, 8, 8]]
    for i in range(1, 12):
        b = f32(e * f32(i))
        lo, hi = f32(b - f32(0.4) * f32(radius)), f32(b + f32(0.4) * f32(radius))
        pts += [[b, b, 0], [np.nextafter(b, f32(0)), b, 0], [lo, 1, 1], [hi, 1, 1], [2, lo, hi], [2, hi, lo]]
    return np.array(pts, f32)


def _filter_cases():
    cases = {}
    for n, pts in uniform_clouds().items():
        for radius, min_nb in PARAMS:
            cases[f"uniform{n}_r{radius}"] = (pts, radius, min_nb)
    cases["lattice_min0"] = (lattice(), 0.5, 0)
    cases["lattice_min1"] = (lattice(), 0.5, 1)
    u = uniform_clouds()[257]
    cases["duplicated"] = (np.repeat(u, 2, axis=0), 1.0, 3)
    cases["isolated"] = (_isolated(), 0.5, 10)
    cases["cell_border_0.5"] = (_cell_border(0.5), 0.5, 1)
    cases["cell_border_0.3"] = (_cell_border(0.3), 0.3, 1)
    cases["below_min_equal"] = (u[:5], 50.0, 5)                # n = min_neighbors: every k_i = 5, nothing stays
    cases["below_min"] = (u[:5], 50.0, 10)
    cases["empty"] = (np.zeros((0, 3), f32), 0.5, 1)
    return cases


FILTER_CASES = _filter_cases()


@pytest.fixture(scope="module")
def filter_refs():
    return {name: R.radius_keep(pts, radius, min_nb) for name, (pts, radius, min_nb) in FILTER_CASES.items()}


@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_filter_is_identical_to_the_restatement_in_both_forms(pkg, filter_refs, name):
    pts, radius, min_nb = FILTER_CASES[name]
    idx, k = filter_refs[name]
    cloud = _xyzi(pts)
    kept, counts = pkg.radius_filter(cloud, radius, min_nb)
    print(f"{name}: n {len(pts)}, kept {len(kept)} (restatement {len(idx)}), counts differ at {int((counts != k).sum())}")
    np.testing.assert_array_equal(counts, k)
    _same_bits(kept, cloud[idx])                               # input order, intensity carried
    early, none = pkg.radius_filter(cloud, radius, min_nb, want_counts=False)
    assert none is None
    _same_bits(early, kept)                                    # the form that stops early keeps the same bytes
    again, counts2 = pkg.radius_filter(cloud, radius, min_nb)
    _same_bits(again, kept)
    np.testing.assert_array_equal(counts2, counts)


def test_isolated_case_takes_the_coarse_cell_path():
    """the box of the isolated case at an edge of the radius would need more than 2^22 cells"""
    pts = _isolated()
    ext = pts.max(axis=0) - pts.min(axis=0)
    assert np.prod(np.floor(ext / 0.5005) + 1) > 2 ** 22
    assert len(R.radius_keep(pts, 0.5, 10)[0]) not in (0, len(pts))


def test_nonfinite_points_take_no_part(pkg):
    rng = np.random.default_rng(9)
    good = rng.uniform([-3, -3, 0], [3, 3, 1], (300, 3)).astype(f32)
    pts = good.copy()
    bad = [7, 100, 200, 250, 299]
    pts[7, 0] = np.nan; pts[100, 1] = np.inf; pts[200, 2] = -np.inf; pts[250, 0] = 2.0e15; pts[299, 2] = -1.5e15
    ok = np.setdiff1d(np.arange(300), bad)
    kept_ref, counts_ref = pkg.radius_filter(_xyzi(pts)[ok], 0.5, 2)          # the same cloud without the bad records
    np.testing.assert_array_equal(counts_ref, R.radius_counts(pts[ok], 0.5))
    kept, counts = pkg.radius_filter(_xyzi(pts), 0.5, 2)
    assert (counts[bad] == -1).all()
    np.testing.assert_array_equal(counts[ok], counts_ref)      # the bad records are nobody's neighbour
    _same_bits(kept, kept_ref)
    _same_bits(pkg.radius_filter(_xyzi(pts), 0.5, 2, want_counts=False)[0], kept_ref)
    only_bad, c = pkg.radius_filter(_xyzi(pts[bad]), 0.5, 0)
    assert len(only_bad) == 0 and (c == -1).all()


def test_refusals_leave_the_filter_usable(pkg):
    pts = uniform_clouds()[257]
    cloud = _xyzi(pts)
    before = pkg.radius_filter(cloud, 1.0, 3)
    for radius, min_nb in ((0.0, 3), (-1.0, 3), (float("nan"), 3), (float("inf"), 3), (1.0, -1)):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            pkg.radius_filter(cloud, radius, min_nb)
    after = pkg.radius_filter(cloud, 1.0, 3)
    _same_bits(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])


# ------------------------------------------------------------------ the chain on a host cloud
def _chain_cloud():
    """the raster cloud, lifted so that the default slice cuts it on both sides"""
    return raster_cloud() * f32([1, 1, 0.25]) + f32([0, 0, 1.2])


def _check_chain(pkg, pts, **kw):
    cfg = pkg.ogm_default_config(**kw)
    ref_grid, ref = R.occupancy_grid(pts, cfg.z_min, cfg.z_max, cfg.z_negative, cfg.remove_outliers, cfg.radius, cfg.min_neighbors,
                                     cfg.resolution, cfg.whole_box)
    grid, info = pkg.occupancy_grid(pts, cfg)
    got = dict(width=info.width, height=info.height, origin=(info.origin[0], info.origin[1]), n_in=info.n_in, n_slice=info.n_slice,
               n_inliers=info.n_inliers, n_binned=info.n_binned, n_occupied=info.n_occupied)
    print(kw, got)
    assert got == ref
    assert grid.dtype == np.int8 and grid.shape == ref_grid.shape
    np.testing.assert_array_equal(grid, ref_grid)
    # grid == NULL: the same geometry and counts
    none, info2 = pkg.occupancy_grid(pts, cfg, want_grid=False)
    assert none is None and bytes(info2) == bytes(info)
    return grid, info


CHAIN = dict(radius=1.0, min_neighbors=3, resolution=0.25)


@pytest.mark.parametrize("whole_box", [0, 1])
@pytest.mark.parametrize("z_negative", [0, 1])
@pytest.mark.parametrize("remove_outliers", [0, 1])
def test_chain_matches_the_restatement(pkg, whole_box, z_negative, remove_outliers):
    grid, info = _check_chain(pkg, _chain_cloud(), whole_box=whole_box, z_negative=z_negative, remove_outliers=remove_outliers,
                              z_min=0.6, z_max=1.9, **CHAIN)
    assert 0 < info.n_slice < info.n_in and info.n_occupied > 0
    assert (info.n_inliers < info.n_slice) == bool(remove_outliers)
    if not whole_box:
        assert not grid[-1].any()                              # OG:181


def test_chain_with_the_drafts_defaults(pkg):
    rng = np.random.default_rng(17)
    pts = rng.uniform([-2, -2, -0.5], [2, 2, 2.5], (4000, 3)).astype(f32)
    grid, info = _check_chain(pkg, pts)
    assert (info.width, info.height) == (79, 79) and 0 < info.n_inliers < info.n_slice


@pytest.mark.parametrize("whole_box", [0, 1])
@pytest.mark.parametrize("last", [(9.0, -8.5), (-6.1, -6.2), (40.0, 40.0)])
def test_chain_when_the_last_point_is_the_extreme(pkg, whole_box, last):
    """more than a cell outside the box, and less than a cell below its minimum (column / row 0 as written)"""
    pts = _chain_cloud()
    lo = pts[:-4, :2].min(axis=0)
    pts[-1, :2] = last if last[0] > -6 else lo - f32([0.1, 0.2])
    pts[-1, 2] = 1.0
    # company two cells nearer the middle, so that the filter keeps the last point and the box still ends short of it
    inward = -np.sign(pts[-1, :2])
    for k, d in enumerate(([0.5, 0.5], [0.6, 0.45], [0.45, 0.6])):
        pts[-2 - k] = [pts[-1, 0] + inward[0] * d[0], pts[-1, 1] + inward[1] * d[1], 1.0 + 0.05 * k]
    for remove_outliers in (0, 1):
        _check_chain(pkg, pts, whole_box=whole_box, remove_outliers=remove_outliers, z_min=0.6, z_max=1.9, **CHAIN)
    sl = pts[R.slice_z(pts, 0.6, 1.9)]
    assert np.array_equal(sl[R.radius_keep(sl, 1.0, 3)[0]][-1], pts[-1])


def test_chain_degenerate_clouds(pkg):
    one = np.array([[1.5, -2.5, 1.0]], f32)
    grid, info = _check_chain(pkg, one, remove_outliers=0)
    assert (info.width, info.height, info.origin[0], info.origin[1], info.n_inliers) == (0, 0, 1.5, -2.5, 1)
    line = np.array([[1, 0, 1], [1, 2, 1], [1, 1, 1]], f32)    # no extent along x
    grid, info = _check_chain(pkg, line, remove_outliers=0, resolution=0.25)
    assert (info.width, info.height, info.n_binned) == (0, 8, 0)
    _check_chain(pkg, one, remove_outliers=1)                  # the filter removes the only point
    _check_chain(pkg, np.array([[0, 0, 5.0], [np.nan, 0, 1]], f32))   # the slice leaves nothing
    assert pkg.occupancy_grid(np.zeros((0, 3), f32))[1].n_in == 0


def test_chain_grid_cap_and_null_grid(pkg):
    pts = _chain_cloud()
    cfg = pkg.ogm_default_config(z_min=0.6, z_max=1.9, **CHAIN)
    ref_grid, ref = R.occupancy_grid(pts, 0.6, 1.9, 0, 1, 1.0, 3, 0.25, 0)
    lib = pkg.load_library()
    p = np.ascontiguousarray(pts)
    info = pkg.OgmInfo()
    cells = ref["width"] * ref["height"]
    small = np.full(cells - 1, 7, np.int8)
    rc = lib.lio_occupancy_grid(0, p.ctypes.data, len(p), 12, C.byref(cfg), small.ctypes.data, small.size, C.byref(info))
    assert rc == -1 and (info.width, info.height) == (ref["width"], ref["height"])
    assert (info.origin[0], info.origin[1]) == ref["origin"] and (small == 7).all()
    exact = np.full(cells + 3, 7, np.int8)
    rc = lib.lio_occupancy_grid(0, p.ctypes.data, len(p), 12, C.byref(cfg), exact.ctypes.data, cells, C.byref(info))
    assert rc == 0 and (exact[cells:] == 7).all()
    np.testing.assert_array_equal(exact[:cells].reshape(ref_grid.shape), ref_grid)
    rc = lib.lio_occupancy_grid(0, p.ctypes.data, len(p), 12, C.byref(cfg), None, 0, C.byref(info))
    assert rc == 0 and (info.n_binned, info.n_occupied) == (ref["n_binned"], ref["n_occupied"])
    # PointXYZI records give the same grid as packed xyz
    rec = np.zeros((len(p), 8), f32)
    rec[:, :3] = p
    rec[:, 4] = 3.0
    again = np.zeros(cells, np.int8)
    assert lib.lio_occupancy_grid(0, rec.ctypes.data, len(rec), 32, C.byref(cfg), again.ctypes.data, cells, C.byref(info)) == 0
    np.testing.assert_array_equal(again, exact[:cells])


# ------------------------------------------------------------------ from the store
@pytest.fixture(scope="module")
def six_keyframes():
    rng = np.random.default_rng(23)
    clouds, poses = [], []
    for k in range(6):
        n = 500 + 37 * k
        xyz = rng.uniform([-8, -8, -1.0], [8, 8, 2.5], (n, 3))
        clouds.append(np.concatenate([xyz, rng.uniform(0, 100, (n, 1))], axis=1).astype(f32))
        poses.append([0.01 * k, -0.02 * k, 0.3 * k, 3.0 * k, 1.5 * k, 0.05 * k])
    return clouds, np.array(poses, f32)


def _store(pkg, clouds, poses):
    st = pkg.KeyframeStore()
    for c in clouds:
        st.add(c)
    if len(clouds):
        st.set_poses(0, poses[:len(clouds)], np.zeros(len(clouds)))
    return st


@pytest.mark.parametrize("resolution", [0.0, 0.4])
def test_store_grid_is_the_chain_on_the_exported_map(pkg, six_keyframes, resolution):
    clouds, poses = six_keyframes
    st = _store(pkg, clouds, poses)
    try:
        cfg = pkg.ogm_default_config(radius=0.8, min_neighbors=2, resolution=0.25)
        full, ds, counts = st.export_map(resolution)
        gm = st.global_map()
        cloud = full if resolution == 0.0 else ds
        assert len(cloud) > 1000
        ref_grid, ref_info = pkg.occupancy_grid(cloud[:, :3], cfg)
        grid, info, n_map = st.occupancy_grid(resolution, cfg)
        print(resolution, n_map, info.width, info.height, info.n_slice, info.n_inliers, info.n_binned, info.n_occupied)
        assert n_map == len(cloud) and info.n_occupied > 0 and 0 < info.n_inliers < info.n_slice < info.n_in
        assert bytes(info) == bytes(ref_info)
        np.testing.assert_array_equal(grid, ref_grid)
        # and the restatement on the same cloud, so that the two device paths are not merely equal to each other
        r_grid, r = R.occupancy_grid(cloud[:, :3], radius=0.8, min_neighbors=2, resolution=0.25)
        np.testing.assert_array_equal(grid, r_grid)
        assert (info.n_slice, info.n_inliers, info.n_binned, info.n_occupied) == (r["n_slice"], r["n_inliers"], r["n_binned"], r["n_occupied"])
        # the store is left as found: the export and the global map return the bytes they returned before
        full2, ds2, counts2 = st.export_map(resolution)
        _same_bits(full2, full)
        if resolution != 0.0:
            _same_bits(ds2, ds)
        assert counts2 == counts
        gm2 = st.global_map()
        _same_bits(gm2[0], gm[0])
        assert gm2[1].tolist() == gm[1].tolist()
        again, info_again, _ = st.occupancy_grid(resolution, cfg)
        np.testing.assert_array_equal(again, grid)
        assert bytes(info_again) == bytes(info)
    finally:
        st.close()


def test_store_empty_and_unposed(pkg, six_keyframes):
    clouds, poses = six_keyframes
    st = pkg.KeyframeStore()
    try:
        grid, info, n_map = st.occupancy_grid(0.0)
        assert (info.width, info.height, info.n_in, n_map) == (0, 0, 0, 0) and grid.size == 0
    finally:
        st.close()
    st = _store(pkg, clouds[:3], poses)
    st.add(clouds[3])                                          # a keyframe without a pose
    try:
        with pytest.raises(pkg.LioError, match="no pose"):
            st.occupancy_grid(0.0)
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.occupancy_grid(-1.0)
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.occupancy_grid(0.0, pkg.ogm_default_config(whole_box=3))
    finally:
        st.close()
