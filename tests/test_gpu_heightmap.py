"""The planning height map on the device (lio_height_map, lio_kf_store_height_map) through the C ABI against the numpy
restatement of tests/heightmap_restate.py, which tests/test_heightmap_cpu.py pins against closed forms.  "Bit-identical"
below means: to that restatement.  Parity with PCL, Eigen and grid_map themselves is unpinned (none can be built here)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_restate as H                                  # noqa: E402
import localmap_restate as L                                   # noqa: E402
from test_localmap_cpu import assert_bracket_empty             # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
PLAIN = dict(remove_outliers=0, level_and_ego_filter=0)        # stages 4-7 alone


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_grid(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), (what, int((nan_g != nan_w).sum()))
    diff = bits(got)[~nan_g] != bits(want)[~nan_w]
    assert not diff.any(), (what, int(diff.sum()))


def check(pkg, pts, what="", **cfg):
    """One call against the restatement: geometry, counts, grid.  -> (grid, info, restatement)"""
    ref = H.height_map(pts, **cfg)
    grid, info = pkg.height_map(pts, pkg.height_map_default_config(**cfg))
    print(f"  {what}: {info.rows} x {info.cols}, in {info.n_in}, inliers {info.n_inliers}, filtered {info.n_filtered}, binned {info.n_binned}, "
          f"valid {info.n_valid_cells}, filled {info.n_filled_cells}; restatement {ref['rows']} x {ref['cols']}, {ref['n_inliers']}, "
          f"{ref['n_filtered']}, {ref['n_binned']}, {ref['n_valid_cells']}, {ref['n_filled_cells']}")
    assert (info.rows, info.cols) == (ref["rows"], ref["cols"]), what
    assert list(info.length) == list(ref["length"]) and list(info.position) == list(ref["position"]), what
    assert (info.n_in, info.n_inliers, info.n_filtered) == (ref["n_in"], ref["n_inliers"], ref["n_filtered"]), what
    assert (info.n_binned, info.n_valid_cells, info.n_filled_cells) == (ref["n_binned"], ref["n_valid_cells"], ref["n_filled_cells"]), what
    assert_same_grid(grid, ref["grid"], what)
    return grid, info, ref


def scene():
    """3 000 points: a tilted ground plane of 12 m x 9 m, a box, and a pole next to the vehicle the ego filter cuts"""
    rng = np.random.default_rng(17)
    g = np.stack([rng.uniform(-6, 6, 2500), rng.uniform(-4.5, 4.5, 2500)], 1)
    ground = np.c_[g, 0.05 * g[:, 0] - 0.03 * g[:, 1] + rng.normal(0, 0.01, 2500)]
    box = np.c_[rng.uniform(3, 4, 350), rng.uniform(1, 2, 350), rng.uniform(0, 1.5, 350)]
    pole = np.c_[rng.normal(1.0, 0.02, 150), rng.normal(1.0, 0.02, 150), rng.uniform(0, 3, 150)]
    return np.concatenate([ground, box, pole]).astype(f32)[rng.permutation(3000)]


def test_default_chain(pkg):
    pts = scene()
    assert_bracket_empty(L.sor(pts, 10, 1.0), "scene")          # no point for which the fixed-order sums could decide differently
    grid, info, ref = check(pkg, pts, "default chain", roll=0.03, pitch=-0.02)
    assert info.rows != info.cols and info.rows > 50 and info.cols > 35 and info.n_in == 3000
    assert info.n_inliers < 3000 and info.n_filtered < info.n_inliers and 0 < info.n_binned <= info.n_filtered
    # the same bytes again, and the voxel filter in front = lio_voxel_grid's output fed in
    again, _ = pkg.height_map(pts, pkg.height_map_default_config(roll=0.03, pitch=-0.02))
    assert again.tobytes() == grid.tobytes()
    vox, vrc = pkg.voxel_grid(np.c_[pts, np.zeros(len(pts), f32)], 0.3)
    assert vrc == 0 and len(vox) < len(pts)
    a, ia = pkg.height_map(pts, pkg.height_map_default_config(remove_outliers=0, downsample=1, voxel=(0.3, 0.3, 0.3), roll=0.03, pitch=-0.02))
    b, ib = pkg.height_map(vox[:, :3], pkg.height_map_default_config(remove_outliers=0, roll=0.03, pitch=-0.02))
    assert (ia.rows, ia.cols, ia.n_filtered, ia.n_binned, ia.voxel_passthrough) == (ib.rows, ib.cols, ib.n_filtered, ib.n_binned, 0)
    assert_same_grid(a, b, "voxel filter in front")


@pytest.mark.parametrize("extent", [(2.125, 1.625), (2.0625, 1.5625), (2.0, 1.5)])
def test_binning_edges(pkg, extent):
    # resolution 0.25: length / resolution = 8.5 and 6.5 (the size rounds up, the grid is longer than the cloud), 8.25 and 6.25
    # (rounds down: the maximum corner has a positive index vector that truncates to 0), 8 and 6 (exact).  A lattice of
    # eighths puts points on cell borders whatever the half-cell shift; both extreme corners are points.
    ex, ey = extent
    xs = np.r_[np.arange(0, ex, 0.375), ex]
    ys = np.r_[np.arange(0, ey, 0.375), ey]
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    rng = np.random.default_rng(3)
    pts = np.c_[X.ravel(), Y.ravel(), rng.uniform(-1, 1, X.size)].astype(f32)
    assert 30 <= len(pts) <= 50 and (pts[0, :2] == 0).all() and (pts[-1, :2] == [ex, ey]).all()
    grid, info, ref = check(pkg, pts, f"edges {extent}", resolution=0.25, **PLAIN)
    assert (info.rows, info.cols) == (H.c_round(ex / 0.25), H.c_round(ey / 0.25)) and info.n_filtered == len(pts)
    # a grid longer than the cloud holds the minimum corner too; otherwise its index equals the size and it is dropped
    assert info.n_binned == len(pts) if ex == 2.125 else info.n_binned < len(pts)
    assert not np.isnan(grid[0, 0])                             # the maximum corner's cell


def test_ordered_sum(pkg):
    # one cell of 2 000 points with z over 1e-6 .. 50 in an order whose fp64 sum differs from the ascending one, and one cell
    # of four points for which the two orders give different floats
    for seed in range(50):
        rng = np.random.default_rng(seed)
        z = (10.0 ** rng.uniform(-6, math.log10(50.0), 2000)).astype(f32)
        in_order, ascending = np.cumsum(z.astype(np.float64))[-1], np.cumsum(np.sort(z).astype(np.float64))[-1]
        if in_order != ascending:
            break
    assert in_order != ascending
    big = np.c_[rng.uniform(1.2, 1.8, 2000), rng.uniform(1.2, 1.8, 2000), z]
    z4 = np.array([2.0 ** 40, 2.0 ** -14, -2.0 ** 40, 2.0 ** -14])
    assert f32(np.cumsum(z4)[-1] / 4.0) == f32(2.0 ** -16) and f32(np.cumsum(np.sort(z4))[-1] / 4.0) == f32(0.0)
    four = np.c_[np.full(4, 0.5), np.full(4, 0.5), z4]
    pts = np.concatenate([[[0, 0, 0]], big[:1000], four[:2], big[1000:], four[2:], [[2, 2, 0]]]).astype(f32)
    grid, info, ref = check(pkg, pts, "ordered sum", resolution=1.0, **PLAIN)
    assert (info.rows, info.cols) == (2, 2)
    assert grid[0, 0] == f32(in_order / 2001.0)                 # (the corner point (2, 2, 0) is this cell's last)
    assert grid[1, 1] == f32(2.0 ** -16)


def ego_candidates(roll, pitch):
    """name -> points whose levelled coordinate steps through one threshold of the ego filter float by float"""
    R1, _ = H.rotations(roll, pitch)
    inv = np.linalg.inv(R1.astype(np.float64))
    groups = {}
    def steps(v):
        out = [f32(v)]
        for _ in range(12):
            out.append(np.nextafter(out[-1], f32(np.inf)))
        lo = [f32(v)]
        for _ in range(12):
            lo.append(np.nextafter(lo[-1], f32(-np.inf)))
        return np.array(lo[:0:-1] + out, f32).astype(np.float64)
    for name, axis, thr, base in (("x2.5", 0, 2.5, (0, 1.0, 1.5)), ("x20", 0, 20.0, (0, 3.0, 2.5)), ("y5", 1, 5.0, (1.0, 0, 1.5)),
                                  ("y30", 1, 30.0, (3.0, 0, 2.5)), ("z1", 2, 1.0, (1.0, 2.0, 0)), ("z2", 2, 2.0, (10.0, 2.0, 0))):
        for sign in ((1, -1) if axis < 2 else (1,)):
            s = steps(thr)
            lev = np.tile(np.array(base, np.float64), (len(s), 1))
            lev[:, axis] = sign * s
            groups[f"{name}{'+' if sign > 0 else '-'}"] = ((inv @ lev.T).T.astype(f32), axis, f32(thr))
    return groups


@pytest.mark.parametrize("angles", [(0.0, 0.0), (0.03, -0.02)])
def test_ego_filter(pkg, angles):
    roll, pitch = angles
    R1, _ = H.rotations(roll, pitch)
    far = np.array([[40.0, 40.0, 0.0], [-40.0, -40.0, 0.0]], f32)         # outside every threshold: they fix the grid
    for name, (cand, axis, thr) in ego_candidates(roll, pitch).items():
        lev = np.abs(H.apply(R1, cand)[:, axis])
        assert (lev < thr).any() and (lev >= thr).any(), name           # the candidates do lie on both sides
        pts = np.concatenate([far, cand])
        kept, keep = H.level_ego(pts, roll, pitch)
        assert 2 < keep.sum() < len(pts), name                           # ... and the filter cuts between them
        grid, info, ref = check(pkg, pts, f"ego {name} {angles}", roll=roll, pitch=pitch, remove_outliers=0, resolution=0.5)
        assert info.n_filtered == int(keep.sum()), name


def layered_cells(rng, rows=10, cols=6, res=0.2):
    """rows x cols cells, each with two or three thin z-layers 0.4 and 1.5 m apart of 1 .. 6 points, shuffled"""
    pts = []
    for r in range(rows):
        for c in range(cols):
            z0 = rng.uniform(-1, 1)
            for k, dz in enumerate((0.0, 0.4, 1.9)):
                if k == 2 and (r + c) % 2:
                    continue
                m = int(rng.integers(1, 7))
                pts.append(np.c_[rng.uniform(r * res + 0.02, (r + 1) * res - 0.02, m), rng.uniform(c * res + 0.02, (c + 1) * res - 0.02, m),
                                 z0 + dz + rng.uniform(-0.02, 0.02, m)])
    pts = np.concatenate(pts)[rng.permutation(sum(len(p) for p in pts))]
    return np.concatenate([[[0, 0, 0]], pts, [[rows * res, cols * res, 0]]]).astype(f32)


@pytest.mark.parametrize("tol", [1.0, 0.3])
@pytest.mark.parametrize("use_max", [0, 1])
def test_clusters(pkg, tol, use_max):
    pts = layered_cells(np.random.default_rng(23))
    grid, info, ref = check(pkg, pts, f"clusters tol {tol} max {use_max}", use_cluster=1, cluster_tolerance=tol, cluster_min_points=3,
                            use_max_height=use_max, **PLAIN)
    assert (info.rows, info.cols) == (10, 6) and 0 < info.n_valid_cells <= 60
    plain, _ = pkg.height_map(pts, pkg.height_map_default_config(**PLAIN))
    assert not np.array_equal(bits(plain), bits(grid))          # clustering changes the layer
    # a cluster size limit from above
    check(pkg, pts, "clusters max 4", use_cluster=1, cluster_tolerance=tol, cluster_min_points=2, cluster_max_points=4, use_max_height=use_max, **PLAIN)


def test_cluster_cell_past_the_lds_tile(pkg):
    rng = np.random.default_rng(29)
    n = 5000
    layer = rng.integers(0, 3, n)
    z = np.array([0.0, 0.4, 1.9])[layer] + rng.uniform(-0.02, 0.02, n)
    big = np.c_[rng.uniform(0.21, 0.39, n), rng.uniform(0.21, 0.39, n), z]
    small = np.c_[rng.uniform(0.01, 0.19, 40), rng.uniform(0.01, 0.19, 40), rng.uniform(0, 0.1, 40)]
    pts = np.concatenate([[[0, 0, 0]], big[:2500], small, big[2500:], [[0.6, 0.6, 0]]]).astype(f32)
    for tol, use_max in ((0.3, 0), (0.3, 1), (1.0, 1)):
        grid, info, ref = check(pkg, pts, f"5000-point cell tol {tol} max {use_max}", use_cluster=1, cluster_tolerance=tol, cluster_min_points=3,
                                use_max_height=use_max, **PLAIN)
        assert (info.rows, info.cols) == (3, 3) and info.n_binned == n + 41


def holes_cloud():
    """One point per valid cell of a 30 x 24 grid at resolution 0.5 -> (points, valid mask)"""
    rng = np.random.default_rng(31)
    valid = rng.uniform(size=(30, 24)) < 0.45
    valid[8:24, 4:20] = False                                   # a hole wider than the window
    valid[15, 11] = valid[16, 12] = valid[14, 12] = True        # ... with three valid cells in its middle
    valid[0, :3] = valid[:3, 0] = False                         # holes at the borders
    valid[29, 20:] = valid[27:, 23] = False
    valid[0, 0] = True                                          # the maximum corner's cell
    r, c = np.nonzero(valid)
    x, y = 15.0 - 0.5 * (r + 0.5), 12.0 - 0.5 * (c + 0.5)       # cell centres: row 0 is at the largest x
    pts = np.c_[x, y, rng.uniform(-2, 2, len(r))]
    return np.concatenate([[[0, 0, 0]], pts, [[15.0, 12.0, 0.5]]]).astype(f32), valid


def test_fill(pkg):
    pts, valid = holes_cloud()
    grid0, info0, ref0 = check(pkg, pts, "fill off", resolution=0.5, **PLAIN)
    assert (info0.rows, info0.cols) == (30, 24) and np.array_equal(~np.isnan(grid0), valid) and info0.n_filled_cells == 0
    grid1, info1, ref1 = check(pkg, pts, "fill on", resolution=0.5, fill_holes=1, **PLAIN)
    assert np.array_equal(bits(grid1[valid]), bits(grid0[valid])) and info1.n_valid_cells == info0.n_valid_cells == int(valid.sum())
    assert 0 < info1.n_filled_cells == int((~np.isnan(grid1)).sum() - valid.sum())
    # a hole with exactly three valid cells in its window stays; ties at equal distance occurred
    three = [(r, c) for r, c in zip(*np.nonzero(~valid)) if valid[max(r - 5, 0):min(r + 5, 30), max(c - 5, 0):min(c + 5, 24)].sum() == 3]
    assert three and all(np.isnan(grid1[r, c]) for r, c in three)
    tied = 0
    for r, c in zip(*np.nonzero(~valid & ~np.isnan(grid1))):
        ii, jj = np.nonzero(valid[max(r - 5, 0):min(r + 5, 30), max(c - 5, 0):min(c + 5, 24)])
        d = np.sort((ii + max(r - 5, 0) - r) ** 2 + (jj + max(c - 5, 0) - c) ** 2)
        tied += int(len(d) > 4 and d[3] == d[4])
    assert tied > 0


@pytest.fixture(scope="module")
def small_store(pkg):
    rng = np.random.default_rng(37)
    st = pkg.KeyframeStore()
    poses = []
    for k in range(6):
        n = 480 + 7 * k
        xy = rng.uniform(-9, 9, (n, 2))
        cloud = np.c_[xy, 0.04 * xy[:, 0] + rng.normal(0, 0.02, n) + (rng.uniform(size=n) < 0.1) * rng.uniform(0, 2.5, n), rng.uniform(0, 255, n)]
        st.add(cloud.astype(f32))
        poses.append([0.01 * k, -0.005 * k, 0.1 * k, 0.5 * k, 0.2 * k, 0.02 * k])
    st.set_poses(0, np.array(poses, f32), times=np.arange(6) * 1.0)
    yield st
    st.close()


def test_from_the_store(pkg, small_store):
    st = small_store
    pose = np.array([0.02, -0.01, 0.4, 2.0, 0.8, 0.1], f32)
    lm = pkg.local_map_default_config(n_keyframes=4, front=8.0, left=6.0, back=5.0, right=6.0)
    cloud, lm_ref, rc = st.local_map(pose, lm)
    assert rc == 0 and lm_ref.n_keyframes == 4 and 500 < lm_ref.n_out < lm_ref.n_summed
    for res in (0.2, 0.35):                                     # the second call: another grid from the same store (stale buffers)
        cfg = pkg.height_map_default_config(roll=0.02, pitch=-0.01, resolution=res, fill_holes=1)
        grid, info, lm_info = st.height_map(pose, lm, cfg)
        direct, info_d = pkg.height_map(cloud[:, :3], cfg)
        for name, _ in pkg.LocalMapInfo._fields_:
            assert getattr(lm_info, name) == getattr(lm_ref, name), name
        for name, _ in pkg.HeightMapInfo._fields_:
            a, b = getattr(info, name), getattr(info_d, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name
        assert info.rows > 10 and info.n_in == lm_ref.n_out and info.n_filled_cells > 0
        assert_same_grid(grid, direct, f"store, resolution {res}")
    # the store still gives the same local map; an empty store gives an empty grid
    again, _, _ = st.local_map(pose, lm)
    assert np.array_equal(bits(again), bits(cloud))
    empty = pkg.KeyframeStore()
    grid, info, lm_info = empty.height_map(pose)
    assert grid.shape == (0, 0) and (info.rows, info.cols, info.n_in, lm_info.n_summed) == (0, 0, 0, 0)
    empty.close()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.height_map(pose, pkg.local_map_default_config(n_keyframes=0))


def test_arguments_and_edges(pkg):
    lib = pkg.load_library()
    pts = scene()[:600]
    cfg = pkg.height_map_default_config(**PLAIN)
    ref = H.height_map(pts, **PLAIN)
    info = pkg.HeightMapInfo()
    call = lambda p, grid, cap, c=cfg: lib.lio_height_map(0, p.ctypes.data, len(p), 12, C.byref(c), grid, cap, C.byref(info))
    # grid == NULL: the geometry only; a grid one cell too small: refused with the size; then room
    assert call(pts, None, 0) == 0 and (info.rows, info.cols) == (ref["rows"], ref["cols"]) and info.n_filtered == 600
    n_cells = info.rows * info.cols
    buf = np.full(n_cells, 7.0, f32)
    info.rows = info.cols = -1
    assert call(pts, buf.ctypes.data, n_cells - 1) == -1 and (info.rows, info.cols) == (ref["rows"], ref["cols"]) and (buf == 7.0).all()
    assert call(pts, buf.ctypes.data, n_cells) == 0
    assert_same_grid(buf.reshape(info.cols, info.rows).T, ref["grid"], "column-major")
    # an empty cloud, a single point, a vertical line, a line along x: no grid, no error
    for p, want in ((np.zeros((0, 3), f32), (0, 0)), (np.array([[1, 2, 3]], f32), (0, 0)), (np.array([[1, 2, 0], [1, 2, 5], [1, 2, 9]], f32), (0, 0)),
                    (np.array([[0, 2, 0], [1, 2, 5]], f32), (5, 0))):
        grid, inf = pkg.height_map(p, cfg)
        assert (inf.rows, inf.cols) == want and grid.size == 0 and inf.n_in == len(p)
    # a NaN / inf coordinate: dropped, the others as without it
    bad = np.concatenate([pts[:100], [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], pts[100:]]).astype(f32)
    for kw in (PLAIN, dict(roll=0.03, pitch=-0.02)):
        c = pkg.height_map_default_config(**kw)
        g_bad, i_bad = pkg.height_map(bad, c)
        g_ok, i_ok = pkg.height_map(pts, c)
        assert (i_bad.n_in, i_bad.n_filtered, i_bad.n_binned, i_bad.rows, i_bad.cols) == (603, i_ok.n_filtered, i_ok.n_binned, i_ok.rows, i_ok.cols)
        assert_same_grid(g_bad, g_ok, "non-finite")
    # refused, never clamped
    for kw in (dict(resolution=5e-5), dict(resolution=float("nan")), dict(roll=float("nan")), dict(pitch=float("inf")), dict(mean_k=0), dict(mean_k=33),
               dict(stddev_mul=float("nan")), dict(level_and_ego_filter=2), dict(remove_outliers=-1), dict(downsample=2), dict(use_cluster=2),
               dict(use_max_height=3), dict(fill_holes=2), dict(downsample=1, voxel=(0.1, 0.1, 0.2)), dict(downsample=1, voxel=(0.0, 0.0, 0.0)),
               dict(min_points_per_cell=-1), dict(use_cluster=1, cluster_tolerance=float("nan"))):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            pkg.height_map(pts, pkg.height_map_default_config(**kw))
    assert lib.lio_height_map(0, pts.ctypes.data, len(pts), 12, None, None, 0, C.byref(info)) == -1
    assert lib.lio_height_map(0, pts.ctypes.data, len(pts), 10, C.byref(cfg), None, 0, C.byref(info)) == -1
    # min / max points per cell, and the library still answers
    check(pkg, pts, "min 2 points", min_points_per_cell=2, resolution=0.5, **PLAIN)
    check(pkg, pts, "max 3 points", max_points_per_cell=3, resolution=0.5, **PLAIN)
    check(pkg, pts, "after the refusals", **PLAIN)
