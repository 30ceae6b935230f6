"""numpy restatement of the planning height map (include/liogpu.h lio_height_map) behind the outlier and voxel filters:
stages 3-7 of DESIGN.md section 4e -- level / ego filter / un-level, geometry, binning, elevation (ordered mean or
clusters), hole filling -- written from the semantics stated there, fp32 wherever the reference is fp32 and fp64 wherever it
is fp64.  The outlier filter comes from tests/localmap_restate.py.  The checker of tests/test_heightmap_cpu.py,
tests/test_gpu_heightmap.py and, on the designed inputs of tests/heightmap_cases.py, tests/test_gpu_heightmap_edges.py.  Parity with PCL, Eigen and grid_map themselves is unpinned: none of them can be built here."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_restate as L   # noqa: E402

f32 = np.float32
DEFAULTS = dict(roll=0.0, pitch=0.0, level_and_ego_filter=1, remove_outliers=1, mean_k=10, stddev_mul=1.0, downsample=0,
                voxel=(0.1, 0.1, 0.1), resolution=0.2, min_points_per_cell=1, max_points_per_cell=1000000000, use_cluster=0,
                cluster_tolerance=1.0, cluster_min_points=1, cluster_max_points=1000000000, use_max_height=0, fill_holes=0)
MAX_COORD = f32(1.0e15)


# ---- stage 3 ----------------------------------------------------------------------------------------------------------------
def axis_rotation(angle, axis):
    """Eigen::AngleAxisf(angle, unit axis).toRotationMatrix(), term by term in fp32; sinf / cosf as correctly rounded values."""
    angle = f32(angle)
    s, c = f32(math.sin(float(angle))), f32(math.cos(float(angle)))
    ax = np.zeros(3, f32)
    ax[axis] = 1
    sa, ca = s * ax, (f32(1) - c) * ax
    R = np.zeros((3, 3), f32)
    t = ca[0] * ax[1]
    R[0, 1], R[1, 0] = t - sa[2], t + sa[2]
    t = ca[0] * ax[2]
    R[0, 2], R[2, 0] = t + sa[1], t - sa[1]
    t = ca[1] * ax[2]
    R[1, 2], R[2, 1] = t - sa[0], t + sa[0]
    for k in range(3):
        R[k, k] = ca[k] * ax[k] + c
    return R


def mul3(A, B):
    """3 x 3 product in fp32, every entry (a0 b0 + a1 b1) + a2 b2"""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    C = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            C[i, j] = f32(f32(A[i, 0] * B[0, j]) + f32(A[i, 1] * B[1, j])) + f32(A[i, 2] * B[2, j])
    return C


def rigid(rx, ry):
    """getRigidBodyTransform's linear part: ((I Rx) Ry) Rz(0), then rotate() on the identity"""
    I = np.eye(3, dtype=f32)
    M = mul3(mul3(mul3(I, axis_rotation(rx, 0)), axis_rotation(ry, 1)), axis_rotation(0.0, 2))
    return mul3(I, M)


def rotations(roll, pitch):
    """R1 = Rx(-roll) Ry(-pitch), R2 = Rx(roll) Ry(pitch); R2 is not R1's inverse"""
    roll, pitch = f32(roll), f32(pitch)
    return rigid(-roll, -pitch), rigid(roll, pitch)


def apply(R, p):
    """pcl::transformPointCloud without translation: (m0 x + m1 y) + m2 z per row, fp32, no contraction"""
    p = np.asarray(p, f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z for i in range(3)], 1).astype(f32)


def finite_mask(p):
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(p, f32)[:, :3]) <= MAX_COORD).all(1)


def ego_keep(lev):
    """PointcloudProcessor.cpp:39-55 on levelled points"""
    ax, ay, z = np.abs(lev[:, 0]), np.abs(lev[:, 1]), lev[:, 2]
    near = (ax < f32(20.0)) & (ay < f32(30.0))
    inner = (ax < f32(2.5)) & (ay < f32(5.0))
    return np.where(near, np.where(inner, z < f32(1.0), z < f32(2.0)), True)


def level_ego(pts, roll, pitch, level=1):
    """-> (points the grid is laid around [m, 3] in input order, keep bool [n])"""
    p = np.asarray(pts, f32)[:, :3]
    fin = finite_mask(p)
    if not level:
        return p[fin].copy(), fin
    R1, R2 = rotations(roll, pitch)
    with np.errstate(all="ignore"):
        lev = apply(R1, p)
        keep = fin & ego_keep(lev)
    return apply(R2, lev[keep]), keep


# ---- stage 4 ----------------------------------------------------------------------------------------------------------------
def c_round(x):
    """round(): halves away from zero (x >= 0 here)"""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def geometry(pts, resolution):
    """-> dict(rows, cols, length (2,), position (2,)): GridMapPclLoader.cpp:97-108 + GridMap::setGeometry"""
    p = np.asarray(pts, f32)
    mn, mx = p[:, :2].min(0), p[:, :2].max(0)
    res = float(resolution)
    size = [c_round(float(f32(mx[a] - mn[a])) / res) for a in range(2)]
    return dict(rows=size[0], cols=size[1], length=np.array([size[0] * res, size[1] * res]),
                position=np.array([float(f32(mx[a] + mn[a])) / 2.0 for a in range(2)]), resolution=res)


# ---- stage 5 ----------------------------------------------------------------------------------------------------------------
def bin_cells(pts, g):
    """-> (row, col, inside): index = (int)(-((p - 0.5 length_) - position_) / resolution) in fp64, truncating toward zero;
    a point whose index is negative or equals the size is outside"""
    p = np.asarray(pts, f32)[:, :2].astype(np.float64)
    a = -(((p - 0.5 * g["length"]) - g["position"]) / g["resolution"])
    size = np.array([g["rows"], g["cols"]], np.float64)
    inside = ((a > -1.0) & (a < size)).all(1)
    idx = np.trunc(np.where(inside[:, None], a, 0.0)).astype(np.int64)
    return idx[:, 0], idx[:, 1], inside


# ---- stage 6 ----------------------------------------------------------------------------------------------------------------
def ordered_mean(z):
    """(float)(sum of (double) z in the given order / count)"""
    z = np.asarray(z, f32).astype(np.float64)
    return f32(np.cumsum(z)[-1] / float(len(z)))


def components(pts, tol):
    """Connected components under fp32 squared distance ((dx dx) + dy dy) + dz dz <= (float)((double)tol * tol): -> the label
    of every point = the smallest index of its component.  Flood fill from every unlabelled point in index order."""
    p = np.asarray(pts, f32)[:, :3]
    n = len(p)
    tol2 = f32(float(f32(tol)) * float(f32(tol)))
    lab = np.full(n, -1, np.int64)
    for seed in range(n):
        if lab[seed] >= 0:
            continue
        lab[seed] = seed
        stack = [seed]
        while stack:
            i = stack.pop()
            d = p[i] - p
            d2 = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            new = np.nonzero((d2 <= tol2) & (lab < 0))[0]
            lab[new] = seed
            stack.extend(new.tolist())
    return lab


def cell_height(pts, cfg):
    """The elevation of one cell from its points in input order (NaN: none)"""
    m = len(pts)
    if m == 0 or m < cfg["min_points_per_cell"] or m > cfg["max_points_per_cell"]:
        return f32(np.nan)
    if not cfg["use_cluster"]:
        return ordered_mean(pts[:, 2])
    lab = components(pts, cfg["cluster_tolerance"])
    best = None
    for r in np.unique(lab):                                   # ascending first member: the order of the clusters
        z = pts[lab == r, 2]
        if len(z) < cfg["cluster_min_points"] or len(z) > cfg["cluster_max_points"]:
            continue
        h = ordered_mean(z)
        if best is None or (h > best if cfg["use_max_height"] else h < best):      # the first of equal heights stays
            best = h
    return f32(np.nan) if best is None else best


def elevation(pts, g, cfg):
    """-> (layer [rows, cols] float32, points binned)"""
    p = np.asarray(pts, f32)[:, :3]
    layer = np.full((g["rows"], g["cols"]), np.nan, f32)
    r, c, inside = bin_cells(p, g)
    key = (r + c * g["rows"])[inside]
    q = p[inside]
    order = np.argsort(key, kind="stable")
    key, q = key[order], q[order]
    heads = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0] if len(key) else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], len(key)]
    for b, e in zip(heads, ends):
        layer[key[b] % g["rows"], key[b] // g["rows"]] = cell_height(q[b:e], cfg)
    return layer, int(inside.sum())


# ---- stage 7 ----------------------------------------------------------------------------------------------------------------
def fill_cell(layer, row, col):
    """The value the labelled extension gives NaN cell (row, col), or None: the four nearest valid cells of rows
    [row - 5, row + 5) x cols [col - 5, col + 5), rows outermost, by the strict-< insertion cascade; their fp64 mean"""
    rows, cols = layer.shape
    d = [math.inf] * 4
    v = [0.0] * 4
    for i in range(max(row - 5, 0), min(row + 5, rows)):
        for j in range(max(col - 5, 0), min(col + 5, cols)):
            x = layer[i, j]
            if np.isnan(x):
                continue
            dist = math.sqrt(float((i - row) * (i - row) + (j - col) * (j - col)))
            for k in range(4):
                if dist < d[k]:
                    d[k + 1:] = d[k:3]
                    v[k + 1:] = v[k:3]
                    d[k], v[k] = dist, float(x)
                    break
    if d[3] == math.inf:
        return None
    return f32((((v[0] + v[1]) + v[2]) + v[3]) / 4.0)


def fill(layer):
    """-> (layer after the pass, cells filled): reads `layer`, writes a copy"""
    out = layer.copy()
    n = 0
    for row, col in zip(*np.nonzero(np.isnan(layer))):
        h = fill_cell(layer, int(row), int(col))
        if h is not None:
            out[row, col] = h
            n += 1
    return out, n


# ---- the chain --------------------------------------------------------------------------------------------------------------
def height_map(pts, **overrides):
    """-> dict(grid [rows, cols], rows, cols, length, position, n_in, n_inliers, n_filtered, n_binned, n_valid_cells,
    n_filled_cells, kept (the points after stage 3)).  downsample is not restated (K7 has its own tests)."""
    cfg = dict(DEFAULTS, **overrides)
    assert not cfg["downsample"]
    p = np.asarray(pts, f32)
    p = (p if p.ndim == 2 else p.reshape(-1, 3))[:, :3]
    out = dict(n_in=len(p), rows=0, cols=0, length=np.zeros(2), position=np.zeros(2), n_binned=0, n_valid_cells=0, n_filled_cells=0,
               grid=np.zeros((0, 0), f32))
    if cfg["remove_outliers"] and len(p):
        p = p[L.sor(p, cfg["mean_k"], cfg["stddev_mul"])["keep"]]
    out["n_inliers"] = len(p)
    kept, _ = level_ego(p, cfg["roll"], cfg["pitch"], cfg["level_and_ego_filter"]) if len(p) else (p, None)
    out["kept"], out["n_filtered"] = kept, len(kept)
    if len(kept) == 0:
        return out
    g = geometry(kept, cfg["resolution"])
    out.update(rows=g["rows"], cols=g["cols"], length=g["length"], position=g["position"])
    if g["rows"] == 0 or g["cols"] == 0:
        out["grid"] = np.zeros((g["rows"], g["cols"]), f32)
        return out
    layer, out["n_binned"] = elevation(kept, g, cfg)
    out["n_valid_cells"] = int((~np.isnan(layer)).sum())
    if cfg["fill_holes"]:
        layer, out["n_filled_cells"] = fill(layer)
    out["grid"] = layer
    return out
