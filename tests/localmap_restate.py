"""numpy restatement of publishLocalMap's stages behind the keyframe sum (MO:2474-2540) as include/liogpu.h states them:
the vehicle-frame transform and the two pcl::PassThrough filters, and pcl::StatisticalOutlierRemoval<PointXYZI>::applyFilter
(PCL 1.10, not negative, not organised).  The checker of tests/test_localmap_cpu.py and tests/test_gpu_localmap.py.
Brute-force fp32 distances in chunks, the conventions of DESIGN.md section 4d line by line (parity unpinned).
Also the filter's search restated for tests/sor_cases.py: sor_grid (the grid the hook lio_sor_debug_grid arbitrates), walk (the
shell walk of sor_nearest in np.float32, with the real exit rule and three wrong ones) and knn_d2_fast (the exact k-NN for the
one large case, under a condition it checks)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_restate import transform_points, grid_of, grid_cells, MAX_COORD   # noqa: E402

DEFAULTS = dict(n_keyframes=30, front=70.0, left=40.0, back=20.0, right=40.0, remove_outliers=1, mean_k=10, stddev_mul=1.0,
                downsample=1, leaf=np.float32(0.01))
MAX_MEAN_K = 32


def finite_mask(pts):
    """The points that take part in the filter (include/liogpu.h lio_sor_filter): every coordinate finite
    and within float32(1e15) in magnitude, the bound of the cell sort."""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(pts, np.float32)[:, :3]) <= MAX_COORD).all(1)


def crop_finite_mask(pts):
    """The crop's own rule (LmCropPred): every coordinate finite, |v| <= FLT_MAX -- whatever its size."""
    return np.isfinite(np.asarray(pts, np.float32)[:, :3]).all(1)


def knn_d2(pts, k, chunk=256):
    """The k smallest fp32 squared distances ((dx*dx)+dy*dy)+dz*dz (FLANN L2_Simple) from every point to all points of the
    cloud, itself included, ascending.  pts: finite [n, 3] with n >= k.  -> float32 [n, k].  A function of the multiset."""
    p = np.asarray(pts, np.float32)[:, :3]
    out = np.empty((len(p), k), np.float32)
    for a in range(0, len(p), chunk):
        q = p[a:a + chunk]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        if k < d2.shape[1]:
            d2 = np.partition(d2, k - 1, axis=1)[:, :k]
        out[a:a + chunk] = np.sort(d2, axis=1)
    return out


def knn_d2_fast(pts, k, extra=8):
    """knn_d2 for a large cloud, exact under a condition that is asserted: the candidates are the k + extra nearest of scipy's
    cKDTree in fp64, their d2 is formed in fp32 as knn_d2 forms it, the k smallest are kept.  A point outside the candidates is
    at least as far, in exact arithmetic, as the (k + extra)-th; its fp32 d2 is within 3 * 2^-24 relative of the exact one, so it
    cannot undercut the k-th fp32 distance when the (k + extra)-th fp64 distance exceeds that by more than 1e-5 relative.
    Raises ValueError where that does not hold for some point."""
    from scipy.spatial import cKDTree
    p = np.asarray(pts, np.float32)[:, :3]
    m = min(k + extra, len(p))
    p64 = p.astype(np.float64)
    dist, idx = cKDTree(p64).query(p64, k=m)
    c = p[idx]                                                           # [n, m, 3]
    dx, dy, dz = p[:, None, 0] - c[:, :, 0], p[:, None, 1] - c[:, :, 1], p[:, None, 2] - c[:, :, 2]
    d2 = np.sort(((dx * dx) + dy * dy) + dz * dz, axis=1)[:, :k]
    if m < len(p):
        kth = np.sqrt(d2[:, k - 1].astype(np.float64))
        bad = ~(dist[:, m - 1] > kth * (1.0 + 1e-5))
        if bad.any():
            raise ValueError(f"knn_d2_fast: {int(bad.sum())} points whose candidates do not separate (first {int(np.nonzero(bad)[0][0])})")
    return d2


def mean_distances(pts, mean_k, knn=knn_d2):
    """dist_i = (float)(sum_{k=1..mean_k} (double)sqrtf(d2_k) / mean_k): the smallest of the mean_k + 1 dropped (the point
    itself, or a duplicate at distance 0), the sum in fp64 in ascending order of d2."""
    d2 = knn(pts, mean_k + 1)
    root = np.sqrt(d2[:, 1:]).astype(np.float64)            # np.sqrt on float32: correctly rounded
    acc = np.zeros(len(d2), np.float64)
    for j in range(mean_k):
        acc = acc + root[:, j]
    return (acc / np.float64(mean_k)).astype(np.float32)


def sor(pts, mean_k=10, stddev_mul=1.0, knn=knn_d2):
    """-> dict(rc, keep bool [n], mean_dist float32 [n] (NaN: skipped), stats (mean, stddev, threshold), n_finite, var).
    rc 1: at most mean_k participating points, they pass through (mean_dist 0, stats 0, 0, inf).  knn: knn_d2 or knn_d2_fast."""
    if not (1 <= mean_k <= MAX_MEAN_K) or not math.isfinite(stddev_mul):
        raise ValueError("mean_k in [1, 32], stddev_mul finite")
    p = np.asarray(pts, np.float32)
    p = p if p.ndim == 2 else p.reshape(-1, 3)
    fin = finite_mask(p)
    n = int(fin.sum())
    dist = np.full(len(p), np.nan, np.float32)
    if n <= mean_k:
        dist[fin] = 0.0
        return dict(rc=1, keep=fin.copy(), mean_dist=dist, stats=(0.0, 0.0, math.inf), n_finite=n, var=0.0)
    d = mean_distances(p[fin], mean_k, knn)
    dist[fin] = d
    # the threshold: over the points in index order, in fp64; the square in fp32
    s = float(np.cumsum(d.astype(np.float64))[-1])
    sq = float(np.cumsum((d * d).astype(np.float64))[-1])
    mean = s / n
    var = (sq - s * s / n) / (n - 1.0)
    sd = math.sqrt(var) if var >= 0.0 else math.nan
    thr = mean + float(np.float32(stddev_mul)) * sd
    keep = fin.copy()
    keep[fin] = d.astype(np.float64) <= thr
    return dict(rc=0, keep=keep, mean_dist=dist, stats=(mean, sd, thr), n_finite=n, var=var)


def bracket(thr, n):
    """Half-width of the band around the threshold inside which the device's fixed-order sums may decide differently."""
    return 64.0 * n * 2.0 ** -52 * abs(thr)


# ---- the search of k_sor_search, restated: the grid and the shell walk -----------------------------------------------------
def sor_per_cell(mean_k):
    return np.float32(mean_k + 1) / np.float32(3.0)


def sor_grid(pts, mean_k):
    """The grid lio_sor_filter lays over the cloud (icp_restate.grid_of at (mean_k + 1) / 3 points per occupied cell); where an
    axis has no participating coordinate the filter lays one empty cell at the origin.  The hook lio_sor_debug_grid arbitrates."""
    G = grid_of(np.asarray(pts, np.float32)[:, :3], sor_per_cell(mean_k))
    if G is None:
        one = np.float32(1.0)
        G = dict(origin=np.zeros(3, np.float32), edge=one, inv_cell=one, nx=1, ny=1, nz=1, n_cells=1, occupied=-1)
    return G


WALK_RULES = ("real", "no_slack", "one_shell_early", "stop_when_full")


def walk(pts, mean_k, rule="real", only=None):
    """sor_nearest in np.float32, point by point: the cell floor((p - o) * inv_cell) clamped to the grid, Chebyshev shells
    outwards clipped to the grid (r_far), before shell r > 1 the exit test lb = (r - 1) e - slack, lb > 0 and
    lb * lb * 0.99999f >= worst, slack = 1e-3 e + 1e-5 max|q - o|.  The list after a shell is the k smallest of the multiset
    seen so far (an equal distance changes nothing), so each shell is taken at once.  pts: the participating points.
    rule: "real", or a wrong rule that exists so that the CPU tests can show a case bites -- "no_slack" (lb = (r - 1) e),
    "one_shell_early" (r e in place of (r - 1) e) or "stop_when_full" (leave as soon as the list is full).
    only: the indices to walk (default all).  -> (d2 float32 [m, mean_k + 1] ascending, shells walked int [m])."""
    assert rule in WALK_RULES
    f32 = np.float32
    p = np.asarray(pts, f32)[:, :3]
    k = mean_k + 1
    G = sor_grid(p, mean_k)
    o, e, inv = np.asarray(G["origin"], f32), f32(G["edge"]), f32(G["inv_cell"])
    dims = np.array([G["nx"], G["ny"], G["nz"]], np.int64)
    cells = np.clip(grid_cells(G, p), 0, (dims - 1)[None, :].astype(np.float64)).astype(np.int64)
    ids = np.arange(len(p)) if only is None else np.asarray(only, np.int64)
    out = np.full((len(ids), k), np.inf, f32)
    shells = np.zeros(len(ids), np.int64)
    for row, i in enumerate(ids):
        q, c = p[i], cells[i]
        dx, dy, dz = q[0] - p[:, 0], q[1] - p[:, 1], q[2] - p[:, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        cheb = np.abs(cells - c[None, :]).max(1)
        order = np.argsort(cheb, kind="stable")
        cheb_s, d2_s = cheb[order], d2[order]
        r_far = int(max(c.max(), (dims - 1 - c).max()))
        span = max(max(abs(q[0] - o[0]), abs(q[1] - o[1])), abs(q[2] - o[2]))
        slack = f32(1.0e-3) * e + f32(1.0e-5) * span
        if rule == "no_slack":
            slack = f32(0.0)
        lst = np.full(k, np.inf, f32)
        worst, pos, r = f32(np.inf), 0, 0
        while r <= r_far:
            if r > 1:
                lb = f32(r if rule == "one_shell_early" else r - 1) * e - slack
                if lb > 0 and lb * lb * f32(0.99999) >= worst:
                    break
            if rule == "stop_when_full" and r > 0 and worst < np.inf:
                break
            end = int(np.searchsorted(cheb_s, r, side="right"))
            if end > pos:
                lst = np.sort(np.concatenate([lst, d2_s[pos:end]]))[:k]
                worst, pos = lst[k - 1], end
            r += 1
        out[row], shells[row] = lst, r
    return out, shells


def vehicle_frame(pose):
    """M = Translation(-tX, -tY, -tZ) * Rz(-yaw), MO:2474-2488: cosf / sinf of -yaw in fp32 (the correctly rounded values:
    libm's cosf and the rounded fp64 cosine agree but for arguments nobody has named), tX .. in fp32, no contraction."""
    pose = np.asarray(pose, np.float32)
    yaw, x, y, z = pose[2], pose[3], pose[4], pose[5]
    c = np.float32(math.cos(float(-yaw)))
    s = np.float32(math.sin(float(-yaw)))
    tx = np.float32(x * c) - np.float32(y * s)
    ty = np.float32(y * c) + np.float32(x * s)
    M = np.eye(4, dtype=np.float32)
    M[0, :] = [c, -s, 0.0, -tx]
    M[1, :] = [s, c, 0.0, -ty]
    M[2, 3] = -z
    return M


def crop(world_xyzi, pose, front=70.0, left=40.0, back=20.0, right=40.0):
    """pcl::transformPointCloud under vehicle_frame(pose), then PassThrough x in [-left, right], y in [-back, front], limits
    kept.  -> (survivors [m, 4] transformed, intensity carried; keep bool [n])."""
    w = np.asarray(world_xyzi, np.float32)
    moved = transform_points(vehicle_frame(pose), w[:, :3])
    f32 = np.float32
    with np.errstate(invalid="ignore"):
        keep = (crop_finite_mask(w) & (moved[:, 0] >= -f32(left)) & (moved[:, 0] <= f32(right)) &
                (moved[:, 1] >= -f32(back)) & (moved[:, 1] <= f32(front)))
    out = np.concatenate([moved[keep], w[keep, 3:4]], 1)
    return out, keep
