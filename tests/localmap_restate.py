"""numpy restatement of publishLocalMap's stages behind the keyframe sum (MO:2474-2540) as include/liogpu.h states them:
the vehicle-frame transform and the two pcl::PassThrough filters, and pcl::StatisticalOutlierRemoval<PointXYZI>::applyFilter
(PCL 1.10, not negative, not organised).  The checker of tests/test_localmap_cpu.py and tests/test_gpu_localmap.py.
Brute-force fp32 distances in chunks, the conventions of DESIGN.md section 4d line by line (parity unpinned)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_restate import transform_points   # noqa: E402

DEFAULTS = dict(n_keyframes=30, front=70.0, left=40.0, back=20.0, right=40.0, remove_outliers=1, mean_k=10, stddev_mul=1.0,
                downsample=1, leaf=np.float32(0.01))
MAX_MEAN_K = 32


def finite_mask(pts):
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


def mean_distances(pts, mean_k):
    """dist_i = (float)(sum_{k=1..mean_k} (double)sqrtf(d2_k) / mean_k): the smallest of the mean_k + 1 dropped (the point
    itself, or a duplicate at distance 0), the sum in fp64 in ascending order of d2."""
    d2 = knn_d2(pts, mean_k + 1)
    root = np.sqrt(d2[:, 1:]).astype(np.float64)            # np.sqrt on float32: correctly rounded
    acc = np.zeros(len(d2), np.float64)
    for j in range(mean_k):
        acc = acc + root[:, j]
    return (acc / np.float64(mean_k)).astype(np.float32)


def sor(pts, mean_k=10, stddev_mul=1.0):
    """-> dict(rc, keep bool [n], mean_dist float32 [n] (NaN: skipped), stats (mean, stddev, threshold), n_finite).
    rc 1: at most mean_k finite points, they pass through (mean_dist 0, stats 0, 0, inf)."""
    if not (1 <= mean_k <= MAX_MEAN_K) or not math.isfinite(stddev_mul):
        raise ValueError("mean_k in [1, 32], stddev_mul finite")
    p = np.asarray(pts, np.float32)
    p = p if p.ndim == 2 else p.reshape(-1, 3)
    fin = finite_mask(p)
    n = int(fin.sum())
    dist = np.full(len(p), np.nan, np.float32)
    if n <= mean_k:
        dist[fin] = 0.0
        return dict(rc=1, keep=fin.copy(), mean_dist=dist, stats=(0.0, 0.0, math.inf), n_finite=n)
    d = mean_distances(p[fin], mean_k)
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
    return dict(rc=0, keep=keep, mean_dist=dist, stats=(mean, sd, thr), n_finite=n)


def bracket(thr, n):
    """Half-width of the band around the threshold inside which the device's fixed-order sums may decide differently."""
    return 64.0 * n * 2.0 ** -52 * abs(thr)


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
        keep = (finite_mask(w) & (moved[:, 0] >= -f32(left)) & (moved[:, 0] <= f32(right)) &
                (moved[:, 1] >= -f32(back)) & (moved[:, 1] <= f32(front)))
    out = np.concatenate([moved[keep], w[keep, 3:4]], 1)
    return out, keep
