"""numpy restatement of pcl::IterativeClosestPoint<PointXYZI, PointXYZI>::computeTransformation (PCL 1.10, no rejectors,
TransformationEstimationSVD, DefaultConvergenceCriteria) and getFitnessScore as include/liogpu.h lio_icp_align states them:
the checker of tests/test_icp_cpu.py, tests/test_gpu_icp.py and tests/test_gpu_icp_edges.py.  Brute-force fp32 1-NN,
np.linalg.svd in fp64, the criteria line by line, and grid_of: the search grid of the target in np.float32, which the hook
lio_icp_debug_grid arbitrates.  The conventions where PCL is not a function of its inputs are DESIGN.md section 2's (parity unpinned)."""
import numpy as np

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DBL_MAX = np.finfo(np.float64).max

DEFAULTS = dict(max_corr_dist=30.0, transform_eps=1e-6, fitness_eps=1e-6, rel_mse_eps=1e-5, rotation_threshold=0.99999,
                fitness_max=0.3, max_iters=100, min_corr=3, max_similar=0, min_source_points=300, min_target_points=1000)


MAX_COORD = np.float32(1.0e15)                              # LIO_MAX_COORD: the bound of the target's cell sort
F32 = np.float32


def target_ok(tgt):
    """The target points that take part (include/liogpu.h lio_icp_align): every coordinate within MAX_COORD in magnitude."""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(tgt, np.float32)[:, :3]) <= MAX_COORD).all(1)


def nn_brute(src, tgt, chunk=512):
    """1-NN of every src point in tgt: FLANN L2_Simple ((dx*dx)+dy*dy)+dz*dz in fp32, ties to the lower index.
    -> (idx int64 [n], d2 float32 [n]); non-finite src points get idx -1.  A target point takes part when all three of its
    coordinates are within MAX_COORD (a distance that overflows is inf and still orders: the lowest index of those)."""
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)
    ok_t = target_ok(tgt)
    ids = np.nonzero(ok_t)[0]
    t = tgt[ok_t]
    idx = np.full(len(src), -1, np.int64)
    d2o = np.full(len(src), np.inf, np.float32)
    if len(t) == 0:
        return idx, d2o
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(src), chunk):
            s = src[a:a + chunk]
            dx = s[:, None, 0] - t[None, :, 0]
            dy = s[:, None, 1] - t[None, :, 1]
            dz = s[:, None, 2] - t[None, :, 2]
            d2 = ((dx * dx) + dy * dy) + dz * dz
            j = np.argmin(d2, axis=1)                       # first minimum = lowest index
            fin = np.isfinite(s).all(1)
            idx[a:a + chunk] = np.where(fin, ids[j], -1)
            d2o[a:a + chunk] = np.where(fin, d2[np.arange(len(s)), j], np.inf)
    return idx, d2o


def _ord(v):
    """float32 -> uint32 whose unsigned order is the float order (-0 below +0), as the device's box reduction orders them."""
    b = np.asarray(v, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def grid_cells(G, pts):
    """floor((p - origin) * inv_cell) per axis in fp32 (the formula that bins the target and places a query), unclamped,
    as float64 integers [n, 3]."""
    p = np.asarray(pts, np.float32)[:, :3]
    o = np.asarray(G["origin"], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor((p - o[None, :]) * F32(G["inv_cell"])).astype(np.float64)


def _lay(mn, mx, e):
    inv = F32(1.0) / F32(e)
    n = [int(np.floor((mx[a] - mn[a]) * inv)) + 1 for a in range(3)]
    return inv, n


def grid_of(target, per_cell=F32(4.0)):
    """The grid lio_icp_choose_grid lays over `target` at `per_cell` points per occupied cell (the alignment's 4; the outlier
    filter passes (mean_k + 1) / 3, tests/localmap_restate.py sor_grid), in np.float32 arithmetic:
    -> dict(origin [3], edge, inv_cell, nx, ny, nz, n_cells, occupied) or None when an axis has no coordinate in range.
    occupied = -1: the box is a point, no trial grid, edge 1."""
    t = np.asarray(target, np.float32)[:, :3]
    n = len(t)
    with np.errstate(invalid="ignore"):
        ok = np.abs(t) <= MAX_COORD                         # the box: per axis, whatever the point's other coordinates are
    if n == 0 or not ok.any(0).all():
        return None
    mn = np.zeros(3, np.float32)
    mx = np.zeros(3, np.float32)
    for a in range(3):
        v = t[ok[:, a], a]
        o = _ord(v)
        mn[a], mx[a] = v[np.argmin(o)], v[np.argmax(o)]
    ext = max(max(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2])
    e, occ = F32(1.0), -1
    if ext > F32(1.0e-6):
        e0 = ext / F32(64.0)
        inv0, n0 = _lay(mn, mx, e0)
        pts = t[ok.all(1)]                                  # lio_map_cell: the point's three coordinates in range ...
        c = np.floor((pts - mn[None, :]) * inv0)
        c = np.minimum(np.maximum(c, F32(-4.0)), np.array(n0, np.float32)[None, :] + F32(3.0)).astype(np.int64)
        inside = ((c >= 0) & (c < np.array(n0)[None, :])).all(1)                                    # ... and its cell in the grid
        c = c[inside]
        occ = len(np.unique((c[:, 2] * n0[1] + c[:, 1]) * n0[0] + c[:, 0]))
        ppc = F32(n) / F32(occ) if occ > 0 else F32(1.0)
        e = e0 * np.sqrt(F32(per_cell) / ppc)
        e = min(max(e, ext / F32(500.0)), ext)
        while True:
            _, nn = _lay(mn, mx, e)
            if nn[0] * nn[1] * nn[2] <= (1 << 22):
                break
            e = e * F32(1.26)
    inv, nn = _lay(mn, mx, e)
    nc = nn[0] * nn[1] * nn[2]
    return dict(origin=mn, edge=F32(e), inv_cell=F32(inv), nx=nn[0], ny=nn[1], nz=nn[2], n_cells=min(nc, 0x7fffffff), occupied=occ)


def transform_points(M, p):
    """pcl::transformPointCloud per point: ((m00 x + m01 y) + m02 z) + m03 in fp32; non-finite points pass through."""
    M = np.asarray(M, np.float32)
    p = np.asarray(p, np.float32)
    out = p.copy()
    fin = np.isfinite(p).all(1)
    x, y, z = p[fin, 0], p[fin, 1], p[fin, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            out[fin, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    return out


def compose(step, final):
    """final = step * final, fp32, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    a = np.asarray(step, np.float32)
    b = np.asarray(final, np.float32)
    out = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            out[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return out


def umeyama_rotation(cov):
    """R = U S V^T of the 3x3 cross-covariance (target x source^T), S = diag(1, 1, sign(det U det V)); -> (R, reflected)."""
    U, _, Vt = np.linalg.svd(cov)
    refl = np.linalg.det(U) * np.linalg.det(Vt) < 0
    S = np.diag([1.0, 1.0, -1.0 if refl else 1.0])
    return U @ S @ Vt, bool(refl)


def umeyama_step(s, t):
    """TransformationEstimationSVD on the pairs (s_i -> t_i): fp64 sums of s, t and t s^T (the fp32 products are exact),
    means and cross-covariance from the sums, fp64 SVD, rounded once to fp32.  -> (step 4x4 float32, reflected)."""
    s = np.asarray(s, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    n = len(s)
    ms, mt = s.sum(0) / n, t.sum(0) / n
    cov = (t[:, :, None] * s[:, None, :]).sum(0) / n - np.outer(mt, ms)
    R, refl = umeyama_rotation(cov)
    step = np.eye(4, dtype=np.float32)
    step[:3, :3] = R.astype(np.float32)
    step[:3, 3] = (mt - R @ ms).astype(np.float32)
    return step, refl


class Criteria:
    """DefaultConvergenceCriteria::hasConverged, evaluated after ++iterations on the fp32 step and the correspondences' MSE."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.mse_prev = DBL_MAX
        self.similar = 0

    def has_converged(self, iters, step, mse):
        c = self.cfg
        step = np.asarray(step, np.float32).astype(np.float64)
        if iters >= c["max_iters"]:
            return True, ITERATIONS
        similar = False
        cos = 0.5 * (((step[0, 0] + step[1, 1]) + step[2, 2]) - 1.0)
        tsq = (step[0, 3] * step[0, 3] + step[1, 3] * step[1, 3]) + step[2, 3] * step[2, 3]
        if cos >= c["rotation_threshold"] and tsq <= c["transform_eps"]:
            if self.similar >= c["max_similar"]:
                return True, TRANSFORM
            similar = True
        with np.errstate(all="ignore"):
            if abs(mse - self.mse_prev) < c["fitness_eps"]:
                if self.similar >= c["max_similar"]:
                    return True, ABS_MSE
                similar = True
            if np.float64(abs(mse - self.mse_prev)) / np.float64(self.mse_prev) < c["rel_mse_eps"]:
                if self.similar >= c["max_similar"]:
                    return True, REL_MSE
                similar = True
        self.similar = self.similar + 1 if similar else 0
        self.mse_prev = mse
        return False, NOT_CONVERGED


def correspondences(cur, tgt, cfg):
    """-> (corr int64 [n] with -1 for none, mse double, n_corr)."""
    idx, d2 = nn_brute(cur, tgt)
    keep = (idx >= 0) & (d2.astype(np.float64) <= cfg["max_corr_dist"] ** 2)
    corr = np.where(keep, idx, -1)
    n = int(keep.sum())
    mse = float(d2[keep].astype(np.float64).sum() / n) if n else 0.0
    return corr, mse, n


def fitness(final, src, tgt):
    """getFitnessScore(): the original source under `final` in one step, 1-NN without a gate, double mean of the fp32 d2."""
    moved = transform_points(final, src)
    idx, d2 = nn_brute(moved, tgt)
    keep = (idx >= 0) & (d2.astype(np.float64) <= DBL_MAX)
    n = int(keep.sum())
    return float(d2[keep].astype(np.float64).sum() / n) if n else DBL_MAX


def icp(src, tgt, cfg=None, guess=None):
    """-> dict(converged, state, iters, n_corr_last, T, fitness, steps, n_corr, mse)."""
    cfg = dict(DEFAULTS, **(cfg or {}))
    src = np.asarray(src, np.float32)[:, :3]
    tgt = np.asarray(tgt, np.float32)[:, :3]
    final = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).reshape(4, 4).copy()
    cur = transform_points(final, src)
    crit = Criteria(cfg)
    out = dict(converged=0, state=NOT_CONVERGED, iters=0, n_corr_last=0, steps=[], n_corr=[], mse=[])
    while True:
        corr, mse, n = correspondences(cur, tgt, cfg)
        out["n_corr"].append(n); out["mse"].append(mse); out["n_corr_last"] = n
        if n < cfg["min_corr"]:
            out["state"] = NO_CORRESPONDENCES
            break
        keep = corr >= 0
        step, _ = umeyama_step(cur[keep], tgt[corr[keep]])
        cur = transform_points(step, cur)                   # incrementally, not from the original
        final = compose(step, final)
        out["steps"].append(step)
        out["iters"] += 1
        conv, state = crit.has_converged(out["iters"], step, mse)
        if conv:
            out["converged"], out["state"] = 1, state
            break
    out["T"] = final
    out["fitness"] = fitness(final, src, tgt) if len(src) and len(tgt) else DBL_MAX
    return out


def pose_corrected(T, pose_wrong):
    """[roll,pitch,yaw,x,y,z] of T * tWrong (MO:1140-1143: pclPointToAffine3f, then getTranslationAndEulerAngles), fp64."""
    r, p, y = (float(v) for v in pose_wrong[:3])
    A, B, C, D, E, F = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    W = np.array([[A * C, A * D * F - B * E, B * F + A * D * E, float(pose_wrong[3])],
                  [B * C, A * E + B * D * F, B * D * E - A * F, float(pose_wrong[4])],
                  [-D, C * F, C * E, float(pose_wrong[5])], [0, 0, 0, 1.0]])
    Tc = np.asarray(T, np.float32).astype(np.float64).reshape(4, 4) @ W
    return np.array([np.arctan2(Tc[2, 1], Tc[2, 2]), np.arcsin(-Tc[2, 0]), np.arctan2(Tc[1, 0], Tc[0, 0]),
                     Tc[0, 3], Tc[1, 3], Tc[2, 3]])


def detect_loop_literal(xyz, times, radius, time_diff, time_cur):
    """MO:1271-1304 as a literal loop: radius set d2 < r2 around the last pose ordered by (d2, index), the first entry whose
    |time - time_cur| > time_diff.  -> (key_cur, key_pre) or None."""
    xyz = np.asarray(xyz, np.float32)
    last = len(xyz) - 1
    if last < 0:
        return None
    d = xyz - xyz[last]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r2 = np.float32(np.float64(np.float32(radius)) ** 2)
    hits = sorted((float(d2[i]), i) for i in range(len(xyz)) if d2[i] < r2)
    pre = -1
    for _, i in hits:
        if abs(times[i] - time_cur) > time_diff:
            pre = i
            break
    if pre == -1 or pre == last:
        return None
    return last, pre
