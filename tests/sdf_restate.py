"""grid_map_sdf restated in numpy: the checker of lio-slam_amd/csrc/lio_sdf.h, not a second implementation to ship.

Every float expression is fp32 in the order the reference writes it (numpy's float32 array arithmetic rounds each operation
to fp32, its sqrt is correctly rounded).  The serial sweep of SignedDistance2d.cpp:30-167 is restated as written -- the float
loop counter, the `s < n` skip, the backward search, the bound that dominates all previous ones, the `> 0` skip -- but over
many independent lines at once: every line carries its own lower-bound stack and cursor, and one numpy statement advances
all of them by the same step of the same loop.  tests/test_sdf_cpu.py pins this file against the brute-force definition.

PBD = PixelBorderDistance.hpp, SD2 = SignedDistance2d.cpp, SDF = SignedDistanceField.cpp, DD = DistanceDerivatives.hpp,
G3L = Gridmap3dLookup.hpp."""
import math

import numpy as np

f32 = np.float32
INF = f32(np.inf)
MIXED, ALL_OBSTACLE, ALL_FREE = 0, 1, 2


# ---- PBD:26-101 ----------------------------------------------------------------------------------------------------------
def pixel_border_distance(i, j):
    a = np.abs(f32(i) - f32(j)) - f32(0.5)
    return np.where(a < 0, f32(0), a).astype(f32)


def square_pixel_border_distance(i, j, f):
    d = pixel_border_distance(i, j)
    return (d * d + f).astype(f32)


def right_of_origin(p, fp):
    """intersectionPointRightSideOfOrigin: the five solutions, chosen by the same comparisons in the same order"""
    with np.errstate(all="ignore"):
        pp = p * p
        sol1 = (pp + p + fp) / (f32(2) * p)
        sol5 = (pp - p + fp) / (f32(2) * p)
        bound = pp - f32(2) * p + f32(1)
        sol2 = f32(0.5) + np.sqrt(np.where(fp > 0, fp, f32(0)))
        sol4 = p - f32(0.5) - np.sqrt(np.where(fp < 0, -fp, f32(0)))
        sol3 = (pp - p + fp) / (f32(2) * p - f32(2))
        inner = np.where(fp > bound, sol2, np.where(fp < -bound, sol4, sol3))
        return np.where(fp > pp, sol1, np.where(fp < -pp, sol5, inner)).astype(f32)


def equidistance_point(q, fq, p, fp):
    with np.errstate(all="ignore"):
        q, fq, p, fp = np.broadcast_arrays(f32(q), fq, p, fp)
        df, dr = fp - fq, p - q
        off = np.where(dr > 0, right_of_origin(dr, df), -right_of_origin(-dr, df))
        return np.where(fp == fq, f32(0.5) * (p + q), off + q).astype(f32)


# ---- SD2:30-167 on many lines at once --------------------------------------------------------------------------------------
def transform_lines(f, sqrt):
    """f: [m, n] float32, every row one line.  -> the in-place transform of every line (squared, or the distance with
    sqrt = True: squaredDistanceTransform_1d_inplace / distanceTransform_1d_inplace)."""
    f = np.ascontiguousarray(f, f32)
    m, n = f.shape
    ar = np.arange(m)
    pos = f > 0
    # lastZeroFromFront
    first_pos = np.where(pos.any(axis=1), pos.argmax(axis=1), n)
    start = np.where(first_pos == n, n, np.maximum(first_pos - 1, 0))
    has = start < n
    s0 = np.where(has, start, 0)
    # fillLowerBounds: per bound the pixel index and z_rhs; z_lhs = the z_rhs of the bound below, f = the input there
    bv = np.zeros((m, n), np.int64)
    bz = np.full((m, n), INF, f32)
    bv[ar, 0] = s0
    top = np.zeros(m, np.int64)
    first = np.zeros(m, np.int64)
    tv = s0.astype(f32)
    tf = f[ar, s0].copy()
    tzl = np.full(m, -INF, f32)
    nf, sf = f32(n), start.astype(f32)
    for q in range(1, n):
        qf = f32(q)                                            # start + 1, then += 1.0F: the same float below 2^24
        fq = f[:, q]
        s = equidistance_point(qf, fq, tv, tf)
        live = has & (q > start) & (s < nf)
        while True:
            back = live & (s < tzl)
            if not back.any():
                break
            i = np.nonzero(back)[0]
            top[i] -= 1
            v = bv[i, top[i]]
            tv[i] = v.astype(f32)
            tf[i] = f[i, v]
            tzl[i] = np.where(top[i] == first[i], -INF, bz[i, top[i] - 1])
            s[i] = equidistance_point(qf, fq[i], tv[i], tf[i])
        push = np.nonzero(live & (s > sf))[0]
        dom = np.nonzero(live & ~(s > sf))[0]
        bz[push, top[push]] = s[push]
        top[push] += 1
        bv[push, top[push]] = q
        bz[push, top[push]] = INF
        tzl[push] = s[push]
        bv[dom, top[dom]] = q
        bz[dom, top[dom]] = INF
        tzl[dom] = -INF
        first[dom] = top[dom]
        tv[live] = qf
        tf[live] = fq[live]
    # extractSquareDistances / extractDistances
    out = f.copy()
    it = first.copy()
    lastz = bz[ar, it].copy()
    for q in range(n):
        qf = f32(q)
        todo = has & (q >= start) & pos[:, q]
        adv = todo & (qf > lastz)
        if adv.any():
            it[adv] += 1
            while True:
                more = adv & (bz[ar, np.minimum(it, n - 1)] < qf)
                if not more.any():
                    break
                it[more] += 1
            lastz[adv] = bz[adv, it[adv]]
        i = np.nonzero(todo)[0]
        v = bv[i, it[i]]
        d2 = square_pixel_border_distance(qf, v.astype(f32), f[i, v])
        out[i, q] = np.sqrt(d2) if sqrt else d2
    return out


def pixel_distance_2d(init):
    """computePixelDistance2dTranspose on [k, rows, cols] stacked matrices -> [k, rows, cols] (not transposed)"""
    k, rows, cols = init.shape
    a = transform_lines(init.transpose(0, 2, 1).reshape(k * cols, rows), False).reshape(k, cols, rows)      # the columns
    return transform_lines(a.transpose(0, 2, 1).reshape(k * rows, cols), True).reshape(k, rows, cols)         # the rows, with the sqrt


# ---- SD2:190-287 -----------------------------------------------------------------------------------------------------------
def init_obstacle(elev, h, res):
    d = f32(h) - elev
    t = (f32(1) / f32(res)) * np.where(d < 0, f32(0), d)
    return (t * t).astype(f32)


def init_free(elev, h, res):
    d = f32(h) - elev
    t = (f32(1) / f32(res)) * np.where(0 < d, f32(0), d)
    return (t * t).astype(f32)


def layer_mode(h, e_min, e_max):
    return ALL_OBSTACLE if f32(h) < f32(e_min) else (ALL_FREE if f32(h) > f32(e_max) else MIXED)


def signed_distance_at_height(elev, h, res, e_min, e_max):
    """signedDistanceAtHeight: [rows, cols]"""
    elev, res = np.asarray(elev, f32), f32(res)
    mode = layer_mode(h, e_min, e_max)
    with np.errstate(all="ignore"):
        if mode == ALL_OBSTACLE:
            return (pixel_distance_2d(init_free(elev, h, res)[None])[0] * -res).astype(f32)
        if mode == ALL_FREE:
            return (pixel_distance_2d(init_obstacle(elev, h, res)[None])[0] * res).astype(f32)
        d = pixel_distance_2d(np.stack([init_obstacle(elev, h, res), init_free(elev, h, res)]))
        return (res * (d[0] - d[1])).astype(f32)


def signed_distance_at_heights(elev, heights, res, e_min, e_max):
    """signedDistanceAtHeight for every height -> [len(heights), rows, cols]; the lines of all layers advance together"""
    elev, res = np.asarray(elev, f32), f32(res)
    modes = [layer_mode(h, e_min, e_max) for h in heights]
    inits, where = [], []
    for h, mode in zip(heights, modes):
        where.append((len(inits) if mode != ALL_OBSTACLE else None, len(inits) + (mode != ALL_OBSTACLE) if mode != ALL_FREE else None))
        if mode != ALL_OBSTACLE:
            inits.append(init_obstacle(elev, h, res))
        if mode != ALL_FREE:
            inits.append(init_free(elev, h, res))
    d = pixel_distance_2d(np.stack(inits))
    out = []
    with np.errstate(all="ignore"):
        for mode, (io, i_f) in zip(modes, where):
            out.append(d[i_f] * -res if mode == ALL_OBSTACLE else (d[io] * res if mode == ALL_FREE else res * (d[io] - d[i_f])))
    return np.stack(out).astype(f32)


def signed_distance_from_occupancy(occ, res):
    """signedDistanceFromOccupancy: occ [rows, cols] bool -> [rows, cols]"""
    occ = np.asarray(occ, bool)
    if not occ.any():
        return np.full(occ.shape, INF, f32)
    if occ.all():
        return np.full(occ.shape, -INF, f32)
    with np.errstate(all="ignore"):
        d = pixel_distance_2d(np.stack([np.where(occ, f32(0), INF), np.where(occ, INF, f32(0))]).astype(f32))
        return (f32(res) * (d[0] - d[1])).astype(f32)


# ---- SDF:25-171 ------------------------------------------------------------------------------------------------------------
def num_layers(min_h, max_h, res):
    return int(max(math.ceil((float(max_h) - float(min_h)) / float(res)), 2.0))


def layer_height(origin_z, res, z):
    origin_z, res = f32(origin_z), f32(res)
    if z == 0:
        return origin_z
    if z == 1:
        return f32(origin_z + res)
    return f32(origin_z + f32(f32(z) * res))


def difference(d, axis, step):
    """columnwiseCentralDifference / layerFiniteDifference / layerCentralDifference along `axis` of d"""
    step = f32(step)
    inv1, inv2 = f32(1) / step, f32(1) / (f32(2) * step)
    d = np.moveaxis(d, axis, 0)
    out = np.empty_like(d)
    with np.errstate(all="ignore"):
        out[0] = inv1 * (d[1] - d[0])
        out[1:-1] = inv2 * (d[2:] - d[:-2])
        out[-1] = inv1 * (d[-1] - d[-2])
    return np.moveaxis(out, 0, axis)


class Field:
    """SignedDistanceField: .dist [layers, rows, cols], .nodes [layers, cols, rows, 4] in data_ order, and the lookup"""

    def __init__(self, elev, res, length, position, min_h=None, max_h=None, nan_fill=False):
        elev = np.array(elev, f32)
        finite = np.isfinite(elev)
        self.n_nan = int((~finite).sum())
        self.e_min, self.e_max = f32(elev[finite].min()), f32(elev[finite].max())
        if nan_fill:
            elev[~finite] = self.e_min
        min_h = float(self.e_min) if min_h is None else float(min_h)
        max_h = float(self.e_max) if max_h is None else float(max_h)
        self.rows, self.cols = elev.shape
        self.res = float(res)
        self.layers = num_layers(min_h, max_h, res)
        self.origin = (position[0] + (0.5 * length[0] - 0.5 * self.res), position[1] + (0.5 * length[1] - 0.5 * self.res), min_h)
        self.heights = [layer_height(f32(min_h), f32(res), z) for z in range(self.layers)]
        self.modes = [layer_mode(h, self.e_min, self.e_max) for h in self.heights]
        self.dist = signed_distance_at_heights(elev, self.heights, res, self.e_min, self.e_max)
        dx = difference(self.dist, 1, -f32(res))
        dy = difference(self.dist, 2, -f32(res))
        dz = difference(self.dist, 0, f32(res))
        self.nodes = np.ascontiguousarray(np.stack([self.dist, dx, dy, dz], -1).transpose(0, 2, 1, 3))

    def nearest_node(self, p):
        inv = 1.0 / self.res
        return (nearest_index((self.origin[0] - p[0]) * inv, self.rows - 1), nearest_index((self.origin[1] - p[1]) * inv, self.cols - 1),
                nearest_index((p[2] - self.origin[2]) * inv, self.layers - 1))

    def linear_index(self, idx):
        return (idx[2] * self.cols + idx[1]) * self.rows + idx[0]

    def value_and_derivative(self, p):
        ix, iy, iz = idx = self.nearest_node(p)
        node = self.nodes.reshape(-1, 4)[self.linear_index(idx)]
        nx, ny, nz = self.origin[0] - ix * self.res, self.origin[1] - iy * self.res, self.origin[2] + iz * self.res
        der = [float(node[1]), float(node[2]), float(node[3])]
        with np.errstate(all="ignore"):
            dot = (np.float64(der[0]) * (p[0] - nx) + np.float64(der[1]) * (p[1] - ny)) + np.float64(der[2]) * (p[2] - nz)
            return float(np.float64(node[0]) + dot), der


def std_round(v):
    """std::round: halves away from zero"""
    if not math.isfinite(v):
        return v
    t = math.trunc(v)
    return float(t + (math.copysign(1.0, v) if abs(v - t) >= 0.5 else 0.0))


def nearest_index(val, mx):
    """getNearestPositiveInteger with std::min / std::max as written: a NaN ends at 0"""
    r = std_round(val)
    m = float(mx) if float(mx) < r else r
    return int(m if 0.0 < m else 0.0)


# ---- the definition (naiveSignedDistance.hpp's formula, written down in fp64) ---------------------------------------------
def brute_force_at_height(elev, h, res):
    """cell centre to the border of the nearest cell column of the other class, the height difference as third component;
    the sign by elevation >= height"""
    e = np.asarray(elev, np.float64)
    rows, cols = e.shape
    h, res = float(f32(h)), float(f32(res))
    px = res * np.maximum(np.abs(np.arange(rows)[:, None] - np.arange(rows)[None, :]) - 0.5, 0.0)      # [r, i]
    py = res * np.maximum(np.abs(np.arange(cols)[:, None] - np.arange(cols)[None, :]) - 0.5, 0.0)      # [c, j]
    planar2 = px[:, None, :, None] ** 2 + py[None, :, None, :] ** 2                                     # [r, c, i, j]
    up = np.sqrt(planar2 + np.maximum(h - e, 0.0)[None, None] ** 2).reshape(rows, cols, -1).min(-1)     # to the nearest obstacle
    down = np.sqrt(planar2 + np.maximum(e - h, 0.0)[None, None] ** 2).reshape(rows, cols, -1).min(-1)   # to the nearest free cube
    return np.where(e >= h, -down, up)


def brute_force_occupancy(occ, res):
    occ = np.asarray(occ, bool)
    rows, cols = occ.shape
    res = float(f32(res))
    px = res * np.maximum(np.abs(np.arange(rows)[:, None] - np.arange(rows)[None, :]) - 0.5, 0.0)
    py = res * np.maximum(np.abs(np.arange(cols)[:, None] - np.arange(cols)[None, :]) - 0.5, 0.0)
    d = np.sqrt(px[:, None, :, None] ** 2 + py[None, :, None, :] ** 2)
    to_obstacle = np.where(occ[None, None], d, np.inf).reshape(rows, cols, -1).min(-1)
    to_free = np.where(~occ[None, None], d, np.inf).reshape(rows, cols, -1).min(-1)
    return np.where(occ, -to_free, to_obstacle)


def is_equal_sdf(a, b, tol):
    """isEqualSdf: equal (the infinities), or closer than tol -> (verdict, the largest finite deviation)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = a == b
    with np.errstate(all="ignore"):
        dev = np.where(same, 0.0, np.abs(a - b))
    return bool((same | (dev < tol)).all()), float(np.nanmax(dev))
