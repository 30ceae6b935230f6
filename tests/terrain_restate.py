"""numpy restatement of the terrain layers: grid_map_demos' filter chain behind `elevation_inpainted`,
restated from the source text of grid_map_core / grid_map_filters and from the published algorithm of Eigen's
SelfAdjointEigenSolver<Matrix3d>::computeDirect.  Python floats are IEEE doubles and numpy's float32 scalars round after
every operation, so each line below is one rounded operation in the order the reference performs it.  Plain loops: the
grids of the tests are small.  tests/test_terrain_cpu.py pins this file."""
import math

import numpy as np

f32 = np.float32
EPS = 2.0 ** -52                                               # std::numeric_limits<double>::epsilon()
LAYERS = ("smooth", "normal_x", "normal_y", "normal_z", "slope", "roughness", "edges", "traversability")
DEFAULTS = dict(normal_method=0, normal_axis=2, normal_radius=0.05, smooth_radius=0.06, edge_window_size=0, edge_window_length=0.05,
                slope_critical=0.6, roughness_critical=0.1, slope_weight=0.5, roughness_weight=0.5)


class Geom:
    """GridMap::setGeometry's members for a grid of rows x cols cells, default start index"""
    def __init__(self, rows, cols, resolution, position):
        self.rows, self.cols, self.res = int(rows), int(cols), float(resolution)
        self.size = (self.rows, self.cols)
        self.pos = (float(position[0]), float(position[1]))
        self.len = (self.rows * self.res, self.cols * self.res)
        self.half = (0.5 * self.len[0], 0.5 * self.len[1])                                # getVectorToOrigin
        self.base = tuple(self.pos[a] + (self.half[a] - 0.5 * self.res) for a in range(2))   # mapPosition + getVectorToFirstCell


def centre(G, a, i):
    """getPositionFromIndex, GridMapMath.cpp:130-145, one component"""
    return G.base[a] + G.res * float(-i)


def index_of(G, a, p):
    """boundPositionToRange (GridMapMath.cpp:255-280), then getIndexFromPosition (:147-160) whose verdict nobody reads; an
    index outside the buffer is brought back to the last cell"""
    eps = 10.0 * EPS
    if abs(p) > 1.0:
        eps *= abs(p)
    sh = (p - G.pos[a]) + G.half[a]
    if sh <= 0.0:
        sh = eps
    elif sh >= G.len[a]:
        sh = G.len[a] - eps
    q = (sh + G.pos[a]) - G.half[a]
    v = ((q - G.half[a]) - G.pos[a]) / G.res
    return min(max(int(-v), 0), G.size[a] - 1)                 # int(): toward zero, as the conversion to Index


def window(G, a, c, radius):
    """CircleIterator::findSubmapParameters along one axis: first and last candidate"""
    return index_of(G, a, c + radius), index_of(G, a, c - radius)


def circle(G, r, c, radius):
    """the cells CircleIterator visits around cell (r, c), in its order (SubmapIterator: column index fastest)"""
    cx, cy = centre(G, 0, r), centre(G, 1, c)
    i0, i1 = window(G, 0, cx, radius)
    j0, j1 = window(G, 1, cy, radius)
    r2 = radius * radius
    out = []
    for i in range(i0, i1 + 1):
        dx = centre(G, 0, i) - cx
        dx2 = dx * dx
        for j in range(j0, j1 + 1):
            dy = centre(G, 1, j) - cy
            if dx2 + dy * dy <= r2:
                out.append((i, j))
    return out


def smooth(grid, G, radius):
    """MeanInRadiusFilter.cpp:59-79"""
    out = np.full(grid.shape, np.nan, f32)
    for r in range(G.rows):
        for c in range(G.cols):
            s, n = 0.0, 0
            for i, j in circle(G, r, c, radius):
                v = grid[i, j]
                if np.isfinite(v):
                    s += float(v)
                    n += 1
            if n:
                out[r, c] = f32(s / float(n))
    return out


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _kernel_of(a00, a11, a22, a10, a20, a21):
    """extract_kernel: -> (unit vector of the kernel, the representative column)"""
    i0, m = 0, abs(a00)
    if abs(a11) > m:
        i0, m = 1, abs(a11)
    if abs(a22) > m:
        i0 = 2
    cols = ((a00, a10, a20), (a10, a11, a21), (a20, a21, a22))
    rep, A, B = cols[i0], cols[(i0 + 1) % 3], cols[(i0 + 2) % 3]
    pa, pb = _cross(rep, A), _cross(rep, B)
    n0, n1 = _dot(pa, pa), _dot(pb, pb)
    if n0 > n1:
        s = math.sqrt(n0)
        return (pa[0] / s, pa[1] / s, pa[2] / s), rep
    s = math.sqrt(n1)
    return (pb[0] / s, pb[1] / s, pb[2] / s), rep


def covariance(n, s, q):
    """sumSquared / nPoints - mean * mean^T as (a00, a10, a11, a20, a21, a22); q = (xx, yx, yy, zx, zy, zz)"""
    dn = float(n)
    m0, m1, m2 = s[0] / dn, s[1] / dn, s[2] / dn
    return (q[0] / dn - m0 * m0, q[1] / dn - m1 * m0, q[2] / dn - m1 * m1, q[3] / dn - m2 * m0, q[4] / dn - m2 * m1, q[5] / dn - m2 * m2)


def eigen_direct(n, s, q):
    """SelfAdjointEigenSolver<Matrix3d>::computeDirect on the covariance -> (eigenvalues (3), eigenvectors().col(0))"""
    a00, a10, a11, a20, a21, a22 = covariance(n, s, q)
    shift = ((a00 + a11) + a22) / 3.0
    a00, a11, a22 = a00 - shift, a11 - shift, a22 - shift
    scale = max(abs(a00), abs(a10), abs(a20), abs(a11), abs(a21), abs(a22))
    if scale > 0.0:
        a00, a10, a20, a11, a21, a22 = a00 / scale, a10 / scale, a20 / scale, a11 / scale, a21 / scale, a22 / scale
    inv3, sqrt3 = 1.0 / 3.0, math.sqrt(3.0)
    c0 = ((((a00 * a11) * a22 + ((2.0 * a10) * a20) * a21) - (a00 * a21) * a21) - (a11 * a20) * a20) - (a22 * a10) * a10
    c1 = ((((a00 * a11 - a10 * a10) + a00 * a22) - a20 * a20) + a11 * a22) - a21 * a21
    c2 = (a00 + a11) + a22
    c2_3 = c2 * inv3
    a_3 = (c2 * c2_3 - c1) * inv3
    a_3 = a_3 if a_3 > 0.0 else 0.0
    half_b = 0.5 * (c0 + c2_3 * ((2.0 * c2_3) * c2_3 - c1))
    qq = (a_3 * a_3) * a_3 - half_b * half_b
    qq = qq if qq > 0.0 else 0.0
    rho = math.sqrt(a_3)
    theta = math.atan2(math.sqrt(qq), half_b) * inv3
    ct, st = math.cos(theta), math.sin(theta)
    r0 = c2_3 - rho * (ct + sqrt3 * st)
    r1 = c2_3 - rho * (ct - sqrt3 * st)
    r2 = c2_3 + (2.0 * rho) * ct
    col0 = (1.0, 0.0, 0.0)
    if not (r2 - r0) <= EPS:
        d0, d1 = r2 - r1, r1 - r0
        if d0 > d1:
            col2, rep = _kernel_of(a00 - r2, a11 - r2, a22 - r2, a10, a20, a21)
            if d1 <= 2.0 * EPS * d1:
                t = _dot(col2, rep)
                col0 = (rep[0] - t * rep[0], rep[1] - t * rep[1], rep[2] - t * rep[2])
                z = _dot(col0, col0)
                if z > 0.0:
                    w = math.sqrt(z)
                    col0 = (col0[0] / w, col0[1] / w, col0[2] / w)
            else:
                col0, _ = _kernel_of(a00 - r0, a11 - r0, a22 - r0, a10, a20, a21)
        else:
            col0, _ = _kernel_of(a00 - r0, a11 - r0, a22 - r0, a10, a20, a21)
    return (r0 * scale + shift, r1 * scale + shift, r2 * scale + shift), col0


def circle_sums(grid, G, r, c, radius):
    """areaSingleNormalComputation's accumulation, NormalVectorsFilter.cpp:207-219 -> (nPoints, sum, sumSquared's six)"""
    s, q, n = [0.0, 0.0, 0.0], [0.0] * 6, 0
    for i, j in circle(G, r, c, radius):
        v = grid[i, j]
        if not np.isfinite(v):
            continue
        x, y, w = centre(G, 0, i), centre(G, 1, j), float(v)
        s[0] += x; s[1] += y; s[2] += w
        q[0] += x * x; q[1] += y * x; q[2] += y * y; q[3] += w * x; q[4] += w * y; q[5] += w * w
        n += 1
    return n, s, q


def _store(normal, axis, out, r, c):
    n = normal
    if n[axis] < 0.0:
        n = (-n[0], -n[1], -n[2])
    for k in range(3):
        out[k][r, c] = f32(n[k])


def normals_area(grid, G, radius, axis):
    """NormalVectorsFilter.cpp:156-170, 195-251 -> ((nx, ny, nz), counts)"""
    out = [np.full(grid.shape, np.nan, f32) for _ in range(3)]
    counts = dict(n_normal_cells=0, n_few_points=0, n_degenerate=0)
    for r in range(G.rows):
        for c in range(G.cols):
            if not np.isfinite(grid[r, c]):
                continue
            n, s, q = circle_sums(grid, G, r, c, radius)
            normal = (0.0, 0.0, 1.0)
            if n < 3:
                counts["n_few_points"] += 1
            else:
                ev, v0 = eigen_direct(n, s, q)
                if ev[1] > 1e-8:
                    normal = v0
                else:
                    counts["n_degenerate"] += 1
            counts["n_normal_cells"] += 1
            _store(normal, axis, out, r, c)
    return out, counts


def normals_raster(grid, G, axis):
    """NormalVectorsFilter.cpp:253-273, 304-394: interior cells"""
    out = [np.full(grid.shape, np.nan, f32) for _ in range(3)]
    counts = dict(n_normal_cells=0, n_few_points=0, n_degenerate=0)
    for r in range(1, G.rows - 1):
        for c in range(1, G.cols - 1):
            centre_v, top, right, bottom, left = (float(grid[r, c]), float(grid[r - 1, c]), float(grid[r, c + 1]), float(grid[r + 1, c]),
                                                  float(grid[r, c - 1]))
            fin = math.isfinite
            kx = 1 * fin(top) + 2 * fin(centre_v) + 4 * fin(bottom)
            ky = 1 * fin(left) + 2 * fin(centre_v) + 4 * fin(right)
            if kx in (7, 5):
                dX = 2.0 * G.res
            elif kx == 6:
                top, dX = centre_v, G.res
            elif kx == 3:
                bottom, dX = centre_v, G.res
            else:
                continue
            if ky in (7, 5):
                dY = 2.0 * G.res
            elif ky == 6:
                left, dY = centre_v, G.res
            elif ky == 3:
                right, dY = centre_v, G.res
            else:
                continue
            n0, n1, n2 = (bottom - top) / dX, (right - left) / dY, 1.0
            ln = math.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            counts["n_normal_cells"] += 1
            _store((n0 / ln, n1 / ln, n2 / ln), axis, out, r, c)
    return out, counts


def slope_of(nz):
    """acos(normal_vectors_z) with the host's double arccos rounded to float: what the device's acosf is held against"""
    with np.errstate(invalid="ignore"):
        return np.arccos(np.asarray(nz, f32).astype(np.float64)).astype(f32)


def roughness_of(grid, sm):
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(grid, f32) - np.asarray(sm, f32))


def edge_window_size(length, resolution, explicit=0):
    """SlidingWindowIterator::setWindowLength, SlidingWindowIterator.cpp:35-42; an explicit size must be odd (:96-98)"""
    if explicit:
        if explicit % 2 == 0:
            raise ValueError("SlidingWindowIterator has a wrong window size!")
        return int(explicit)
    n = int(math.floor(length / resolution + 0.5))             # std::round of a non-negative number
    return n + 1 if n % 2 != 1 else n


def _sum_of_finites(a, b):
    """scalar_sum_of_finites_op, FunctorsPlugin.hpp:3-12, on float32"""
    fa, fb = np.isfinite(a), np.isfinite(b)
    if fa and fb:
        return a + b
    if fa:
        return a
    if fb:
        return b
    return a + b


def _redux(block):
    """Eigen's unvectorised redux: serially, column-major"""
    flat = block.ravel(order="F")
    acc = flat[0]
    for v in flat[1:]:
        acc = _sum_of_finites(acc, v)
    return acc


def edges_of(slope, win):
    """SlidingWindowMathExpressionFilter.cpp:74-92 with edge_handling crop and the yaml's expression, every cell"""
    slope = np.asarray(slope, f32)
    rows, cols = slope.shape
    m = (win - 1) // 2
    out = np.full(slope.shape, np.nan, f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(rows):
            for c in range(cols):
                blk = slope[max(r - m, 0):min(r + m, rows - 1) + 1, max(c - m, 0):min(c + m, cols - 1) + 1]
                n = f32(np.count_nonzero(blk == blk))
                mean = _redux(blk) / n
                d = blk - mean
                out[r, c] = np.sqrt(_redux(d * d) / n)
    return out


def traversability_of(slope, rough, s_crit=0.6, r_crit=0.1, w_s=0.5, w_r=0.5):
    """the MathExpressionFilter in float, then ThresholdFilter.cpp:79-90 twice: a NaN ends at 0"""
    slope, rough = np.asarray(slope, f32), np.asarray(rough, f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (f32(w_s) * (f32(1.0) - slope / f32(s_crit))) + (f32(w_r) * (f32(1.0) - rough / f32(r_crit)))
        t = np.where(~(t >= f32(0.0)), f32(0.0), t)
        t = np.where(~(t <= f32(1.0)), f32(1.0), t)
    return t.astype(f32)


def terrain(grid, resolution, position, **cfg):
    """the whole chain, every stage from the restatement's own preceding layers -> dict of the eight layers and the counts"""
    p = dict(DEFAULTS, **cfg)
    grid = np.asarray(grid, f32)
    G = Geom(grid.shape[0], grid.shape[1], resolution, position)
    out = dict(rows=G.rows, cols=G.cols, n_valid_cells=int(np.isfinite(grid).sum()))
    out["smooth"] = smooth(grid, G, p["smooth_radius"])
    fallback = p["normal_method"] == 0 and p["normal_radius"] <= 0
    if p["normal_method"] == 1 or fallback:
        (nx, ny, nz), counts = normals_raster(grid, G, p["normal_axis"])
    else:
        (nx, ny, nz), counts = normals_area(grid, G, p["normal_radius"], p["normal_axis"])
    out.update(counts, normal_method_used=int(fallback), normal_x=nx, normal_y=ny, normal_z=nz)
    out["slope"] = slope_of(nz)
    out["roughness"] = roughness_of(grid, out["smooth"])
    out["edge_window_size"] = edge_window_size(p["edge_window_length"], resolution, p["edge_window_size"])
    out["edges"] = edges_of(out["slope"], out["edge_window_size"])
    out["traversability"] = traversability_of(out["slope"], out["roughness"], p["slope_critical"], p["roughness_critical"], p["slope_weight"],
                                              p["roughness_weight"])
    return out


# ---- what tests/test_terrain_cpu.py and tests/test_gpu_terrain.py share ------------------------------------------------
def scene_a(position, seed=5, rows=48, cols=36, resolution=0.25):
    """the mixed scene: a tilted plane with 0.01 m noise, a 1.5 m box, a one-cell spike, 8 % random holes, one 4 x 5 hole"""
    rng = np.random.default_rng(seed)
    G = Geom(rows, cols, resolution, position)
    x = np.array([centre(G, 0, i) for i in range(rows)]) - position[0]
    y = np.array([centre(G, 1, j) for j in range(cols)]) - position[1]
    z = 0.08 * x[:, None] - 0.05 * y[None, :] + rng.normal(0, 0.01, (rows, cols))
    z[10:16, 20:26] += 1.5
    z[30, 8] += 2.0
    z[rng.uniform(size=z.shape) < 0.08] = np.nan
    z[36:40, 12:17] = np.nan
    return z.astype(f32)


def conditioning(grid, G, radius):
    """per finite cell with at least 3 points in its circle: (r, c) -> (eigenvalues by LAPACK, its eigenvector of the smallest,
    the Frobenius norm of sumSquared / n, the restatement's eigenvalues and column 0)"""
    out = {}
    for r in range(G.rows):
        for c in range(G.cols):
            if not np.isfinite(grid[r, c]):
                continue
            n, s, q = circle_sums(grid, G, r, c, radius)
            if n < 3:
                continue
            a00, a10, a11, a20, a21, a22 = covariance(n, s, q)
            w, v = np.linalg.eigh(np.array([[a00, a10, a20], [a10, a11, a21], [a20, a21, a22]]))
            ss = np.array([[q[0], q[1], q[3]], [q[1], q[2], q[4]], [q[3], q[4], q[5]]]) / float(n)
            ev, v0 = eigen_direct(n, s, q)
            out[(r, c)] = (w, v[:, 0], float(np.linalg.norm(ss)), ev, np.array(v0))
    return out


def well_conditioned(w):
    """the cells the area normals are held to their bar on: eigenvalue(1) > 1e-6 and (l1 - l0) >= 1e-3 l2"""
    return w[1] > 1e-6 and (w[1] - w[0]) >= 1e-3 * w[2]


def line_angle(a, b):
    """the angle between the lines of two vectors, accurate for small angles"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.atan2(float(np.linalg.norm(np.cross(a, b))), abs(float(np.dot(a, b))))
