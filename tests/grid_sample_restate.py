"""Scalar restatement of grid_map::GridMap::atPosition with its four InterpolationMethods, written from the reference text
(GM = grid_map_core/src/GridMap.cpp, GMM = GridMapMath.cpp, CI = CubicInterpolation.cpp / .hpp), as include/liogpu.h
lio_grid_sample states it.  Python floats are IEEE doubles and nothing here fuses a multiply with an add, so every operation
is the fp64 operation the reference writes, in its order; a layer value is a float32 widened to double; the result is rounded
to float32 once.  startIndex is always 0 (the library's grids are never circular buffers).

What is not the reference's:
 - a position outside the map (or whose index is) reads nothing: value = the quiet NaN 0x7fc00000, method used = OUTSIDE, where
   the reference throws;
 - a linear tap with linear index == rows * cols fails the range test (the reference reads one float past the buffer);
 - border = 1: every tap index of the interpolating methods is clamped into the grid (an extension);
 - the order of the four terms inside a 4 x 4 product is k = 0 .. 3 (Eigen's is not defined by the source: unpinned).
"""
import math

import numpy as np

NEAREST, LINEAR, CUBIC_CONVOLUTION, CUBIC, OUTSIDE = 0, 1, 2, 3, 255
QNAN_BITS = 0x7fc00000
f32, u32 = np.float32, np.uint32

CONV_M = ((0.0, 2.0, 0.0, 0.0), (-1.0, 0.0, 1.0, 0.0), (2.0, -5.0, 4.0, -1.0), (-1.0, 3.0, -3.0, 1.0))        # CI.hpp:70-74
BICUBIC_M = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (-3.0, 3.0, -2.0, -1.0), (2.0, -2.0, 1.0, 1.0))     # CI.hpp:159-163


class Geometry:
    """GridMap::setGeometry's members: size, resolution, length = size * resolution, position"""

    def __init__(self, rows, cols, resolution, position=(0.0, 0.0)):
        self.size = (int(rows), int(cols))
        self.res = float(resolution)
        self.length = (rows * self.res, cols * self.res)
        self.pos = (float(position[0]), float(position[1]))


def in_range(index, size):                                     # checkIfIndexInRange, GMM:206-209
    return 0 <= index[0] < size[0] and 0 <= index[1] < size[1]


def position_from_index(g, index):                             # getPositionFromIndex, GMM:130-145 (None: false, `position` untouched)
    if not in_range(index, g.size):
        return None
    return tuple(g.pos[a] + (0.5 * g.length[a] - 0.5 * g.res) + g.res * float(-index[a]) for a in range(2))


def _trunc(v):
    return int(v) if math.isfinite(v) and abs(v) < 2.0 ** 31 else -2 ** 31


def index_from_position(g, p):                                 # getIndexFromPosition, GMM:147-160 -> (verdict, index)
    index = tuple(_trunc(-((p[a] - 0.5 * g.length[a] - g.pos[a]) / g.res)) for a in range(2))
    return within_map(g, p) and in_range(index, g.size), index


def within_map(g, p):                                          # checkIfPositionWithinMap, GMM:162-172
    t = tuple(-(p[a] - g.pos[a] - 0.5 * g.length[a]) for a in range(2))
    return t[0] >= 0.0 and t[1] >= 0.0 and t[0] < g.length[0] and t[1] < g.length[1]


def clamp(i, n):
    return 0 if i < 0 else (n - 1 if i >= n else i)


def bind(i, n, border):                                        # bindIndexToRange on unsigned int, CI:15-21
    if border:
        return clamp(i, n)
    u = i % (1 << 32)
    return n - 1 if u >= n else u


def dot4(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]


class Layer:
    """a [rows, cols] float32 layer: doubles for the arithmetic, the words for nearest"""

    def __init__(self, a):
        a = np.asarray(a, f32)
        self.rows, self.cols = a.shape
        self.words = np.ascontiguousarray(a).view(u32)
        self.flat = np.asfortranarray(a).ravel(order="F").astype(np.float64).tolist()      # layerMat(indexLin): column-major

    def at(self, r, c):
        assert 0 <= r < self.rows and 0 <= c < self.cols, (r, c)
        return self.flat[c * self.rows + r]

    def at_lin(self, k):
        assert 0 <= k < self.rows * self.cols, k
        return self.flat[k]


def linear(g, layer, p, index, border):                        # atPositionLinearInterpolated, GM:777-846 -> value or None
    rows, cols = g.size
    point = position_from_index(g, index)
    ind = [index, None, None, None]
    if p[0] >= point[0]:
        ind[1] = (index[0] - 1, index[1])
        up = True
    else:
        ind[1] = (index[0] + 1, index[1])
        up = False
    if p[1] >= point[1]:
        ind[2] = (index[0], index[1] - 1)
        shift = (0, 1, 2, 3) if up else (1, 0, 3, 2)
    else:
        ind[2] = (index[0], index[1] + 1)
        shift = (2, 3, 0, 1) if up else (3, 2, 1, 0)
    ind[3] = (ind[1][0], ind[2][1])
    if border:
        ind = [(clamp(i[0], rows), clamp(i[1], cols)) for i in ind]
    f = []
    for k in range(4):
        i = ind[shift[k]]
        lin = i[1] * rows + i[0]                               # getLinearIndexFromIndex, as size_t: negative fails
        if lin < 0 or lin >= rows * cols:                      # (the reference: > endIndexLin)
            return None
        f.append(layer.at_lin(lin))
    moved = position_from_index(g, ind[shift[0]])
    if moved is not None:                                      # (a failed getPosition leaves `point` as it was)
        point = moved
    red = ((p[0] - point[0]) / g.res, (p[1] - point[1]) / g.res)
    flip = (1.0 - red[0], 1.0 - red[1])
    return f[0] * flip[0] * flip[1] + f[1] * red[0] * flip[1] + f[2] * flip[0] * red[1] + f[3] * red[0] * red[1]


def convolve_1d(t, fv):                                        # CI:72-79
    tv = (1.0, t, t * t, t * t * t)
    temp = [dot4(CONV_M[r], fv) for r in range(4)]
    return 0.5 * dot4(tv, temp)


def cubic_convolution(g, layer, p, index, border):             # CI:44-135
    rows, cols = g.size
    i, j = index
    fn = lambda r, c: layer.at(bind(r, rows, border), bind(c, cols, border))
    data = [[fn(i + 1, j + 1), fn(i, j + 1), fn(i - 1, j + 1), fn(i - 2, j + 1)],
            [fn(i + 1, j), fn(i, j), fn(i - 1, j), fn(i - 2, j)],
            [fn(i + 1, j - 1), fn(i, j - 1), fn(i - 1, j - 1), fn(i - 2, j - 1)],
            [fn(i + 1, j - 2), fn(i, j - 2), fn(i - 1, j - 2), fn(i - 2, j - 2)]]
    knot = position_from_index(g, index)
    tx, ty = (p[0] - knot[0]) / g.res, (p[1] - knot[1]) / g.res
    b = [convolve_1d(tx, data[r]) for r in range(4)]
    return convolve_1d(ty, b)


def bicubic(g, layer, p, index, border):                       # CI:150-432
    rows, cols = g.size
    res = g.res
    x0, y0 = position_from_index(g, index)
    i0, j0 = index
    if p[0] > x0:
        if p[1] > y0:
            tl, tr, bl, br = (i0, j0 - 1), (i0 - 1, j0 - 1), (i0, j0), (i0 - 1, j0)
        else:
            tl, tr, bl, br = (i0, j0), (i0 - 1, j0), (i0, j0 + 1), (i0 - 1, j0 + 1)
    else:
        if p[1] > y0:
            tl, tr, bl, br = (i0 + 1, j0 - 1), (i0, j0 - 1), (i0 + 1, j0), (i0, j0)
        else:
            tl, tr, bl, br = (i0 + 1, j0), (i0, j0), (i0 + 1, j0 + 1), (i0, j0 + 1)
    bd = lambda ix: (bind(ix[0], rows, border), bind(ix[1], cols, border))
    tl, tr, bl, br = bd(tl), bd(tr), bd(bl), bd(br)
    br_, bc_ = (lambda i: bind(i, rows, border)), (lambda i: bind(i, cols, border))

    def f(ix):
        return layer.at(ix[0], ix[1])

    def dfx(ix):                                               # firstOrderDerivativeAt, Dim2D::X
        left = layer.at(br_(ix[0] + 1), ix[1])
        right = layer.at(br_(ix[0] - 1), ix[1])
        return (right - left) / (2.0 * res) * res

    def dfy(ix):
        left = layer.at(ix[0], bc_(ix[1] + 1))
        right = layer.at(ix[0], bc_(ix[1] - 1))
        return (right - left) / (2.0 * res) * res

    def ddfxy(ix):                                             # mixedSecondOrderDerivativeAt
        f11 = layer.at(br_(ix[0] - 1), bc_(ix[1] - 1))
        f1m1 = layer.at(br_(ix[0] - 1), bc_(ix[1] + 1))
        fm11 = layer.at(br_(ix[0] + 1), bc_(ix[1] - 1))
        fm1m1 = layer.at(br_(ix[0] + 1), bc_(ix[1] + 1))
        return (f11 - f1m1 - fm11 + fm1m1) / (4.0 * res * res) * res * res

    F = [[0.0] * 4 for _ in range(4)]
    for fn, (r0, c0) in ((f, (0, 0)), (ddfxy, (2, 2)), (dfy, (0, 2)), (dfx, (2, 0))):      # CI:416-432
        F[r0][c0] = fn(bl)
        F[r0 + 1][c0] = fn(br)
        F[r0][c0 + 1] = fn(tl)
        F[r0 + 1][c0 + 1] = fn(tr)
    origin = position_from_index(g, bl)
    tx, ty = (p[0] - origin[0]) / res, (p[1] - origin[1]) / res
    xv = (1.0, tx, tx * tx, tx * tx * tx)
    yv = (1.0, ty, ty * ty, ty * ty * ty)
    temp = [[dot4(F[r], BICUBIC_M[c]) for c in range(4)] for r in range(4)]                  # F * M^T
    coeff = [[dot4(BICUBIC_M[r], [temp[k][c] for k in range(4)]) for c in range(4)] for r in range(4)]
    tv = [dot4(coeff[r], yv) for r in range(4)]
    return dot4(xv, tv)


def to_f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(v)


def at_position(g, layer, p, method=NEAREST, border=0):
    """GM:161-204 -> (float32 value, method used)"""
    inside, index = index_from_position(g, p)
    if not inside:
        return np.array([QNAN_BITS], u32).view(f32)[0], OUTSIDE
    if method == CUBIC_CONVOLUTION:
        v = cubic_convolution(g, layer, p, index, border)
        if math.isfinite(v):
            return to_f32(v), CUBIC_CONVOLUTION
        method = LINEAR
    elif method == CUBIC:
        v = bicubic(g, layer, p, index, border)
        if math.isfinite(v):
            return to_f32(v), CUBIC
        method = LINEAR
    if method == LINEAR:
        v = linear(g, layer, p, index, border)
        if v is not None:
            return to_f32(v), LINEAR
    return layer.words[index[0], index[1]:index[1] + 1].view(f32)[0], NEAREST


def sample(g, layers, positions, method=NEAREST, border=0):
    """-> values [n_layers, n] float32, method used [n_layers, n] uint8, {n_outside, n_method}: what lio_grid_sample returns"""
    layers = [l if isinstance(l, Layer) else Layer(l) for l in layers]
    pts = np.asarray(positions, np.float64).reshape(-1, 2).tolist()
    vals = np.zeros((len(layers), len(pts)), f32)
    used = np.zeros((len(layers), len(pts)), np.uint8)
    for k, layer in enumerate(layers):
        assert (layer.rows, layer.cols) == g.size
        for q, p in enumerate(pts):
            v, m = at_position(g, layer, p, method, border)
            vals[k, q:q + 1].view(u32)[0] = np.array([v], f32).view(u32)[0]
            used[k, q] = m
    info = dict(n_outside=int((used == OUTSIDE).sum()), n_method=[int((used == m).sum()) for m in range(4)])
    return vals, used, info


# ---- the seven analytic surfaces of grid_map_core/test/test_helpers.cpp:21-167 on the maps of CubicInterpolationTest.cpp
WORLDS = {"flat": (2.0, 0.1), "rational": (3.0, 0.01), "saddle": (3.0, 0.1), "poly": (3.0, 0.1), "sine": (3.0, 0.01), "tanh": (2.5, 0.02),
          "gaussian": (3.0, 0.02)}
MAX_ABS_ERROR = 1e-3                                           # test_helpers.hpp:49


def analytic_world(kind, seed, n_points=1000):
    """-> (Geometry, layer [rows, cols] float32, f(x, y) on arrays, points [n, 2]): the reference's parameter ranges drawn with
    numpy.random.default_rng(seed), the map filled as fillGridMap does, the points at least 3 cells from the edges"""
    rng = np.random.default_rng(seed)
    length, res = WORLDS[kind]
    n = int(round(length / res))
    g = Geometry(n, n, res)
    if kind == "flat":
        f = lambda x, y: np.zeros(np.broadcast(x, y).shape)
    elif kind == "rational":
        x0, y0 = rng.uniform(-3.0, 3.0, 2)
        s = rng.uniform(1.0, 20.0)
        f = lambda x, y: s / (1 + (x - x0) ** 2.0 + (y - y0) ** 2.0)
    elif kind == "poly":
        f = lambda x, y: -x * x - y * y + 2.0 * x * y + x * x * y * y
    elif kind == "saddle":
        f = lambda x, y: x * x - y * y
    elif kind == "sine":
        w = rng.uniform(0.1, 4.0, 4)
        f = lambda x, y: np.cos(w[0] * x) + np.sin(w[1] * y) + np.cos(w[2] * x) + np.sin(w[3] * y)
    elif kind == "tanh":
        s = rng.uniform(0.1, 2.0)
        f = lambda x, y: (np.exp(2 * s * x) - 1) / (np.exp(2 * s * x) + 1) + 0.0 * y
    elif kind == "gaussian":
        gs = [(rng.uniform(-4.0, 4.0), rng.uniform(-4.0, 4.0), rng.uniform(0.1, 3.0), rng.uniform(0.1, 3.0), rng.uniform(-3.0, 3.0)) for _ in range(3)]
        f = lambda x, y: sum(s * np.exp(-(x - x0) * (x - x0) / (2.0 * vx) - (y - y0) * (y - y0) / (2.0 * vy)) for x0, y0, vx, vy, s in gs)
    else:
        raise KeyError(kind)
    xs = np.array([position_from_index(g, (i, 0))[0] for i in range(n)])
    ys = np.array([position_from_index(g, (0, j))[1] for j in range(n)])
    layer = np.asarray(f(xs[:, None], ys[None, :]), np.float64).astype(f32)
    dim = g.length[0] / 2.0 - 3.0 * res
    pts = np.c_[rng.uniform(-dim, dim, n_points), rng.uniform(-dim, dim, n_points)]
    return g, layer, f, pts


def border_lattice(g):
    """Test positions that walk every decision of the index work: every cell centre, every cell edge and corner, the four
    quadrants of every cell, both map edges on both axes and one step beyond them."""
    axes = []
    for a in range(2):
        n = g.size[a]
        hi = g.pos[a] + 0.5 * g.length[a]
        ticks = []
        for k in range(n + 1):
            edge = hi - k * g.res
            ticks += [edge, edge - 0.25 * g.res, edge - 0.5 * g.res, edge - 0.75 * g.res]
        ticks = ticks[:-3] + [hi + 0.3 * g.res, hi + g.res, g.pos[a] - 0.5 * g.length[a] - 0.3 * g.res, g.pos[a] - 0.5 * g.length[a] - g.res,
                              math.nextafter(hi, math.inf), math.nextafter(g.pos[a] - 0.5 * g.length[a], math.inf)]
        axes.append(ticks)
    return np.array([(x, y) for x in axes[0] for y in axes[1]], np.float64)
