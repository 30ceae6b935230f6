"""Scalar restatement of grid_map's region iterators, written from the reference text (IT = grid_map_core/src/iterators/,
GMM = GridMapMath.cpp, PG = Polygon.cpp), and of the reduction include/liogpu.h lio_grid_region_reduce states.  Python floats
are IEEE doubles and nothing here fuses a multiply with an add, so every operation is the fp64 operation the reference writes,
in its order.  The loops are the reference's serial ones: SubmapIterator's increment, LineIterator's ++.  startIndex is always
0 (the library's grids are never circular buffers).

A region is a tuple: ("line", x0, y0, x1, y1), ("circle", cx, cy, r), ("ellipse", cx, cy, lx, ly, rotation),
("polygon", ((x, y), ...)).

What is not the reference's:
 - a window index outside the buffer is brought back to the last cell (the reference ignores getIndexFromPosition's verdict);
 - a non-finite parameter or vertex, r < 0, an ellipse length not > 0: INVALID, nothing is iterated;
 - a line end whose walk into the map takes more than MAX_WALK steps: INVALID (the reference keeps walking);
 - a line whose constructor throws, an area without a member cell: EMPTY;
 - the circle's pow(radius, 2) is written r * r.
"""
import math
import sys

import numpy as np

from grid_sample_restate import Geometry, index_from_position, position_from_index    # noqa: F401  (GMM:130-172, restated there)

OK, EMPTY, INVALID = 0, 1, 2
LINE, CIRCLE, ELLIPSE, POLYGON = 0, 1, 2, 3
KIND = {"line": LINE, "circle": CIRCLE, "ellipse": ELLIPSE, "polygon": POLYGON}
MAX_WALK = 4096
MAX_VERTICES = 64
QNAN_BITS = 0x7fc00000
EPS = sys.float_info.epsilon
f32 = np.float32


def bound_position_to_range(g, p):                             # GMM:255-280
    out = []
    for a in range(2):
        shifted = p[a] - g.pos[a] + 0.5 * g.length[a]
        epsilon = 10.0 * EPS
        if abs(p[a]) > 1.0:
            epsilon *= abs(p[a])
        if shifted <= 0:
            shifted = epsilon
        elif shifted >= g.length[a]:
            shifted = g.length[a] - epsilon
        out.append(shifted + g.pos[a] - 0.5 * g.length[a])
    return tuple(out)


def corner_index(g, p):
    """boundPositionToRange, then getIndexFromPosition with its verdict ignored (findSubmapParameters of the three area
    iterators); the labelled deviation: an index outside the buffer is brought back to the last cell"""
    _, index = index_from_position(g, bound_position_to_range(g, p))
    return tuple(min(max(index[a], 0), g.size[a] - 1) for a in range(2))


def submap_cells(start, size):
    """SubmapIterator (IT/SubmapIterator.cpp, incrementIndexForSubmap GMM:485-516): the cells of the window in its order"""
    sub = [0, 0]
    while True:
        yield (start[0] + sub[0], start[1] + sub[1])
        if sub[1] + 1 < size[1]:
            sub[1] += 1
        else:
            sub[0] += 1
            sub[1] = 0
        if not (0 <= sub[0] < size[0] and 0 <= sub[1] < size[1]):
            return


def _finite(*v):
    return all(math.isfinite(x) for x in v)


def window(g, top_left, bottom_right):
    start, end = corner_index(g, top_left), corner_index(g, bottom_right)
    return start, (end[0] - start[0] + 1, end[1] - start[1] + 1)        # getSubmapSizeFromCornerIndices, GMM:343-349


def polygon_is_inside(vertices, point):                        # PG:30-42
    cross = 0
    n = len(vertices)
    j = n - 1
    for i in range(n):
        vi, vj = vertices[i], vertices[j]
        if (vi[1] > point[1]) != (vj[1] > point[1]) and point[0] < (vj[0] - vi[0]) * (point[1] - vi[1]) / (vj[1] - vi[1]) + vi[0]:
            cross += 1
        j = i
    return bool(cross % 2)


def limited_index(g, start, end):
    """getIndexLimitedToMapRange, IT/LineIterator.cpp:75-88 -> (status, index)"""
    v = (end[0] - start[0], end[1] - start[1])
    z = v[0] * v[0] + v[1] * v[1]                              # Eigen's normalized(): v / sqrt(v.v) when v.v > 0, else v
    if z > 0.0:
        n = math.sqrt(z)
        v = (v[0] / n, v[1] / n)
    step = g.res - EPS
    new = start
    k = 0
    while True:
        ok, index = index_from_position(g, new)
        if ok:
            return OK, index
        if k == MAX_WALK:
            return INVALID, None
        k += 1
        new = (new[0] + step * v[0], new[1] + step * v[1])
        r = (end[0] - new[0], end[1] - new[1])
        if math.sqrt(r[0] * r[0] + r[1] * r[1]) < step:
            return EMPTY, None


def line_cells(start, end):
    """LineIterator on two indices: initializeIterationParameters (IT/LineIterator.cpp:90-136) and the serial ++ (:43-55)"""
    delta = (abs(end[0] - start[0]), abs(end[1] - start[1]))
    inc1 = [1 if end[0] >= start[0] else -1, 1 if end[1] >= start[1] else -1]
    inc2 = list(inc1)
    if delta[0] >= delta[1]:
        inc1[0] = 0
        inc2[1] = 0
        denominator, numerator, numerator_add, n_cells = delta[0], delta[0] // 2, delta[1], delta[0] + 1
    else:
        inc2[0] = 0
        inc1[1] = 0
        denominator, numerator, numerator_add, n_cells = delta[1], delta[1] // 2, delta[0], delta[1] + 1
    index = [start[0], start[1]]
    cells = []
    i_cell = 0
    while i_cell < n_cells:                                    # for (; !isPastEnd(); ++iterator)
        cells.append((index[0], index[1]))
        numerator += numerator_add
        if numerator >= denominator:
            numerator -= denominator
            index[0] += inc1[0]
            index[1] += inc1[1]
        index[0] += inc2[0]
        index[1] += inc2[1]
        i_cell += 1
    return cells


def line_cell_closed_form(start, end, k):
    """cell k without the loop, as the kernels form it: k major steps and (denominator / 2 + k numeratorAdd) / denominator minor ones"""
    dr, dc = abs(end[0] - start[0]), abs(end[1] - start[1])
    sr, sc = (1 if end[0] >= start[0] else -1), (1 if end[1] >= start[1] else -1)
    den, add = (dr, dc) if dr >= dc else (dc, dr)
    m = (den // 2 + k * add) // den if den > 0 else 0
    return (start[0] + sr * k, start[1] + sc * m) if dr >= dc else (start[0] + sr * m, start[1] + sc * k)


def region_cells(g, region):
    """-> (status, cells in the iterator's order, their numbers in the order of the sum): the window's cells are numbered
    column-major (row fastest), a line's by their place on it"""
    kind = region[0]
    if kind == "line":
        x0, y0, x1, y1 = (float(v) for v in region[1:5])
        if not _finite(x0, y0, x1, y1):
            return INVALID, [], []
        s0, a = limited_index(g, (x0, y0), (x1, y1))
        if s0 != OK:                                           # (the second walk does not run: &&)
            return s0, [], []
        s1, b = limited_index(g, (x1, y1), (x0, y0))
        if s1 != OK:
            return s1, [], []
        cells = line_cells(a, b)
        return OK, cells, list(range(len(cells)))
    if kind == "circle":
        cx, cy, r = (float(v) for v in region[1:4])
        if not _finite(cx, cy, r) or r < 0.0:
            return INVALID, [], []
        start, size = window(g, (cx + r, cy + r), (cx - r, cy - r))            # IT/CircleIterator.cpp:74-85
        r2 = r * r

        def inside(p):                                         # :66-72
            dx, dy = p[0] - cx, p[1] - cy
            return dx * dx + dy * dy <= r2
    elif kind == "ellipse":
        cx, cy, lx, ly, rot = (float(v) for v in region[1:6])
        if not _finite(cx, cy, lx, ly, rot) or not (lx > 0.0 and ly > 0.0):
            return INVALID, [], []
        s, c = math.sin(rot), math.cos(rot)                    # IT/EllipseIterator.cpp:21-22
        sa = ((0.5 * lx) * (0.5 * lx), (0.5 * ly) * (0.5 * ly))
        # :82-97: Rotation2Dd * (lx, 0) and * (0, ly); the matrix is (c -s; s c) and the products with 0.0 add a zero
        u = (c * lx + (-s) * 0.0, s * lx + c * 0.0)
        v = (c * 0.0 + (-s) * ly, s * 0.0 + c * ly)
        half = (math.sqrt(u[0] * u[0] + v[0] * v[0]), math.sqrt(u[1] * u[1] + v[1] * v[1]))
        start, size = window(g, (cx + half[0], cy + half[1]), (cx - half[0], cy - half[1]))

        def inside(p):                                         # :74-80, transformMatrix_ = (c s; s -c)
            dx, dy = p[0] - cx, p[1] - cy
            t0, t1 = c * dx + s * dy, s * dx + (-c) * dy
            return t0 * t0 / sa[0] + t1 * t1 / sa[1] <= 1
    elif kind == "polygon":
        vertices = [(float(x), float(y)) for x, y in region[1]]
        assert 3 <= len(vertices) <= MAX_VERTICES
        if not all(_finite(x, y) for x, y in vertices):
            return INVALID, [], []
        top, bottom = list(vertices[0]), list(vertices[0])     # IT/PolygonIterator.cpp:71-85
        for vx in vertices:
            for a in range(2):
                top[a] = vx[a] if top[a] < vx[a] else top[a]
                bottom[a] = vx[a] if vx[a] < bottom[a] else bottom[a]
        start, size = window(g, tuple(top), tuple(bottom))

        def inside(p):
            return polygon_is_inside(vertices, p)
    else:
        raise ValueError(kind)
    cells, ranks = [], []
    for cell in submap_cells(start, size):
        if inside(position_from_index(g, cell)):
            cells.append(cell)
            ranks.append((cell[0] - start[0]) + (cell[1] - start[1]) * size[0])
    return (OK if cells else EMPTY), cells, ranks


def f2ord(bits):                                               # lio_f2ord: the words' order is the floats', -0.0 < +0.0
    return (~bits) & 0xffffffff if bits & 0x80000000 else bits | 0x80000000


def reduce_cells(layer, cells, ranks, threshold):
    """the reduction of include/liogpu.h over one region's cells on a [rows, cols] float32 layer ->
    (sum, min bits, max bits, n_finite, n_below)"""
    a = np.asarray(layer, f32)
    bits = a.view(np.uint32)
    thr = f32(threshold)
    part = [0.0] * 64
    lo = hi = None
    n_finite = n_below = 0
    for rank, (r, c) in sorted(zip(ranks, cells)):             # ascending number
        v = a[r, c]
        if not np.isfinite(v):
            continue
        part[rank % 64] = part[rank % 64] + float(v)
        o = f2ord(int(bits[r, c]))
        lo = o if lo is None or o < lo else lo
        hi = o if hi is None or o > hi else hi
        n_finite += 1
        n_below += 1 if v < thr else 0
    s = 32
    while s >= 1:
        for k in range(s):
            part[k] = part[k] + part[k + s]
        s //= 2

    def word(o):
        return QNAN_BITS if o is None else ((o & 0x7fffffff) if o & 0x80000000 else (~o) & 0xffffffff)
    return part[0], word(lo), word(hi), n_finite, n_below


def regions_reduce(g, layers, regions, threshold):
    """every output of lio_grid_region_reduce: stats as a [n_layers, n] structured array, n_cells, status"""
    n = len(regions)
    stat = np.zeros((len(layers), n), STAT_DTYPE)
    n_cells = np.zeros(n, np.int32)
    status = np.zeros(n, np.uint8)
    for q, region in enumerate(regions):
        st, cells, ranks = region_cells(g, region)
        status[q], n_cells[q] = st, len(cells)
        for k, layer in enumerate(layers):
            s, lo, hi, nf, nb = reduce_cells(layer, cells, ranks, threshold)
            stat[k, q] = (s, lo, hi, nf, nb)
    return stat, n_cells, status


def regions_cells(g, regions):
    """every output of lio_grid_region_cells: offsets, the cells' column-major linear indices, status"""
    offsets, lin, status = [0], [], []
    for region in regions:
        st, cells, _ = region_cells(g, region)
        status.append(st)
        lin += [c * g.size[0] + r for r, c in cells]
        offsets.append(len(lin))
    return np.asarray(offsets, np.int64), np.asarray(lin, np.int32), np.asarray(status, np.uint8)


# lio_grid_region_stat with min and max as their words
STAT_DTYPE = np.dtype([("sum", np.float64), ("min", np.uint32), ("max", np.uint32), ("n_finite", np.int32), ("n_below", np.int32)])


# ---- the regions the tests share
def lattice(g):
    """centres, radii, vertices and endpoints on cell centres, cell edges and map edges, and one step outside; every INVALID
    cause; lines with a single cell, equal deltas and the four sign combinations"""
    res = g.res
    hi = (g.pos[0] + 0.5 * g.length[0], g.pos[1] + 0.5 * g.length[1])
    lo = (g.pos[0] - 0.5 * g.length[0], g.pos[1] - 0.5 * g.length[1])
    ax = []
    for a in range(2):
        n = g.size[a]
        ks = sorted({0, 1, n // 2, n - 1, n})
        pts = [hi[a] + res, hi[a] + 0.3 * res]
        for k in ks:
            pts.append(hi[a] - k * res)                        # an edge
            if k < n:
                pts.append(hi[a] - (k + 0.5) * res)            # a centre
        pts += [lo[a] - 0.3 * res, lo[a] - res]
        ax.append(pts)
    pts = [(x, y) for x in ax[0][::2] for y in ax[1][1::2]] + [(x, y) for x in ax[0][1::3] for y in ax[1][::3]]
    out = []
    radii = (0.0, 0.5 * res, res, 1.5 * res, 2.5 * res + 1e-9)
    for k, (x, y) in enumerate(pts):
        out.append(("circle", x, y, radii[k % len(radii)]))
        out.append(("ellipse", x, y, (1 + k % 4) * res, (0.5 + k % 3) * res, 0.4 * (k % 8) - 1.0))
        x1, y1 = pts[(7 * k + 3) % len(pts)]
        out.append(("line", x, y, x1, y1))
        w, h = (0.5 + k % 3) * res, (1 + k % 2) * res
        out.append(("polygon", ((x + w, y + h), (x + w, y - h), (x - w, y - h), (x - w, y + h))))
        out.append(("polygon", ((x, y), (x + 2 * w, y - 0.5 * h), (x + 0.5 * w, y - 2 * h))))
    cx, cy = g.pos
    # lines: one cell, equal deltas, the four sign combinations (shallow and steep)
    out.append(("line", cx, cy, cx, cy))
    out.append(("line", cx + 0.1 * res, cy + 0.1 * res, cx + 0.2 * res, cy + 0.15 * res))
    for sx in (1, -1):
        for sy in (1, -1):
            out.append(("line", cx, cy, cx + sx * 2.0 * res, cy + sy * 2.0 * res))
            out.append(("line", cx, cy, cx + sx * 3.0 * res, cy + sy * 1.0 * res))
            out.append(("line", cx, cy, cx + sx * 1.0 * res, cy + sy * 3.0 * res))
            out.append(("line", cx - sx * 40.0 * res, cy - sy * 90.0 * res, cx + sx * 35.0 * res, cy + sy * 80.0 * res))
    # a concave polygon, one with a repeated vertex, one covering everything, one far outside
    out.append(("polygon", ((cx + 2 * res, cy + 2 * res), (cx, cy + 0.3 * res), (cx - 2 * res, cy + 2 * res), (cx - 2 * res, cy - 2 * res), (cx + 2 * res, cy - 2 * res))))
    out.append(("polygon", ((cx, cy), (cx, cy), (cx + res, cy - res), (cx - res, cy - res))))
    out.append(("polygon", ((hi[0] + res, hi[1] + res), (lo[0] - res, hi[1] + res), (lo[0] - res, lo[1] - res), (hi[0] + res, lo[1] - res))))
    out.append(("polygon", ((hi[0] + 5 * res, hi[1] + 5 * res), (hi[0] + 9 * res, hi[1] + 5 * res), (hi[0] + 7 * res, hi[1] + 8 * res))))
    out.append(("circle", cx, cy, 1e3 * res))
    out.append(("ellipse", cx, cy, 1e3 * res, 1e3 * res, 0.3))
    out.append(("circle", hi[0] + 50 * res, cy, 2 * res))
    # every INVALID cause
    nan, inf = float("nan"), float("inf")
    out += [("circle", nan, cy, res), ("circle", cx, inf, res), ("circle", cx, cy, nan), ("circle", cx, cy, -res), ("circle", cx, cy, inf),
            ("ellipse", cx, cy, 0.0, res, 0.0), ("ellipse", cx, cy, res, -res, 0.0), ("ellipse", cx, cy, res, res, inf), ("ellipse", cx, -inf, res, res, 0.0),
            ("ellipse", cx, cy, nan, res, 0.0),
            ("polygon", ((cx, cy), (nan, cy), (cx, cy + res))), ("polygon", ((cx, cy), (cx + res, cy), (cx, -inf))),
            ("line", nan, cy, cx, cy), ("line", cx, cy, cx, inf),
            ("line", hi[0] + (MAX_WALK + 10) * res, cy, cx, cy),                       # the walk's cap, first end
            ("line", cx, cy, cx, lo[1] - (MAX_WALK + 10) * res),                       # ... second end
            ("line", hi[0] + (MAX_WALK - 10) * res, cy, cx, cy)]                       # just inside the cap: OK
    return out


def exact_windows(g):
    """circles-free windows of exactly 64, 65, 256 and 257 cells (polygons that cover them whole), where the grid has room"""
    out = []
    for h, w in ((8, 8), (64, 1), (5, 13), (65, 1), (16, 16), (64, 4), (1, 257), (257, 1)):
        if h > g.size[0] or w > g.size[1]:
            continue
        top = (g.pos[0] + 0.5 * g.length[0] - 0.25 * g.res, g.pos[1] + 0.5 * g.length[1] - 0.25 * g.res)
        bot = (top[0] - (h - 1) * g.res - 0.5 * g.res, top[1] - (w - 1) * g.res - 0.5 * g.res)
        out.append(("polygon", ((top[0], top[1]), (bot[0], top[1]), (bot[0], bot[1]), (top[0], bot[1]))))
    return out


def random_regions(g, n, seed):
    rng = np.random.default_rng(seed)
    res = g.res
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 4))
        x = g.pos[0] + (rng.random() - 0.5) * 1.2 * g.length[0]
        y = g.pos[1] + (rng.random() - 0.5) * 1.2 * g.length[1]
        if k == LINE:
            out.append(("line", x, y, g.pos[0] + (rng.random() - 0.5) * 1.2 * g.length[0], g.pos[1] + (rng.random() - 0.5) * 1.2 * g.length[1]))
        elif k == CIRCLE:
            out.append(("circle", x, y, rng.random() * 6 * res))
        elif k == ELLIPSE:
            out.append(("ellipse", x, y, (0.2 + rng.random() * 10) * res, (0.2 + rng.random() * 6) * res, (rng.random() - 0.5) * 7.0))
        else:
            nv = int(rng.integers(3, 9))
            ang = np.sort(rng.random(nv) * 2 * math.pi)
            rad = (0.5 + rng.random(nv) * 5) * res
            out.append(("polygon", tuple((x + float(r * math.cos(a)), y + float(r * math.sin(a))) for a, r in zip(ang, rad))))
    return out


def make_layer(rows, cols, holes, seed=1):
    """a [rows, cols] float32 layer in [0, 1) with, when `holes`, 20 % NaN, some infinities, and -0.0 beside +0.0"""
    rng = np.random.default_rng(seed)
    a = rng.random((rows, cols)).astype(f32)
    if holes:
        a[rng.random((rows, cols)) < 0.2] = np.nan
        flat = a.reshape(-1)
        flat[::11] = np.inf
        flat[5::13] = -np.inf
        flat[3::7] = -0.0
        flat[4::7] = 0.0
    return a
