"""Scalar restatement of grid_map::GridMap::getTransformedMap (GM = grid_map_core/src/GridMap.cpp:332-436) and of
GridMapRosConverter::toOccupancyGrid / fromOccupancyGrid (GridMapRosConverter.cpp:283-365), written from the reference text,
as include/liogpu.h lio_grid_transform and lio_grid_to_occupancy state them.  Python floats are IEEE doubles and nothing here
fuses a multiply with an add, so every operation is the fp64 operation the reference writes, in its order; a stored height is a
float32, widened to double where the reference compares it with one.  The geometry helpers are tests/grid_sample_restate.py's.

Three things: the serial loop cell by cell (`serial`), the order-independent winner rule the library runs (`by_rule`), and the
occupancy conversion.  What is not the reference's:
 - transform * p is ((R_i0 x + R_i1 y) + R_i2 z) + t_i per component (Eigen's order inside the product is not defined by the
   source: unpinned);
 - a new size below 1 raises ValueError, where the reference asserts.
"""
import math

import numpy as np

import grid_sample_restate as gs

QNAN_BITS = 0x7fc00000
f32, u32 = np.float32, np.uint32


def apply(T, i, x, y, z):
    """component i of transform * (x, y, z); T: 3 rows of [R | t]"""
    return ((T[i][0] * x + T[i][1] * y) + T[i][2] * z) + T[i][3]


def as_rows(transform):
    t = np.asarray(transform, np.float64).reshape(-1, 4)[:3]
    return [[float(v) for v in row] for row in t]


def c_round(v):
    """round(): halves away from zero"""
    a = abs(v)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1.0
    return math.copysign(r, v)


def new_geometry(g, T):
    """GM:347-382 -> the new map's gs.Geometry (setGeometry: size = (int)round(length / resolution))"""
    hx, hy = g.length[0] * 0.5, g.length[1] * 0.5
    corners = ((g.pos[0] + hx, g.pos[1] + hy), (g.pos[0] + hx, g.pos[1] - hy), (g.pos[0] - hx, g.pos[1] + hy), (g.pos[0] - hx, g.pos[1] - hy))
    edges = [(apply(T, 0, x, y, 0.0), apply(T, 1, x, y, 0.0)) for x, y in corners]
    centre, length = [], []
    for a in range(2):
        c = 0.0
        for e in edges:
            c += e[a]
        c *= 0.25
        m = 0.0
        for e in edges:
            m = math.fabs(e[a] - c) if math.fabs(e[a] - c) > m else m          # fmax on finite values
        centre.append(c)
        length.append(2.0 * m)
    size = [c_round(length[a] / g.res) for a in range(2)]
    if not all(math.isfinite(s) and s >= 1.0 for s in size):
        raise ValueError("the new map has no cell along an axis")
    return gs.Geometry(int(size[0]), int(size[1]), g.res, centre)


def samples_of(g, r, c, sample_length, n_samples):
    """GM:394-403: the positions (x, y) of a cell's samples, in order"""
    cx, cy = gs.position_from_index(g, (r, c))
    five = ((cx, cy), (cx - sample_length, cy), (cx + sample_length, cy), (cx, cy - sample_length), (cx, cy + sample_length))
    return five[:n_samples]


def visits(g, height, T, ratio, ng):
    """The loop of GM:385-412 up to the rule, in visit order: (visit number, source linear index, new (row, col), z) of every
    sample that lands in the new map; and the counts (source cells with a finite height, samples outside)."""
    rows, cols = g.size
    sample_length = g.res * ratio
    n_samples = 5 if ratio > 0.0 else 1
    out, n_source, n_outside = [], 0, 0
    for lin in range(rows * cols):                               # GridMapIterator: column-major linear index ascending
        r, c = lin % rows, lin // rows
        h = height[r, c]
        if not np.isfinite(h):                                   # getPosition3, GM:260-270
            continue
        n_source += 1
        z0 = float(h)
        for s, (x, y) in enumerate(samples_of(g, r, c, sample_length, n_samples)):
            tx, ty, tz = apply(T, 0, x, y, z0), apply(T, 1, x, y, z0), apply(T, 2, x, y, z0)
            ok, index = gs.index_from_position(ng, (tx, ty))
            if not ok:
                n_outside += 1
                continue
            out.append((5 * lin + s, lin, index, tz))
    return out, n_source, n_outside


class Result:
    def __init__(self, ng, n_layers):
        self.g = ng
        self.words = np.full((n_layers,) + tuple(ng.size), QNAN_BITS, u32)     # new cells nothing reaches: the quiet NaN
        self.winner = np.full(ng.size, -1, np.int64)             # the visit number whose values the cell holds
        self.n_source_cells = self.n_samples_outside = self.n_cells_written = 0

    @property
    def layers(self):
        return self.words.view(f32)

    def counters(self):
        return (self.n_source_cells, self.n_samples_outside, self.n_cells_written)


def _words(layers):
    a = np.ascontiguousarray(np.asarray(layers, f32))
    assert a.ndim == 3
    return a.view(u32)


def _store(res, src_words, height_layer, visit, lin, index, z, rows):
    r, c = lin % rows, lin // rows
    res.words[:, index[0], index[1]] = src_words[:, r, c]       # every other layer: the source cell's bits
    res.words[height_layer, index[0], index[1]] = np.array(z, np.float64).astype(f32).view(u32)
    res.winner[index] = visit


def serial(g, layers, transform, height_layer, ratio):
    """getTransformedMap as written: layers [n, rows, cols] float32 -> Result"""
    T = as_rows(transform)
    src = _words(layers)
    ng = new_geometry(g, T)
    res = Result(ng, len(src))
    seq, res.n_source_cells, res.n_samples_outside = visits(g, src[height_layer].view(f32), T, ratio, ng)
    new_h = res.words[height_layer].view(f32)
    with np.errstate(over="ignore"):
        for visit, lin, index, z in seq:
            existing = new_h[index]
            if not np.isnan(existing) and float(existing) > z:   # GM:416-419: a float against a double
                continue
            _store(res, src, height_layer, visit, lin, index, z, g.size[0])
    res.n_cells_written = int((res.winner >= 0).sum())
    return res


def rule_winner(cands):
    """cands: [(visit, z)] of one new cell -> (the winning visit, its z, whether the `last of z >= F` branch chose it).
    F = the largest (float)z; the winner is the largest visit among (float)z == F and z >= (double)F, and where there is none
    the smallest visit among (float)z == F."""
    with np.errstate(over="ignore"):
        fz = [f32(z) for _, z in cands]
    F = max(fz)
    high = [(v, z) for (v, z), f in zip(cands, fz) if f == F and z >= float(F)]
    if high:
        return max(high) + (True,)
    return min((v, z) for (v, z), f in zip(cands, fz) if f == F) + (False,)


def by_rule(g, layers, transform, height_layer, ratio):
    """the same map by the order-independent rule -> Result, with .branch [rows, cols]: 1 where the `last of z >= F` branch
    chose the winner, 0 where the `first of the class` branch did, -1 where nothing landed"""
    T = as_rows(transform)
    src = _words(layers)
    ng = new_geometry(g, T)
    res = Result(ng, len(src))
    res.branch = np.full(ng.size, -1, np.int8)
    seq, res.n_source_cells, res.n_samples_outside = visits(g, src[height_layer].view(f32), T, ratio, ng)
    cells = {}
    for visit, lin, index, z in reversed(seq):                   # (any order gives the same result: reversed, to show it)
        cells.setdefault(index, []).append((visit, z))
    with np.errstate(over="ignore"):
        for index, cands in cells.items():
            visit, z, high = rule_winner(cands)
            _store(res, src, height_layer, visit, visit // 5, index, z, g.size[0])
            res.branch[index] = 1 if high else 0
    res.n_cells_written = len(cells)
    return res


# ---- GridMapRosConverter
def to_occupancy(g, layer, data_min, data_max):
    """toOccupancyGrid (:329-365) in float, as written -> (data [rows * cols] int8, width, height, resolution (float32),
    origin (x, y))"""
    v = np.asarray(layer, f32)
    lo, hi = f32(data_min), f32(data_max)
    with np.errstate(all="ignore"):
        value = (v - lo) / (hi - lo)
        clamped = np.where(f32(0.0) < value, value, f32(0.0)).astype(f32)          # max(0.0f, value)
        clamped = np.where(f32(1.0) < clamped, f32(1.0), clamped).astype(f32)      # min(.., 1.0f)
        cell = np.where(np.isnan(value), f32(-1.0), f32(0.0) + clamped * f32(100.0)).astype(f32)
    assert cell.dtype == f32 and value.dtype == f32
    data = np.trunc(cell).astype(np.int8).ravel(order="F")[::-1].copy()            # data[n - 1 - (col * rows + row)]
    origin = tuple(g.pos[a] - 0.5 * g.length[a] for a in range(2))
    return data, g.size[0], g.size[1], f32(g.res), origin


def from_occupancy(data, width, height):
    """fromOccupancyGrid's cells (:316-323): data(i) = the i-th cell from the end, -1 -> NaN -> [width, height] float32"""
    d = np.asarray(data, np.int8)[::-1].astype(f32)
    d[np.asarray(data, np.int8)[::-1] == -1] = np.nan
    return d.reshape((width, height), order="F")
