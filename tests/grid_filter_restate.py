"""numpy restatement of the filters behind lio_grid_filter_radius / _window / _curvature / _threshold:
grid_map_filters' MinInRadiusFilter, MeanInRadiusFilter, SlidingWindowMathExpressionFilter over grid_map_core's
SlidingWindowIterator, CurvatureFilter and ThresholdFilter, restated from their source text.  Python floats are IEEE doubles
and numpy's float32 scalars round after every operation, so each line is one rounded operation in the order the reference
performs it.  Plain serial loops in the reference's visiting order: the grids of the tests are small.  The circle's geometry is
tests/terrain_restate.py's (pinned by tests/test_terrain_cpu.py).  tests/test_grid_filter_cpu.py pins this file.

Every filter returns (layer [rows, cols] float32, counts): the layer starts as mapOut.add(output_layer) leaves it, all
0x7fc00000; counts = dict(n_visited, n_written, n_changed, mask), mask the cells that received a value."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_restate as T                                    # noqa: E402

f32 = np.float32
QNAN_BITS = 0x7FC00000
MIN, MEAN = 0, 1                                               # LIO_GF_*
INSIDE, CROP, EMPTY, EDGE_MEAN = 0, 1, 2, 3                     # SlidingWindowIterator::EdgeHandling
SUM, MEAN_OF_FINITES, MIN_OF_FINITES, MAX_OF_FINITES, NUMBER_OF_FINITES, STDDEV, WEIGHTED_SUM = range(7)
MAX_CELLS = 32                                                 # LIO_TILE_MAX_REACH


class Refused(ValueError):
    """what the library answers with LIO_ERR_ARG"""


def new_layer(shape):
    """GridMap::add(layer): NAN, the word 0x7fc00000"""
    return np.full(shape, QNAN_BITS, np.uint32).view(f32)


def _counts(visited=0, written=0, changed=0, mask=None):
    """mask: the cells that received a value (every other cell must hold exactly 0x7fc00000)"""
    return dict(n_visited=int(visited), n_written=int(written), n_changed=int(changed), mask=mask)


# ---- MinInRadiusFilter.cpp:50-93, MeanInRadiusFilter.cpp:51-82
def radius_filter(grid, resolution, position, op, radius, less=None, valid=np.isfinite):
    """less / valid: what a variant of the restatement replaces (tests/test_grid_filter_cpu.py)"""
    grid = np.asarray(grid, f32)
    if not math.isfinite(radius) or radius < 0.0:
        raise Refused("radius must be finite and not negative")
    if not radius / resolution <= MAX_CELLS:
        raise Refused("the radius reaches further than 32 cells")
    G = T.Geom(grid.shape[0], grid.shape[1], resolution, position)
    out = new_layer(grid.shape)
    mask = np.zeros(grid.shape, bool)
    visited = 0
    for lin in range(G.rows * G.cols):                         # GridMapIterator: the column-major linear index
        r, c = lin % G.rows, lin // G.rows
        if op == MIN:
            if not valid(grid[r, c]):
                continue
            visited += 1
            init, lowest = False, 0.0
            for i, j in T.circle(G, r, c, radius):
                if not valid(grid[i, j]):
                    continue
                value = float(grid[i, j])                      # double value = mapOut.at(...)
                if not init:
                    lowest, init = value, True
                    continue
                if (value < lowest) if less is None else less(value, lowest):
                    lowest = value
            if init:
                out[r, c] = f32(lowest)
                mask[r, c] = True
        else:
            visited += 1
            s, n = 0.0, 0
            for i, j in T.circle(G, r, c, radius):
                if not valid(grid[i, j]):
                    continue
                s += float(grid[i, j])
                n += 1
            if n != 0:
                out[r, c] = f32(s / n)
                mask[r, c] = True
    return out, _counts(visited, mask.sum(), 0, mask)


# ---- grid_map_core/eigen_plugins: FunctorsPlugin.hpp, DenseBasePlugin.hpp, on float32
def sum_of_finites_op(a, b):
    fa, fb = np.isfinite(a), np.isfinite(b)
    if fa and fb:
        return a + b
    if fa:
        return a
    if fb:
        return b
    return a + b


def _std_min(a, b):
    return b if b < a else a                                   # std::min


def _std_max(a, b):
    return b if a < b else a                                   # std::max


def min_of_finites_op(a, b):
    fa, fb = np.isfinite(a), np.isfinite(b)
    if fa and fb:
        return _std_min(a, b)
    if fa:
        return a
    if fb:
        return b
    return _std_min(a, b)


def max_of_finites_op(a, b):
    fa, fb = np.isfinite(a), np.isfinite(b)
    if fa and fb:
        return _std_max(a, b)
    if fa:
        return a
    if fb:
        return b
    return _std_max(a, b)


def redux(block, op, order="F"):
    """Eigen's default-traversal redux with a functor that has no packet form: serial, column-major, the first coefficient
    initialises"""
    flat = np.asarray(block, f32).ravel(order=order)
    acc = flat[0]
    for v in flat[1:]:
        acc = op(acc, v)
    return f32(acc)


def number_of_finites(block, count=lambda b: b == b):
    return f32(np.count_nonzero(count(np.asarray(block, f32))))


def mean_of_finites(block, order="F", count=lambda b: b == b):
    return f32(redux(block, sum_of_finites_op, order) / number_of_finites(block, count))


# ---- SlidingWindowIterator.cpp
class SlidingWindowIterator:
    """GridMapIterator's linear index with SlidingWindowIterator's setup(), operator++, dataInsideMap() and getData()"""

    def __init__(self, data, edge, window_size=3):
        self.data = np.asarray(data, f32)
        self.rows, self.cols = self.data.shape
        self.linear_size = self.rows * self.cols
        self.lin, self.past_end = 0, False
        self.edge = edge
        self.window_size = int(window_size)
        self.setup()

    def set_window_length(self, length, resolution):
        self.window_size = int(math.floor(length / resolution + 0.5))      # static_cast<size_t>(std::round(.)) of a non-negative number
        if self.window_size % 2 != 1:
            self.window_size += 1
        self.setup()

    def setup(self):
        if self.window_size % 2 == 0:
            raise Refused("SlidingWindowIterator has a wrong window size!")
        self.margin = (self.window_size - 1) // 2
        if self.edge == INSIDE and not self.data_inside_map():
            self.increment()

    def index(self):
        return self.lin % self.rows, self.lin // self.rows      # getIndexFromLinearIndex

    def _base_increment(self):
        if self.lin + 1 < self.linear_size:
            self.lin += 1
        else:
            self.past_end = True

    def increment(self):
        if self.edge == INSIDE:
            while not self.past_end:
                self._base_increment()
                if self.data_inside_map():
                    break
        else:
            self._base_increment()

    def data_inside_map(self):
        r, c = self.index()
        m = self.margin
        return r - m >= 0 and c - m >= 0 and r - m < self.rows and c - m < self.cols and r + m >= 0 and c + m >= 0 and r + m < self.rows and c + m < self.cols

    def get_data(self, order="F"):
        r, c = self.index()
        m = self.margin
        o0, o1 = r - m, c - m                                  # originalTopLeftIndex
        t0, t1 = min(max(o0, 0), self.rows - 1), min(max(o1, 0), self.cols - 1)            # boundIndexToRange
        b0, b1 = min(max(r + m, 0), self.rows - 1), min(max(c + m, 0), self.cols - 1)
        block = self.data[t0:b0 + 1, t1:b1 + 1]
        if self.edge in (INSIDE, CROP):
            return block.copy()
        w = self.window_size
        ret = new_layer((w, w))                                # setConstant(NAN)
        if self.edge == EDGE_MEAN:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                ret[:] = mean_of_finites(block, order)
        ret[t0 - o0:t0 - o0 + block.shape[0], t1 - o1:t1 - o1 + block.shape[1]] = block
        return ret


def window_size_of(resolution, window_size, window_length):
    """the size the filter ends with, and the refusals that need no grid"""
    if window_size < 0 or (window_size != 0 and window_size % 2 == 0):
        raise Refused("window_size must be odd")
    if not math.isfinite(window_length) or window_length < 0.0:
        raise Refused("window_length must be finite and not negative")
    if window_size == 0:
        cells = math.floor(window_length / resolution + 0.5)
        if not cells <= 2 * MAX_CELLS + 1:
            raise Refused("the window reaches further than 32 cells")
        window_size = int(cells) + (0 if int(cells) % 2 == 1 else 1)
    if (window_size - 1) // 2 > MAX_CELLS:
        raise Refused("the window reaches further than 32 cells")
    return window_size


def evaluate(W, op, K=None, order="F", count=lambda b: b == b):
    """the expression on one window matrix -> float32"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if op == SUM:
            return redux(W, sum_of_finites_op, order)
        if op == MEAN_OF_FINITES:
            return mean_of_finites(W, order, count)
        if op == MIN_OF_FINITES:
            return redux(W, min_of_finites_op, order)
        if op == MAX_OF_FINITES:
            return redux(W, max_of_finites_op, order)
        if op == NUMBER_OF_FINITES:
            return number_of_finites(W, count)
        if op == STDDEV:                                       # sqrt(sumOfFinites(square(W - meanOfFinites(W))) ./ numberOfFinites(W))
            d = W - mean_of_finites(W, order, count)
            return f32(np.sqrt(f32(redux(d * d, sum_of_finites_op, order) / number_of_finites(W, count))))
        if op == WEIGHTED_SUM:                                 # sumOfFinites(K .* W): EigenLab.h:1291-1304, sizes must agree
            if K.shape != W.shape:
                raise Refused("the window and the weights disagree in size")
            return redux(K * W, sum_of_finites_op, order)
    raise Refused("op")


def window_filter(grid, resolution, op, edge, window_size=0, window_length=0.0, weights=None, order="F", count=lambda b: b == b, double_setup=True):
    """SlidingWindowMathExpressionFilter::update.  weights: [size, size] float32, K[a, b] against W[a, b].  order, count,
    double_setup: what a variant of the restatement replaces."""
    grid = np.asarray(grid, f32)
    if op not in range(7) or edge not in range(4):
        raise Refused("op or edge_handling out of range")
    if (op == WEIGHTED_SUM) != (weights is not None):
        raise Refused("weights")
    size = window_size_of(resolution, window_size, window_length)
    K = None if weights is None else np.asarray(weights, f32).reshape(size, size)
    if op == WEIGHTED_SUM and edge == CROP and size > 1:
        raise Refused("with crop the window and the weights disagree in size at the border")
    if window_size != 0:
        it = SlidingWindowIterator(grid, edge, window_size)
    elif double_setup:
        it = SlidingWindowIterator(grid, edge)                 # windowSize_(3), the filter's constructor default
        it.set_window_length(window_length, resolution)
    else:
        it = SlidingWindowIterator(grid, edge, size)
    out = new_layer(grid.shape)
    mask = np.zeros(grid.shape, bool)
    while not it.past_end:
        r, c = it.index()
        out[r, c] = evaluate(it.get_data(order), op, K, order, count)
        mask[r, c] = True
        it.increment()
    return out, _counts(mask.sum(), mask.sum(), 0, mask), size


# ---- CurvatureFilter.cpp:39-68
def curvature_filter(grid, resolution):
    grid = np.asarray(grid, f32)
    rows, cols = grid.shape
    out = new_layer(grid.shape)
    L2 = f32(resolution * resolution)
    mask = np.zeros(grid.shape, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(cols):
            for i in range(rows):
                if not np.isfinite(grid[i, j]):
                    continue
                z = float(grid[i, j])
                D = f32((float(grid[i, j if j == 0 else j - 1] + grid[i, j if j == cols - 1 else j + 1]) / 2.0 - z) / float(L2))
                E = f32((float(grid[i if i == 0 else i - 1, j] + grid[i if i == rows - 1 else i + 1, j]) / 2.0 - z) / float(L2))
                if not np.isfinite(D):
                    D = f32(0.0)
                if not np.isfinite(E):
                    E = f32(0.0)
                out[i, j] = f32(-2.0 * float(D + E))
                mask[i, j] = True
    return out, _counts(rows * cols, mask.sum(), 0, mask)


# ---- ThresholdFilter.cpp:62-92
def threshold_filter(condition, data, upper, threshold, set_to):
    """-> (data afterwards, counts); `data` may be `condition` itself"""
    condition, out = np.asarray(condition, f32), np.array(data, f32)
    word = np.array([set_to], np.float64).astype(f32).view(np.uint32)[0]
    bits = out.view(np.uint32)
    changed = 0
    for lin in range(condition.size):
        r, c = lin % condition.shape[0], lin // condition.shape[0]
        v = float(condition[r, c])
        if (not v <= threshold) if upper else (not v >= threshold):
            bits[r, c] = word
            changed += 1
    return out, _counts(condition.size, changed, changed)


def identical(got, want, mask=None):
    """the comparison rule: the same NaN mask, every other word equal; outside `mask` (the cells that received a value)
    exactly 0x7fc00000"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    if got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    same = bool(np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw]))
    return same and (mask is None or bool((got.view(np.uint32)[~mask] == QNAN_BITS).all()))
