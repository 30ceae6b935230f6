"""Designed inputs of the layer filters (lio_grid_filter_*), as builders: what tests/test_grid_filter_cpu.py shows to bite
on the restatement and tests/test_gpu_grid_filter.py runs through the C ABI.  Every grid is tiny: the restatement loops over
cells in Python."""
import numpy as np

import grid_filter_restate as R

f32 = np.float32
FLT_MAX = np.finfo(f32).max
# 1 x 1, a single row across 38 tiles, 2 x 2, one cell past a 32 x 8 tile on both axes, three tiles each way, and the 8 x 5
# grid of the reference's SlidingWindowIteratorTest.cpp
SHAPES = ((1, 1), (1, 300), (2, 2), (33, 9), (69, 19), (8, 5))
POSITIONS = ((0.0, 0.0), (1e4, -3e4))
RES = 0.1                                                      # not a binary fraction: the centres round
RES_BINARY = 0.25                                              # radius / resolution is exact: 32 cells are 32 cells


def plane(rows, cols, seed=3, holes=True):
    """a tilted plane with 0.01 noise, 8 % random holes and (where it fits) one 4 x 5 hole"""
    rng = np.random.default_rng(seed)
    z = 0.08 * np.arange(rows)[:, None] - 0.05 * np.arange(cols)[None, :] + rng.normal(0, 0.01, (rows, cols))
    if holes:
        z[rng.uniform(size=z.shape) < 0.08] = np.nan
        if rows >= 12 and cols >= 9:
            z[6:10, 2:7] = np.nan
    return z.astype(f32)


def all_nan(rows, cols):
    return R.new_layer((rows, cols)).copy()


def with_inf(rows, cols, seed=4):
    """the plane with +inf and -inf cells among the values, and a corner block that holds nothing finite: NaN first in
    column-major order, then infinities of both signs (the functors' last branch)"""
    z = plane(rows, cols, seed)
    rng = np.random.default_rng(seed + 100)
    u = rng.uniform(size=z.shape)
    z[u < 0.05] = np.inf
    z[u > 0.95] = -np.inf
    if rows >= 5 and cols >= 4:
        z[:5, :4] = np.nan
        z[1, 0], z[2, 0], z[0, 1], z[3, 2] = np.inf, -np.inf, np.inf, np.inf
    return z.astype(f32)


def zero_pairs(rows=5, cols=4):
    """ones with +0 at (0, 1) and -0 at (1, 0), and the same pair mirrored lower down: the circle's order (row index outer)
    meets +0 first, the window's column-major order meets -0 first"""
    z = np.ones((rows, cols), f32)
    z[0, 1], z[1, 0] = 0.0, -0.0
    if rows >= 5 and cols >= 4:
        z[3, 3], z[4, 2] = -0.0, 0.0
    return z


def near_flt_max(rows=6, cols=5):
    """values whose neighbour sum overflows (curvature's D or E becomes infinite and is zeroed) beside ordinary ones"""
    z = plane(rows, cols, seed=9, holes=False)
    z[1, 1], z[1, 3] = FLT_MAX, FLT_MAX                         # left + right of (1, 2) overflows
    z[3, 2], z[5, 2] = -FLT_MAX, -FLT_MAX                       # up + down of (4, 2)
    z[0, 0] = FLT_MAX                                           # a border cell that replaces its missing neighbours
    return z.astype(f32)


def iterator_grid(seed=8):
    """the 8 x 5 map of SlidingWindowIteratorTest.cpp (setRandom: values in [-1, 1])"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (8, 5)).astype(f32)


def threshold_case():
    """threshold_filter_test.cpp: 20 x 20 at 0.02, 0.03 everywhere, 0.06 in the bottom-right 5 x 5, NaN in the top-left 3 x 3;
    the output layer ones -> (condition, data, expected)"""
    cond = np.full((20, 20), 0.03, f32)
    cond[-5:, -5:] = 0.06
    cond[:3, :3] = np.nan
    data = np.ones((20, 20), f32)
    want = data.copy()
    want[:3, :3] = np.nan
    want[-5:, -5:] = np.nan
    return cond, data, want


# radii in cells: the cell alone, half a cell, exact multiples of the resolution (membership decided by the rounding of the
# centres), 3.3 cells
RADII_CELLS = (0.0, 0.5, 1.0, 2.0, 3.0, 3.3)
RADIUS_MAX_CELLS, RADIUS_REFUSED_CELLS = 32.0, 32.5            # on a grid of at most 40 x 9, at RES_BINARY
SHAPE_MAX_RADIUS = (40, 9)
WINDOW_SIZES = (1, 3, 5)
WINDOW_SIZE_MAX = 65
LENGTHS_DERIVING = ((0.0, 1), (0.1, 1), (0.2, 3), (0.25, 3))    # window_length at RES -> the size setWindowLength derives
KERNEL_EDGE = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], f32)          # filters_demo_filter_chain.yaml:97
KERNEL_SHARPEN = np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], f32)    # :98


def weights_for(size, seed=12):
    """size x size weights with every kind of word among them: zeros of both signs, an infinity and a NaN beside ordinary
    values (any weight bits are allowed)"""
    k = np.random.default_rng(seed + size).uniform(-2.0, 2.0, (size, size)).astype(f32)
    if size >= 3:
        k[0, 0], k[1, 0], k[0, 1], k[2, 2] = 0.0, -0.0, np.inf, np.nan
    return k


def contents(rows, cols):
    """name -> grid, the contents every filter is run on at this shape"""
    out = {"plane": plane(rows, cols), "all_nan": all_nan(rows, cols), "inf": with_inf(rows, cols)}
    if rows >= 5 and cols >= 4:
        out["zeros"] = zero_pairs(rows, cols)
    if rows >= 6 and cols >= 5:
        out["flt_max"] = near_flt_max(rows, cols)
    return out


# ---- the cases both the host run of the header (tests/test_grid_filter_cpu.py) and the device (tests/test_gpu_grid_filter.py)
# are held to, grouped by shape so that one group stays within seconds.  A case is (kind, key, arguments); its grid is
# grid_of(key), its expectation expected(case), computed once a process and shared.
def grid_of(key):
    name, rows, cols = key
    return contents(rows, cols)[name]


def radius_cases(shape):
    rows, cols = shape
    out = []
    for pi, pos in enumerate(POSITIONS):
        for name in ("plane", "inf") if pi == 0 or rows * cols <= 400 else ("inf",):
            for cells in RADII_CELLS:
                for op in (R.MIN, R.MEAN):
                    out.append(("radius", (name, rows, cols), (RES, pos, op, cells * RES)))
    for name in ("all_nan", "zeros", "flt_max"):
        if name in contents(rows, cols):
            for cells in (1.0, 3.3):
                for op in (R.MIN, R.MEAN):
                    out.append(("radius", (name, rows, cols), (RES if name != "zeros" else 1.0, POSITIONS[0], op, cells * (RES if name != "zeros" else 1.0))))
    return out


def radius_max_cases():
    rows, cols = SHAPE_MAX_RADIUS
    return [("radius", ("inf", rows, cols), (RES_BINARY, pos, op, RADIUS_MAX_CELLS * RES_BINARY)) for pos in POSITIONS for op in (R.MIN, R.MEAN)]


def window_cases(shape, edge):
    rows, cols = shape
    names = ["inf"] + (["plane", "zeros", "all_nan"] if rows * cols <= 400 else [])
    out = []
    for name in names:
        if name not in contents(rows, cols):
            continue
        for op in range(7):
            sizes = [(s, 0.0) for s in (WINDOW_SIZES if rows * cols <= 400 else WINDOW_SIZES[1:])]
            if name == "inf":
                sizes += [(0, length) for length, _ in LENGTHS_DERIVING]
            for size, length in sizes:
                derived = size or dict(LENGTHS_DERIVING)[length]
                if op == R.WEIGHTED_SUM and edge == R.CROP and derived > 1:
                    continue                                   # refused: tests/test_gpu_grid_filter.py::test_refusals
                weights = None
                if op == R.WEIGHTED_SUM:
                    weights = weights_for(derived) if name != "plane" or derived != 3 else (KERNEL_EDGE if rows > 8 else KERNEL_SHARPEN)
                out.append(("window", (name, rows, cols), (RES, op, edge, size, length, weights)))
    return out


def window_max_cases(edge):
    """65 cells: on the 8 x 5 grid every window is the whole map; on 33 x 9 (two tiles each way) two forms only"""
    out = [("window", ("inf", 8, 5), (RES, op, edge, WINDOW_SIZE_MAX, 0.0, weights_for(WINDOW_SIZE_MAX) if op == R.WEIGHTED_SUM else None))
           for op in (R.SUM, R.MIN_OF_FINITES, R.STDDEV, R.WEIGHTED_SUM) if not (op == R.WEIGHTED_SUM and edge == R.CROP)]
    if edge == R.CROP:
        out.append(("window", ("inf", 33, 9), (RES, R.STDDEV, edge, WINDOW_SIZE_MAX, 0.0, None)))
    if edge == R.EMPTY:
        out.append(("window", ("inf", 33, 9), (RES, R.SUM, edge, 0, 6.5, None)))           # derived: round(65.0) = 65
    return out


def curvature_cases():
    out = []
    for rows, cols in SHAPES:
        for name, _ in contents(rows, cols).items():
            for res in (RES, RES_BINARY):
                out.append(("curvature", (name, rows, cols), (res,)))
    return out


_EXPECTED = {}


def expected(case):
    """-> (layer, counts, window size or 0), once per case"""
    kind, key, args = case
    k = (kind, key) + tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args)
    if k not in _EXPECTED:
        z = grid_of(key)
        if kind == "radius":
            res, pos, op, radius = args
            _EXPECTED[k] = R.radius_filter(z, res, pos, op, radius) + (0,)
        elif kind == "window":
            res, op, edge, size, length, weights = args
            _EXPECTED[k] = R.window_filter(z, res, op, edge, size, length, weights)
        else:
            _EXPECTED[k] = R.curvature_filter(z, args[0]) + (0,)
    return _EXPECTED[k]


def describe(case):
    kind, key, args = case
    return f"{kind} {key} " + " ".join("weights" if isinstance(a, np.ndarray) else repr(a) for a in args)
