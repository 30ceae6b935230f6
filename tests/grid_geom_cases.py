"""The cases tests/test_grid_geom_cpu.py (the header on the host) and tests/test_gpu_grid_geom.py (the device) both run against
tests/grid_geom_restate.py: the shapes, layers with special words, the move targets, the submap windows and the placements of
`other` for extendToInclude and addDataFrom.  The smallest shapes at which the kernels can still go wrong: 1 and 2 rows, one
short of, equal to and one past a wave (63, 64, 65), more than one 256-lane block (257 rows; 65 x 5), 1, 2 and 5 columns."""
import numpy as np

import grid_sample_restate as gs
import grid_geom_restate as R

f32, u32 = np.float32, np.uint32
ROWS, COLS, N_LAYERS = (1, 2, 63, 64, 65, 257), (1, 2, 5), (1, 10, 16)
# NaN with payloads (quiet, negative, signalling), +-inf, -0.0f
SPECIAL = (0x7fc12345, 0xffc54321, 0x7f812345, 0x7f800000, 0xff800000, 0x80000000)


def shapes():
    """every (rows, cols) once, the layer counts cycling -> [(rows, cols, n_layers, resolution)]"""
    out = []
    for i, rows in enumerate(ROWS):
        for j, cols in enumerate(COLS):
            out.append((rows, cols, N_LAYERS[(i + j) % 3], 0.1 if (i + j) % 2 else 0.25))
    return out


def layers_of(shape, n_layers, seed):
    """[n_layers, rows, cols] float32: uniform values, a fifth of the cells special words"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (n_layers,) + tuple(shape)).astype(f32)
    special = rng.random(a.shape) < 0.2
    a.view(u32)[special] = np.asarray(SPECIAL, u32)[rng.integers(0, len(SPECIAL), int(special.sum()))]
    return a


def geometry(rows, cols, res):
    return gs.Geometry(rows, cols, res, (1.5, -2.25))


def move_targets(g):
    """positions that shift by 0, +-1, size - 1, size, size + 1 cells per axis and on both, and by fractions of a cell"""
    rows, cols = g.size
    shifts = [(s, 0) for s in (0, 1, -1, rows - 1, -(rows - 1), rows, -rows, rows + 1)]
    shifts += [(0, s) for s in (1, -1, cols - 1, cols, -cols, -(cols + 1))]
    shifts += [(1, -1), (rows - 1, cols - 1), (rows, 1), (-(rows + 1), cols + 1), (-1, cols)]
    out = [(g.pos[0] - s0 * g.res, g.pos[1] - s1 * g.res) for s0, s1 in shifts]
    out += [(g.pos[0] + 0.49 * g.res, g.pos[1] - 0.49 * g.res),            # no move
            (g.pos[0] + 0.5 * g.res, g.pos[1]), (g.pos[0], g.pos[1] - 0.5 * g.res),            # exactly half a cell: moves by 1
            (g.pos[0] + 0.35, g.pos[1] - 0.45), (g.pos[0] - 1.3, g.pos[1] - 2.65)]
    return out


def submap_windows(g):
    """(position, length): inside the map, over each edge and each corner, zero length, larger than the map, and requested
    centres outside it (which fail)"""
    (l0, l1), (p0, p1) = g.length, g.pos
    frac = [(0.0, 0.0, 0.3, 0.3), (0.1, -0.2, 0.45, 0.6), (0.5, 0.0, 0.4, 0.2), (-0.5, 0.0, 0.4, 0.2), (0.0, 0.5, 0.2, 0.4), (0.0, -0.5, 0.2, 0.4),
            (0.45, 0.45, 0.3, 0.3), (0.45, -0.45, 0.3, 0.3), (-0.45, 0.45, 0.3, 0.3), (-0.45, -0.45, 0.3, 0.3), (0.1, -0.2, 0.0, 0.0),
            (0.0, 0.0, 3.0, 3.0), (0.2, 0.1, 1e6, 1e6), (0.75, 0.0, 1.0, 1.0), (0.0, -0.51, 0.1, 0.1), (-2.0, 3.0, 9.0, 9.0)]
    return [((p0 + a * l0, p1 + b * l1), (c * l0, d * l1)) for a, b, c, d in frac]


def add_cases(g, n_layers, full):
    """`other` inside g, across each side and disjoint; offsets of 0, 0.2 and 0.5 cells; other's resolution x 0.5, 1, 2, 3 (0.3
    against 0.1); overwrite 0 and 1; basicLayers_ empty, one layer, all layers; an id g lacks; the listed layers all, one, some
    -> dicts.  full: every placement, otherwise inside and disjoint only (the large shapes)."""
    (l0, l1), (p0, p1) = g.length, g.pos
    places = [(0.0, 0.0), (0.6, 0.0), (-0.6, 0.0), (0.0, 0.6), (0.0, -0.6), (1.5, -1.5)]
    g_ids = list(range(n_layers))
    other_ids = list(range({1: 3, 10: 12, 16: 16}[n_layers]))             # (an upload's layers are 0 .. n - 1) two that g lacks
    some = [other_ids[-1], 0, other_ids[-2]]
    out = []
    for k, (a, b) in enumerate(places if full else places[0::5]):
        off = (0.0, 0.2, 0.5)[k % 3] * g.res
        ores = g.res * (0.5, 1.0, 2.0, 3.0)[(k + n_layers) % 4]
        orows, ocols = (7, 4)
        if (a, b) == (0.0, 0.0):                               # inside g where g is large enough to hold a cell of `other`
            orows, ocols = max(1, int(0.5 * l0 / ores)), max(1, int(0.5 * l1 / ores))
        out.append(dict(other=gs.Geometry(orows, ocols, ores, (p0 + a * l0 + off, p1 + b * l1 - off)), other_ids=other_ids,
                        extend=k % 4 != 3, overwrite=k % 2, layer_ids=(None, other_ids[-1:], some)[k % 3],
                        basic=([], g_ids[:1], g_ids)[(k // 2) % 3], seed=100 + k))
    return out


# ---- what the library is expected to leave, from the restatement
def expect_submap(g, layers, position, length):
    """-> (the submap as R.GridMap or None, info dict or None); the library's form of the corner rule (clamp)"""
    return R.GridMap.of(g, layers).get_submap(position, length, clamp=True)


def expect_move(g, layers, position):
    m = R.GridMap.of(g, layers)
    return m, R.lib_move(m, position)


def expect_add(g, layers, case, extend_only=False):
    """-> (g's map afterwards, other's map, the counters)"""
    other = R.GridMap.of(case["other"], dict(zip(case["other_ids"], layers_of(case["other"].size, len(case["other_ids"]), case["seed"]))))
    m = R.GridMap.of(g, layers, basic=case["basic"])
    if extend_only:
        return m, other, m.extend_to_include(other)
    ids = case["layer_ids"]
    return m, other, m.add_data_from(other, case["extend"], case["overwrite"], ids is None, ids or ())
