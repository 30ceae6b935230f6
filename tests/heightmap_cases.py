"""Designed inputs for the planning height map (lio_height_map, csrc/lio_heightmap.hip): the edges of its clustering, of its
cell keys and their sort, and of its fill.  numpy only.
case(name) -> (points [n, 3] float32, config overrides); info(name) -> what the case was designed to hold (the defects it
must tell from the correct result, the cells it is about); every case is seeded, built once and cached.  reference(name) is
the restatement's result (tests/heightmap_restate.py), computed once.  tests/test_heightmap_cases_cpu.py proves on the
restatement alone that a case holds what it names and sees its defect; tests/test_gpu_heightmap_edges.py runs the cases on the
device.

Every case runs with remove_outliers = 0 and level_and_ego_filter = 0, so the designed coordinates reach the cell stage as
they are, and carries two corner points that fix the grid: the minimum corner first, the maximum corner last.  The maximum
corner lands in cell (0, 0), which no clustering case designs; the fill cases count it as that cell's one point.  The minimum
corner is dropped (its index equals the size).

Clustering cases are built in units of U = 2^-10 m inside cells of at most 4 m, magnitudes below 8 m: every difference of two
points of a cell and every squared distance that lies near the tolerance is exact in fp32 (test_heightmap_cases_cpu.py checks
the fp32 decisions against integer arithmetic, pair by pair).  A grid cell's points are listed in the order the case wants
them to have inside the cell; `Grid.cloud` merges the cells' lists at random, keeping each list's order, so the in-cell order
is the stable sort's to keep.

What the issue's list asks for and this module states differently:
  * Tied heights.  Two components with equal heights give the same output whichever is taken, so the tie is built in its one
    pinnable form: means +0.0 and -0.0 (equal as floats, different point sets, different bits).  A mean of -0.0 needs an
    underflow in the rounding to float -- the fp64 sum of zeros of either sign from +0.0 is +0.0 -- so that component has one
    member at z = -2^-149 and its other members at zeros of both signs: -2^-149 / 4 rounds to -0.0.
  * 1 x 12 and 12 x 1 with four valid cells: the windows of the first and the last cell are disjoint, so not every hole can
    be filled; the holes whose window holds all four are, and the others stay.
  * Infinite heights cannot reach the fill through this API (coordinates are bounded by LIO_MAX_COORD = 1e15): left out."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_restate as H   # noqa: E402

F = np.float32
U = 2.0 ** -10
PLAIN = dict(remove_outliers=0, level_and_ego_filter=0)
TINY = float(np.finfo(np.float32).smallest_subnormal)          # 2^-149
HM_TILE = 1024                                                  # csrc/lio_heightmap.hip
HM_GROUPS = 4096                                                # the most workgroups k_hm_cluster launches
_BUILDERS, _CACHE, _REF = {}, {}, {}


def up(v):
    """The next float32 above v, as a double"""
    return float(np.nextafter(F(v), F(np.inf)))


class Grid:
    """rows x cols cells of `res` metres laid by the corner points (0, 0) and (X, Y).  slack: X = rows res + res / 4, so the
    size rounds down, the grid is shorter than the cloud and everything within res / 8 of the minimum edges is dropped."""

    def __init__(self, rows, cols, res, slack=False, corner_z=0.0):
        self.rows, self.cols, self.res, self.corner_z = rows, cols, res, corner_z
        self.X, self.Y = (rows * res + (res / 4 if slack else 0.0), cols * res + (res / 4 if slack else 0.0))
        self.top = (rows * res + (res / 8 if slack else 0.0), cols * res + (res / 8 if slack else 0.0))

    def key(self, r, c):
        return r + c * self.rows

    def low(self, r, c):
        """The low corner of cell (r, c): the cell is (low, low + res] on both axes"""
        return self.top[0] - (r + 1) * self.res, self.top[1] - (c + 1) * self.res

    def cell(self, r, c, units):
        """units [k, 3]: x and y offsets from the cell's low corner and absolute z, all in U -> metres, float64"""
        u = np.asarray(units, np.float64).reshape(-1, 3)
        assert (u[:, :2] > 0).all() and (u[:, :2] < self.res / U).all()
        x0, y0 = self.low(r, c)
        return np.stack([x0 + u[:, 0] * U, y0 + u[:, 1] * U, u[:, 2] * U], 1)

    def cloud(self, cells, seed=1):
        """minimum corner, the cells' lists merged at random with each list's order kept, maximum corner"""
        cells = [np.asarray(c, np.float64).reshape(-1, 3) for c in cells]
        n = sum(len(c) for c in cells)
        out = np.zeros((n, 3))
        slots = np.random.default_rng(seed).permutation(n)
        at = 0
        for c in cells:
            out[np.sort(slots[at:at + len(c)])] = c
            at += len(c)
        pts = np.concatenate([[[0.0, 0.0, 0.0]], out, [[self.X, self.Y, self.corner_z]]])
        assert np.array_equal(pts.astype(F).astype(np.float64), pts)          # every coordinate is a float32
        return pts.astype(F)


def register(name, **kw):
    def deco(fn):
        assert name not in _BUILDERS, name
        _BUILDERS[name] = (fn, kw)
        return fn
    return deco


def names(prefix=""):
    return [n for n in _BUILDERS if n.startswith(prefix)]


def _built(name):
    if name not in _CACHE:
        fn, kw = _BUILDERS[name]
        pts, cfg, inf = fn(**kw)
        pts.setflags(write=False)
        _CACHE[name] = (pts, dict(PLAIN, **cfg), inf)
    return _CACHE[name]


def case(name):
    pts, cfg, _ = _built(name)
    return pts, dict(cfg)


def info(name):
    return _built(name)[2]


def reference(name):
    """The restatement on the case, computed once and shared: do not write into it"""
    if name not in _REF:
        pts, cfg = case(name)
        _REF[name] = H.height_map(pts, **cfg)
    return _REF[name]


def cell_points(pts, cfg, r, c):
    """The points of cell (r, c) in the order the stable sort by key leaves them in, and their indices in the cloud"""
    p = np.asarray(pts, F)
    g = H.geometry(p, cfg["resolution"])
    rr, cc, inside = H.bin_cells(p, g)
    idx = np.nonzero(inside & (rr == r) & (cc == c))[0]         # ascending index = the stable order inside one key
    return p[idx], idx


# ------------------------------------------------------------------------------------------------------------ A. clustering
CHAIN_TOL = 2.0 ** -8                                           # 4 U: tol2 = 16 U^2; links 3 U long (d2 <= 13), two apart d2 >= 36
CHAIN_SIZES = (2, 64, 65, 256, 257, 1023, 1024, 1025, 1300)
ORDERS = ("asc", "desc", "perm", "zigzag")


def line_order(m, order, seed=0):
    """k[i]: the place along the line of the point with index i"""
    i = np.arange(m)
    if order == "asc":
        return i
    if order == "desc":
        return m - 1 - i
    if order == "perm":
        return np.random.default_rng(1000 + m + seed).permutation(m)
    assert order == "zigzag"                                   # even indices walk in from one end, odd ones from the other
    return np.where(i % 2 == 0, i // 2, m - 1 - i // 2)


def chain(m, order, z0=0, x0=64, y0=512, seed=0):
    """m points 3 U apart along x whose z climbs 0, 1 or 2 U per link (seeded), in index order `order` -> units [m, 3]"""
    step = np.random.default_rng(7 * m + seed).integers(0, 3, m)
    z = z0 + np.cumsum(step) - step[0]
    k = line_order(m, order, seed)
    return np.stack([x0 + 3 * k, np.full(m, y0), z[k]], 1)


def blob(n, spacing, origin, nx, ny):
    """The first n points of a lattice, x fastest, then y, then z: one component whenever spacing <= tolerance -> units"""
    i = np.arange(n)
    return np.stack([origin[0] + spacing * (i % nx), origin[1] + spacing * ((i // nx) % ny), origin[2] + spacing * (i // (nx * ny))], 1)


def shuffled(parts, seed):
    a = np.concatenate(parts)
    return a[np.random.default_rng(seed).permutation(len(a))]


def _chain_case(m, order):
    g = Grid(2, 1, 4.0)
    pts = g.cloud([g.cell(1, 0, chain(m, order))])
    cfg = dict(resolution=4.0, use_cluster=1, cluster_tolerance=CHAIN_TOL, cluster_min_points=m)
    # two points are one component after a single sweep: that chain pins cluster_min_points at the component's size instead
    return pts, cfg, dict(defects=["one_sweep"] if m > 2 else ["cluster_min_strict"], cell=(1, 0), sizes=[m], chain=True)


for _m in CHAIN_SIZES:
    for _o in ORDERS:
        register(f"chain_{_o}_{_m}", m=_m, order=_o)(_chain_case)


def _two_chains(m, use_max):
    """Two chains at the same x, 2 m apart in z, even indices one and odd indices the other, walked in opposite directions"""
    g = Grid(2, 1, 4.0)
    a, b = chain(m, "asc", z0=0, seed=1), chain(m, "desc", z0=2048, seed=2)
    both = np.empty((2 * m, 3))
    both[0::2], both[1::2] = a, b
    pts = g.cloud([g.cell(1, 0, both)])
    cfg = dict(resolution=4.0, use_cluster=1, cluster_tolerance=CHAIN_TOL, cluster_min_points=m, use_max_height=use_max)
    return pts, cfg, dict(defects=["one_sweep"], cell=(1, 0), sizes=[m, m], chain=True)


for _m in (300, 600):                                           # 600 and 1200 points: LDS and global memory
    for _u in (0, 1):
        register(f"two_chains_{_m}_max{_u}", m=_m, use_max=_u)(_two_chains)


@register("tol_eq_small")
def _tol_eq_small():
    """d2 == tol2 joins (tolerance 0.25 = 256 U, tol2 = 2^-4 exactly); one float further out does not.  cluster_min_points 2."""
    g = Grid(2, 3, 1.0)
    pair = g.cell(1, 0, [[256, 256, 512], [512, 256, 512]])
    split = g.cell(0, 1, [[256, 256, 512], [512, 256, 512]])
    split[1, 0] = up(split[1, 0])
    tri = g.cell(1, 1, [[256, 256, 256], [256, 256, 512], [256, 512, 512]])        # a - b along z, b - c along y, a - c apart
    tri_split = g.cell(0, 2, [[256, 256, 256], [256, 256, 512], [256, 512, 512]])
    tri_split[2, 1] = up(tri_split[2, 1])
    pts = g.cloud([pair, split, tri, tri_split])
    cfg = dict(resolution=1.0, use_cluster=1, cluster_tolerance=0.25, cluster_min_points=2)
    want = {(1, 0): F(0.5), (0, 1): None, (1, 1): F((256 + 512 + 512) * U / 3.0), (0, 2): F(0.375)}
    return pts, cfg, dict(defects=["lt"], want=want, joined=[(1, 0), (1, 1)], split=[(0, 1), (0, 2)])


@register("tol_eq_big")
def _tol_eq_big():
    """The same pair, joined and split, as the first and the last point of a cell of 1102 points; the 1100 others are one
    lattice component 1.5 m above.  The lowest component of at least two points: the pair where it is joined."""
    g = Grid(2, 2, 4.0)
    fill_a = blob(1100, 64, (2048, 2048, 2048), 10, 10)
    a = g.cell(1, 0, np.concatenate([[[256, 256, 512]], fill_a, [[512, 256, 512]]]))
    b = g.cell(0, 1, np.concatenate([[[256, 256, 512]], fill_a, [[512, 256, 512]]]))
    b[-1, 0] = up(b[-1, 0])
    pts = g.cloud([a, b])
    cfg = dict(resolution=4.0, use_cluster=1, cluster_tolerance=0.25, cluster_min_points=2)
    high = H.ordered_mean((fill_a[:, 2] * U).astype(F))
    return pts, cfg, dict(defects=["lt"], want={(1, 0): F(0.5), (0, 1): high}, joined=[(1, 0)], split=[(0, 1)], long_cells=[(1, 0), (0, 1)])


@register("tol_zero")
def _tol_zero():
    """cluster_tolerance 0: only exact duplicates join.  p q p r q p with cluster_min_points 2: {p p p} at 1.0, {q q} at 0.5"""
    g = Grid(2, 1, 1.0)
    p, q, r = [100, 100, 1024], [100, 101, 512], [101, 100, 100]
    pts = g.cloud([g.cell(1, 0, [p, q, p, r, q, p])])
    cfg = dict(resolution=1.0, use_cluster=1, cluster_tolerance=0.0, cluster_min_points=2)
    return pts, cfg, dict(defects=["lt"], want={(1, 0): F(0.5)}, cell=(1, 0), sizes=[3, 2, 1])


def three_chains(n, seed):
    """n points: three chains over the same x, 2.5 m apart in z, of n // 2, n // 3 and the rest, index order shuffled"""
    sizes = [n // 2, n // 3, n - n // 2 - n // 3]
    return shuffled([chain(m, "asc", z0=2560 * k, seed=seed + k) for k, m in enumerate(sizes)], seed), sizes


def _tile_cells(use_max):
    g = Grid(2, 2, 2.0)
    cells, sizes = {}, {}
    for (r, c), n in (((1, 0), HM_TILE - 1), ((0, 1), HM_TILE), ((1, 1), HM_TILE + 1)):
        units, sizes[(r, c)] = three_chains(n, 10 * n)
        cells[(r, c)] = g.cell(r, c, units)
    pts = g.cloud(list(cells.values()))
    cfg = dict(resolution=2.0, use_cluster=1, cluster_tolerance=CHAIN_TOL, cluster_min_points=min(s[2] for s in sizes.values()),
               use_max_height=use_max)
    return pts, cfg, dict(defects=["one_sweep"], cell_sizes=sizes, chain=True)


for _u in (0, 1):
    register(f"tile_cells_max{_u}", use_max=_u)(_tile_cells)


@register("two_long_cells")
def _two_long_cells():
    """Keys 1 and 3 are cells of 1100 points (two chains; four chains), key 2 between them a cell of 15 in three lattices"""
    g = Grid(2, 2, 2.0)
    a = shuffled([chain(600, "desc", z0=0, seed=1), chain(500, "zigzag", z0=3072, seed=2)], 3)
    b = shuffled([chain(m, o, z0=1536 * k, seed=4 + k) for k, (m, o) in enumerate(((300, "asc"), (300, "perm"), (300, "desc"), (200, "zigzag")))], 5)
    small = shuffled([blob(4, 2, (100, 100, 100), 2, 2), blob(5, 2, (100, 100, 1000), 2, 2), blob(6, 2, (100, 100, 2000), 2, 2)], 6)
    pts = g.cloud([g.cell(1, 0, a), g.cell(0, 1, small), g.cell(1, 1, b)])
    cfg = dict(resolution=2.0, use_cluster=1, cluster_tolerance=CHAIN_TOL, cluster_min_points=5, use_max_height=1)
    return pts, cfg, dict(defects=["one_sweep"], cell_sizes={(1, 0): [600, 500], (0, 1): [4, 5, 6], (1, 1): [300, 300, 300, 200]}, chain=True,
                          lattices=[(0, 1)])


TIE_PAIRS = ((0, 300), (63, 64), (255, 256), (700, 5))          # in-cell positions of the two tied components' first members
TIE_TOL = 2.0 ** -4                                             # 64 U


def tie_cell(a, b, neg_at_a):
    """Components N (mean -0.0) and P (mean +0.0) of four points each, first members at in-cell positions a and b (N at a if
    neg_at_a), every other position before them one lattice component D two metres up -> units [n, 3] as float64 (z of N's
    first member is -2^-149 m, kept apart from the unit scale)"""
    n = max(a, b) + 7
    neg = np.array([[64, 64, 0], [96, 64, 0], [128, 64, 0], [160, 64, 0]], np.float64)
    pos = np.array([[64, 256, 0], [96, 256, 0], [128, 256, 0], [160, 256, 0]], np.float64)
    neg[:, 2] = [-TINY / U, -0.0, 0.0, -0.0]
    pos[:, 2] = [0.0, -0.0, 0.0, -0.0]
    first, second = (neg, pos) if neg_at_a else (pos, neg)
    d = blob(n - 8, 16, (512, 512, 2048), 12, 12).astype(np.float64)
    out = np.zeros((n, 3))
    out[a], out[b] = first[0], second[0]
    out[n - 6:n - 3], out[n - 3:] = first[1:], second[1:]
    rest = np.setdiff1d(np.arange(n - 6), [a, b])
    out[rest] = d
    return out


def _ties(use_max):
    """Eight cells: every pair of TIE_PAIRS with -0.0 at its first place and at its second.  cluster_max_points 4 rejects D."""
    g = Grid(3, 3, 1.0)
    where = [(r, c) for c in range(3) for r in range(3) if (r, c) != (0, 0)]
    cells, design = [], {}
    for k, (r, c) in enumerate(where):
        a, b = TIE_PAIRS[k // 2]
        neg_at_a = k % 2 == 0
        cells.append(g.cell(r, c, tie_cell(a, b, neg_at_a)))
        design[(r, c)] = dict(first=(a, b), negative_wins=(a < b) == neg_at_a)
    pts = g.cloud(cells)
    cfg = dict(resolution=1.0, use_cluster=1, cluster_tolerance=TIE_TOL, cluster_min_points=4, cluster_max_points=4, use_max_height=use_max)
    return pts, cfg, dict(defects=["tie_last", "tie_larger_first_member"], ties=design)


for _u in (0, 1):
    register(f"ties_max{_u}", use_max=_u)(_ties)

BEST_AT = (64 + 7, 128 + 33, 192 + 63, 256 + 70, 512 + 129)     # non-zero lanes of waves 1, 2, 3, and of 1 and 2 at later strides


def _best_lane(use_max):
    """The best component's first member at position p of BEST_AT; the lattice component D (first member 0) loses"""
    g = Grid(3, 2, 1.0)
    zb = 4096 if use_max else 512
    where = [(1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]
    cells, design = [], {}
    for (r, c), p in zip(where, BEST_AT):
        best = np.array([[64, 64, zb], [96, 64, zb + 2], [128, 64, zb + 4], [160, 64, zb + 7]])
        units = np.concatenate([blob(p, 16, (512, 512, 2048), 12, 12), best, blob(3, 16, (512, 800, 2048), 12, 12)])
        cells.append(g.cell(r, c, units))
        design[(r, c)] = dict(position=p, height=H.ordered_mean((best[:, 2] * U).astype(F)))
    pts = g.cloud(cells)
    cfg = dict(resolution=1.0, use_cluster=1, cluster_tolerance=TIE_TOL, cluster_min_points=3, use_max_height=use_max)
    return pts, cfg, dict(defects=["wave0_only"], best=design)


for _u in (0, 1):
    register(f"best_lane_max{_u}", use_max=_u)(_best_lane)

SIZE_Z = {2: 256, 3: 1024, 6: 2048, 7: 3072}                    # component size -> its flat height in U


def sized_cell(sizes, seed):
    return shuffled([blob(s, 16, (100 + 200 * k, 100, SIZE_Z[s]), 3, 3) * [1, 1, 0] + [0, 0, SIZE_Z[s]] for k, s in enumerate(sizes)], seed)


def _size_limits(use_max, cl_min=3, cl_max=6, defects=None):
    """cluster_min_points 3, cluster_max_points 6.  Cell (1, 0): flat components of 2, 3, 6 and 7 points, lower the smaller;
    cell (0, 1): of 2 and 7 only, every one rejected; cell (1, 1): of 3 and 6 only."""
    g = Grid(2, 2, 1.0)
    layout = {(1, 0): [2, 3, 6, 7], (0, 1): [7, 2], (1, 1): [6, 3]}
    pts = g.cloud([g.cell(r, c, sized_cell(s, 11 + r + 2 * c)) for (r, c), s in layout.items()])
    cfg = dict(resolution=1.0, use_cluster=1, cluster_tolerance=TIE_TOL, cluster_min_points=cl_min, cluster_max_points=cl_max, use_max_height=use_max)
    return pts, cfg, dict(defects=defects, cell_sizes=layout, heights={s: F(z * U) for s, z in SIZE_Z.items()})


register("size_limits_max0", use_max=0, defects=["cluster_min_lenient", "cluster_min_strict", "cluster_max_lenient"])(_size_limits)
register("size_limits_max1", use_max=1, defects=["cluster_max_lenient", "cluster_max_strict", "cluster_min_lenient"])(_size_limits)
register("cluster_min_zero", use_max=0, cl_min=0, defects=["cluster_min_zero_rejects"])(_size_limits)


def _cell_limits(which):
    """Cells of 4, 5 and 6 points, each two flat components, with min_points_per_cell or max_points_per_cell at 5, clustered"""
    g = Grid(2, 2, 1.0)
    layout = {(1, 0): 5, (0, 1): 6, (1, 1): 4}
    cells = [g.cell(r, c, shuffled([blob(m - 2, 16, (100, 100, 512), 2, 2) * [1, 1, 0] + [0, 0, 512], blob(2, 16, (600, 100, 0), 2, 2) * [1, 1, 0] + [0, 0, 1536]], m))
             for (r, c), m in layout.items()]
    cfg = dict(resolution=1.0, use_cluster=1, cluster_tolerance=TIE_TOL, cluster_min_points=2)
    cfg[f"{which}_points_per_cell"] = 5
    return g.cloud(cells), cfg, dict(defects=[f"cell_{which}_lenient", f"cell_{which}_strict"], cell_counts=layout,
                                     valid=[rc for rc, m in layout.items() if (m >= 5 if which == "min" else m <= 5)])


register("cell_min_points", which="min")(_cell_limits)
register("cell_max_points", which="max")(_cell_limits)


@register("many_cells")
def _many_cells():
    """65 x 64 cells of 64 U; workgroup b of 4096 takes cells b and b + 4096.  Pairs (first cell, second cell):
    long (1100 points, two slabs) at 7, three lattices in LDS at 4103; three lattices at 20, long at 4116; a cell of 1300
    points that max_points_per_cell = 1200 refuses at 33, three lattices at 4129.  Most other cells hold 1 .. 3 points."""
    g = Grid(65, 64, 0.0625)
    rng = np.random.default_rng(41)
    def long_cell(n_low):
        return shuffled([blob(n_low, 4, (4, 4, 0), 15, 15), blob(1100 - n_low, 4, (4, 4, 1024), 15, 15)], n_low)
    def lattices(z):
        return shuffled([blob(5, 4, (4, 4, z[0]), 2, 2), blob(7, 4, (32, 4, z[1]), 2, 2), blob(3, 4, (4, 32, z[2]), 2, 2)], z[0])
    designed = {7: long_cell(600), 7 + HM_GROUPS: lattices((512, 100, 2000)), 20: lattices((300, 900, 40)), 20 + HM_GROUPS: long_cell(450),
                33: blob(1300, 4, (4, 4, 0), 15, 15), 33 + HM_GROUPS: lattices((700, 650, 1300))}
    cells = []
    for key in range(65 * 64):
        r, c = key % 65, key // 65
        if key in designed:
            cells.append(g.cell(r, c, designed[key]))
        elif key and rng.uniform() < 0.8:
            m = int(rng.integers(1, 4))
            cells.append(g.cell(r, c, np.c_[4 * rng.integers(1, 16, (m, 2)), rng.integers(0, 1024, m)]))
    cfg = dict(resolution=0.0625, use_cluster=1, cluster_tolerance=2.0 ** -7, cluster_min_points=1, max_points_per_cell=1200, fill_holes=0)
    return g.cloud(cells, seed=43), cfg, dict(defects=["no_round_robin"], keys=sorted(designed), long=[7, 20 + HM_GROUPS], refused=33)


# ----------------------------------------------------------------------------------------------- B. cell keys and the sort
def _sort_width(rows, cols):
    """rows x cols cells of 16 U on a cloud a quarter cell longer: the size rounds down, and every point within 2 U of the
    minimum edges gets the key behind the last cell.  Cells 0 and n_cells - 1 are occupied; the dropped points stand at 7 m."""
    g = Grid(rows, cols, 2.0 ** -6, slack=True)
    rng = np.random.default_rng(rows * 1000 + cols)
    n = 3000
    r, c = rng.integers(0, rows, n), rng.integers(0, cols, n)
    r[:3], c[:3] = 0, 0
    r[3:6], c[3:6] = rows - 1, cols - 1
    off = rng.integers(1, 16, (n, 2))
    off[3] = [1, 1]                                             # 3 U above the minimum corner: the lowest point still binned
    x0 = g.top[0] - (r + 1) * g.res
    y0 = g.top[1] - (c + 1) * g.res
    kept = np.stack([x0 + off[:, 0] * U, y0 + off[:, 1] * U, rng.integers(0, 1024, n) * U], 1)
    # dropped: x or y at 1 U and at 2 U (index == size exactly), the other coordinate anywhere
    lost = np.array([[1 * U, 5 * U, 7.0], [2 * U, g.Y - U, 7.0], [g.X - U, 1 * U, 7.0], [9 * U, 2 * U, 7.0], [2 * U, 2 * U, 7.0]] * 4)
    lost[:, 2] += np.arange(len(lost)) * U
    body = np.concatenate([kept, lost])[rng.permutation(n + len(lost))]
    pts = np.concatenate([[[0.0, 0.0, 0.0]], body, [[g.X, g.Y, 0.0]]]).astype(F)
    cfg = dict(resolution=2.0 ** -6, fill_holes=0)
    return pts, cfg, dict(defects=["dropped_to_first", "dropped_to_last"], shape=(rows, cols), n_dropped=len(lost) + 1)


for _r, _c in ((15, 17), (16, 16), (257, 1), (255, 257), (256, 256)):
    register(f"sort_{_r * _c}", rows=_r, cols=_c)(_sort_width)

FAR_SHIFT = (65536.0, -32768.0)


def _far(extent, resolution=0.25, defects=("position_ignored",)):
    """The lattice of test_binning_edges, moved by FAR_SHIFT.  At the extents of that test every coordinate, the box's fp32 sum
    and difference and the whole index vector are multiples of 2^-7 below 2^17: exact in fp32 as in fp64, so those three
    cases see a grid's position being used at all, not its precision.  An extent with an odd multiple of 2^-7 makes the box's
    fp32 sum round (the reference's own arithmetic: an fp64 sum is the defect), and a resolution of 0.35 makes the fp32 index
    vector differ from the fp64 one."""
    ex, ey = extent
    xs, ys = np.r_[np.arange(0, ex, 0.375), ex], np.r_[np.arange(0, ey, 0.375), ey]
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    z = np.random.default_rng(3).uniform(-1, 1, X.size)
    pts = np.c_[X.ravel() + FAR_SHIFT[0], Y.ravel() + FAR_SHIFT[1], z].astype(F)
    return pts, dict(resolution=resolution), dict(defects=list(defects), extent=extent)


for _k, _e in enumerate(((2.125, 1.625), (2.0625, 1.5625), (2.0, 1.5))):
    register(f"far_{_k}", extent=_e)(_far)
register("far_odd_extent", extent=(2.0 + 31 * 2.0 ** -7, 1.5625), defects=("box_fp64",))(_far)
register("far_resolution_035", extent=(2.0, 1.5), resolution=0.35, defects=("keys_fp32",))(_far)


def _thin(rows, cols):
    g = Grid(rows, cols, 2.0 ** -5)
    rng = np.random.default_rng(rows + 2 * cols)
    cells = [g.cell(r, c, np.c_[rng.integers(1, 32, (m, 2)), rng.integers(0, 2048, m)])
             for r in range(rows) for c in range(cols) for m in [int(rng.integers(0, 3))] if m and (r, c) != (0, 0)]
    return g.cloud(cells), dict(resolution=2.0 ** -5, fill_holes=1), dict(defects=["swap_axes"], shape=(rows, cols))


for _r, _c in ((1, 12), (12, 1), (1, 300), (300, 1)):
    register(f"thin_{_r}x{_c}", rows=_r, cols=_c)(_thin)


# ------------------------------------------------------------------------------------------------------------------ C. fill
def from_mask(values, res=0.5):
    """One point at the centre of every cell whose value is not NaN; cell (0, 0) must be valid: its point is the maximum
    corner itself -> points"""
    v = np.asarray(values, np.float64)
    rows, cols = v.shape
    assert not np.isnan(v[0, 0])
    r, c = np.nonzero(~np.isnan(v))
    keep = (r > 0) | (c > 0)
    r, c = r[keep], c[keep]
    body = np.c_[rows * res - res * (r + 0.5), cols * res - res * (c + 0.5), v[r, c]]
    body = body[np.random.default_rng(rows * 31 + cols).permutation(len(body))]
    return np.concatenate([[[0.0, 0.0, 0.0]], body, [[rows * res, cols * res, v[0, 0]]]]).astype(F)


def _fill_case(values, defects, **inf):
    v = np.asarray(values, np.float64)
    return from_mask(v), dict(resolution=0.5, fill_holes=1), dict(defects=defects, values=v.astype(F), **inf)


def _small(shape, k):
    """k valid cells with distinct values; at k = 3 no hole can be filled"""
    spots = {(1, 12): [(0, 0), (0, 2), (0, 4), (0, 3)], (12, 1): [(0, 0), (2, 0), (4, 0), (3, 0)],
             (3, 3): [(0, 0), (1, 1), (2, 2), (0, 2)], (4, 4): [(0, 0), (1, 2), (3, 1), (2, 3)]}[shape]
    v = np.full(shape, np.nan)
    for j, rc in enumerate(spots[:k]):
        v[rc] = [1.0, 2.5, -4.0, 8.125][j]
    return _fill_case(v, ["fill_three_enough"] if k == 3 else ["fill_in_place"], k=k)


for _s in ((1, 12), (12, 1), (3, 3), (4, 4)):
    for _k in (3, 4):
        register(f"fill_small_{_s[0]}x{_s[1]}_{_k}", shape=_s, k=_k)(_small)


def _four_in_row(shape, R, transpose, filled, stays):
    """Valid: four cells of row R (and the corner cell).  The hole `filled` has them in row r - 5 of its window or nearer; the
    hole `stays` has them in row r + 5, just outside [r - 5, r + 5).  transpose: the same for columns."""
    v = np.full(shape, np.nan)
    v[0, 0] = 16.0
    v[R, 4:8] = [1.0, 2.0, 4.0, 8.0]
    if transpose:
        v, filled, stays = v.T, filled[::-1], stays[::-1]
    return _fill_case(v, ["fill_symmetric"], filled=tuple(filled), stays=tuple(stays))


register("fill_asym_rows", shape=(14, 12), R=8, transpose=False, filled=(13, 5), stays=(3, 5))(_four_in_row)
register("fill_asym_cols", shape=(14, 12), R=8, transpose=True, filled=(13, 5), stays=(3, 5))(_four_in_row)
# at a border the window is clipped: from row 0 it is [0, 5), from the last row of 12 it is [6, 12)
register("fill_border_top", shape=(12, 12), R=5, transpose=False, filled=(10, 6), stays=(0, 6))(_four_in_row)
register("fill_border_bottom", shape=(12, 12), R=6, transpose=False, filled=(11, 6), stays=(1, 6))(_four_in_row)
register("fill_border_left", shape=(12, 12), R=5, transpose=True, filled=(10, 6), stays=(0, 6))(_four_in_row)
register("fill_border_right", shape=(12, 12), R=6, transpose=True, filled=(11, 6), stays=(1, 6))(_four_in_row)


@register("fill_scan_order")
def _scan_order():
    """Hole (6, 6) of 13 x 13: its only valid cells are the eight a knight's move away, all at squared distance 5.  Rows
    outermost, the strict-< cascade keeps the first four scanned: (4, 5), (4, 7), (5, 4), (5, 8)."""
    v = np.full((13, 13), np.nan)
    v[0, 0] = 0.5
    for k, (dr, dc) in enumerate(((-2, -1), (-2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, -1), (2, 1))):
        v[6 + dr, 6 + dc] = 2.0 ** k
    return _fill_case(v, ["fill_cols_outermost"], hole=(6, 6), want=F((1.0 + 2.0 + 4.0 + 8.0) / 4.0))


@register("fill_sum_order")
def _sum_order():
    """Hole (6, 2): valid cells at distances 1, 2, 3, 4 along its row with values 2^40, 2^-14, -2^40, 2^-14.  In that order the
    fp64 sum is 2^-14 (2^40 + 2^-14 rounds to 2^40); pairwise or sorted it is 0 or 2^-13."""
    v = np.full((13, 13), np.nan)
    v[0, 0] = 0.5
    v[6, 3:7] = [2.0 ** 40, 2.0 ** -14, -2.0 ** 40, 2.0 ** -14]
    return _fill_case(v, ["fill_pairwise_sum"], hole=(6, 2), want=F(2.0 ** -16))


@register("fill_no_chain")
def _no_chain():
    """16 x 1, valid rows 0 .. 4.  Hole 6 sees rows 1 .. 4 and is filled; hole 7 sees rows 2 .. 4 only and stays, unless it reads
    hole 6's (or 5's) new value"""
    v = np.full((16, 1), np.nan)
    v[:5, 0] = [3.0, 1.0, 2.0, 4.0, 8.0]
    return _fill_case(v, ["fill_in_place"], filled=(6, 0), stays=(7, 0))
