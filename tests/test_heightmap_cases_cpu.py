"""tests/heightmap_cases.py on the CPU (no GPU): every designed input has the property it was designed for, and the
restatement (tests/heightmap_restate.py) on that input differs in bits from a plainly wrong variant of itself -- the defect
the case names in info(name)["defects"].  The variants below are variants of the restatement, not of the kernel:

  one_sweep                 one propagation sweep, no iteration: a point's label is its smallest neighbour
  lt                        d2 < tol2 in place of <=
  tie_last                  the last of equal heights instead of the first
  tie_larger_first_member   of equal heights, the component with the larger first member
  wave0_only                only components whose first member is in the first 64 of a 256-stride compete
  cluster_{min,max}_{lenient,strict}, cell_{min,max}_{lenient,strict}   a size limit off by one, either side
  cluster_min_zero_rejects  cluster_min_points = 0 read as "no component passes"
  no_round_robin            cells at index 4096 and beyond are never computed
  dropped_to_first / _last  dropped points folded into cell 0 / cell n_cells - 1
  keys_fp32                 the index vector in fp32
  box_fp64                  the box's difference and sum in fp64 (the reference's are float)
  position_ignored          the grid taken as centred on the origin
  swap_axes                 rows and columns exchanged in the layer
  fill_symmetric            the window [r - 5, r + 5] x [c - 5, c + 5]
  fill_cols_outermost       columns outermost in the fill's scan
  fill_in_place             a fill reads the fills before it
  fill_pairwise_sum         (v1 + v2) + (v3 + v4)
  fill_three_enough         three valid cells are enough"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_cases as K     # noqa: E402
import heightmap_restate as H   # noqa: E402

f32 = np.float32
U = K.U


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))          # (one NaN pattern on the CPU)


# ---- the wrong variants -----------------------------------------------------------------------------------------------------
def v_components(p, tol, defect):
    tol2 = f32(float(f32(tol)) * float(f32(tol)))
    if defect not in ("one_sweep", "lt"):
        return H.components(p, tol)
    d = p[:, None, :] - p[None, :, :]
    d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if defect == "one_sweep":
        return (d2 <= tol2).argmax(1)                           # the first neighbour (a point is its own)
    near = d2 < tol2
    lab = np.full(len(p), -1, np.int64)
    for seed in range(len(p)):
        if lab[seed] >= 0:
            continue
        lab[seed] = seed
        stack = [seed]
        while stack:
            new = np.nonzero(near[stack.pop()] & (lab < 0))[0]
            lab[new] = seed
            stack.extend(new.tolist())
    return lab


def v_cell_height(pts, cfg, defect):
    m = len(pts)
    lo = cfg["min_points_per_cell"] + {"cell_min_lenient": -1, "cell_min_strict": 1}.get(defect, 0)
    hi = cfg["max_points_per_cell"] + {"cell_max_lenient": 1, "cell_max_strict": -1}.get(defect, 0)
    if m == 0 or m < lo or m > hi:
        return f32(np.nan)
    if not cfg["use_cluster"]:
        return H.ordered_mean(pts[:, 2])
    if defect == "cluster_min_zero_rejects" and cfg["cluster_min_points"] == 0:
        return f32(np.nan)
    lab = v_components(pts, cfg["cluster_tolerance"], defect)
    cl_lo = cfg["cluster_min_points"] + {"cluster_min_lenient": -1, "cluster_min_strict": 1}.get(defect, 0)
    cl_hi = cfg["cluster_max_points"] + {"cluster_max_lenient": 1, "cluster_max_strict": -1}.get(defect, 0)
    cand = []                                                   # (height, first member) of the kept components, ascending first member
    for r in np.unique(lab):
        if lab[r] != r or (defect == "wave0_only" and r % 256 >= 64):
            continue
        z = pts[lab == r, 2]
        if cl_lo <= len(z) <= cl_hi:
            cand.append((H.ordered_mean(z), int(r)))
    if not cand:
        return f32(np.nan)
    sign = -1.0 if cfg["use_max_height"] else 1.0
    if defect == "tie_larger_first_member":
        best = min(sign * float(h) for h, _ in cand)
        return [h for h, r in cand if sign * float(h) == best][-1]
    best = cand[0][0]
    for h, _ in cand[1:]:
        if (h >= best if cfg["use_max_height"] else h <= best) if defect == "tie_last" else (h > best if cfg["use_max_height"] else h < best):
            best = h
    return best


def v_fill(layer, defect):
    rows, cols = layer.shape
    src = layer.copy()
    out = layer.copy()
    n = 0
    reach = 6 if defect == "fill_symmetric" else 5
    for row, col in zip(*np.nonzero(np.isnan(layer))):
        row, col = int(row), int(col)
        window = [(i, j) for i in range(max(row - 5, 0), min(row + reach, rows)) for j in range(max(col - 5, 0), min(col + reach, cols))]
        if defect == "fill_cols_outermost":
            window.sort(key=lambda ij: (ij[1], ij[0]))
        cand = [((i - row) ** 2 + (j - col) ** 2, k, float(src[i, j])) for k, (i, j) in enumerate(window) if not np.isnan(src[i, j])]
        cand.sort()                                             # the cascade: by distance, the earliest of equals first
        need = 3 if defect == "fill_three_enough" else 4
        if len(cand) < need:
            continue
        v = [c[2] for c in cand[:4]] + [0.0] * (4 - min(len(cand), 4))
        total = (v[0] + v[1]) + (v[2] + v[3]) if defect == "fill_pairwise_sum" else ((v[0] + v[1]) + v[2]) + v[3]
        out[row, col] = f32(total / 4.0)
        n += 1
        if defect == "fill_in_place":
            src[row, col] = out[row, col]
    return out, n


def variant(name, defect=None):
    """The restatement's chain behind stage 3 with one defect (None: none, which must be H.height_map itself)"""
    pts, overrides = K.case(name)
    cfg = dict(H.DEFAULTS, **overrides)
    assert not cfg["remove_outliers"] and not cfg["level_and_ego_filter"]
    p = np.asarray(pts, f32)
    g = H.geometry(p.astype(np.float64) if defect == "box_fp64" else p, cfg["resolution"])
    if defect == "box_fp64":                                    # (H.geometry rounds to float32 whatever it is given)
        mn, mx = p[:, :2].astype(np.float64).min(0), p[:, :2].astype(np.float64).max(0)
        size = [H.c_round((mx[a] - mn[a]) / g["resolution"]) for a in range(2)]
        g = dict(g, rows=size[0], cols=size[1], length=np.array(size) * g["resolution"], position=(mx + mn) / 2.0)
    if defect == "position_ignored":
        g = dict(g, position=np.zeros(2))
    rows, cols = g["rows"], g["cols"]
    if defect == "keys_fp32":
        a = -(((p[:, :2] - (f32(0.5) * g["length"].astype(f32))) - g["position"].astype(f32)) / f32(g["resolution"]))
        inside = ((a > -1) & (a < np.array([rows, cols], f32))).all(1)
        idx = np.trunc(np.where(inside[:, None], a, 0)).astype(np.int64)
        r, c = idx[:, 0], idx[:, 1]
    else:
        r, c, inside = H.bin_cells(p, g)
    key = r + c * rows
    if defect in ("dropped_to_first", "dropped_to_last"):
        key = np.where(inside, key, 0 if defect == "dropped_to_first" else rows * cols - 1)
        inside = np.ones(len(p), bool)
    layer = np.full((rows, cols), np.nan, f32)
    for k in np.unique(key[inside]):
        if defect == "no_round_robin" and k >= K.HM_GROUPS:
            continue
        layer[k % rows, k // rows] = v_cell_height(p[inside & (key == k)], cfg, defect)
    out = dict(n_binned=int(inside.sum()), n_valid_cells=int((~np.isnan(layer)).sum()), n_filled_cells=0)
    if cfg["fill_holes"]:
        layer, out["n_filled_cells"] = v_fill(layer, defect)
    out["grid"] = layer.T if defect == "swap_axes" else layer
    return out


# ---- every case: the scaffold is honest, the defect is visible ------------------------------------------------------------------
@pytest.mark.parametrize("name", K.names())
def test_case_sees_its_defects(name):
    ref = K.reference(name)
    pts, cfg = K.case(name)
    assert cfg["remove_outliers"] == 0 and cfg["level_and_ego_filter"] == 0 and ref["n_filtered"] == len(pts)
    none = variant(name)
    assert same_bits(none["grid"], ref["grid"]), "the variant scaffold without a defect is not the restatement"
    assert (none["n_binned"], none["n_valid_cells"], none["n_filled_cells"]) == (ref["n_binned"], ref["n_valid_cells"], ref["n_filled_cells"])
    assert len(pts) - 1 in K.cell_points(pts, cfg, 0, 0)[1]     # the maximum corner, the last point, lands in cell (0, 0)
    defects = K.info(name)["defects"]
    assert defects
    for defect in defects:
        wrong = variant(name, defect)
        assert not same_bits(wrong["grid"], ref["grid"]), (name, defect)


# ---- A. clustering ----------------------------------------------------------------------------------------------------------------
def exact_d2(cell):
    """Squared distances of a cell's points in U^2 as integers (the coordinates are multiples of U), and in fp32 as the kernel forms them"""
    q = np.asarray(cell, np.float64) / U
    assert np.array_equal(q, np.round(q))
    q = q.astype(np.int64)
    d = q[:, None, :] - q[None, :, :]
    p = np.asarray(cell, f32)
    e = p[:, None, :] - p[None, :, :]
    return (d * d).sum(2), ((e[..., 0] * e[..., 0]) + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def sizes_of(lab):
    """Component sizes in order of first member"""
    roots, counts = np.unique(lab, return_counts=True)
    return counts.tolist()


def cluster_cells(name):
    """(r, c) -> designed component sizes, for the cases that state them"""
    inf = K.info(name)
    return inf["cell_sizes"] if "cell_sizes" in inf else {inf["cell"]: inf["sizes"]}


CHAINS = [n for n in K.names() if K.info(n).get("chain")]


@pytest.mark.parametrize("name", CHAINS)
def test_chains_are_joined_link_by_link(name):
    pts, cfg = K.case(name)
    tol2_units = int(round(float(f32(cfg["cluster_tolerance"])) ** 2 / (U * U)))
    tol2 = f32(float(f32(cfg["cluster_tolerance"])) ** 2)
    assert tol2_units == 16 and float(tol2) == 16 * U * U
    for (r, c), want in cluster_cells(name).items():
        cell, _ = K.cell_points(pts, cfg, r, c)
        assert len(cell) == sum(want)
        di, df = exact_d2(cell)
        assert np.array_equal(df <= tol2, di <= tol2_units)     # fp32 decides every pair as the integers do
        lab = H.components(cell, cfg["cluster_tolerance"])
        assert sorted(sizes_of(lab)) == sorted(want)
        for root in np.unique(lab) if (r, c) not in K.info(name).get("lattices", []) else []:       # every component is a path: links at d2 <= 13, nothing else within reach
            mem = np.nonzero(lab == root)[0]
            mem = mem[np.argsort(cell[mem, 0], kind="stable")]
            if len(mem) > 1:
                link = di[mem[:-1], mem[1:]]
                assert link.min() >= 9 and link.max() <= 13 < tol2_units
            if len(mem) > 2:
                assert di[mem[:-2], mem[2:]].min() >= 36 > tol2_units
            near = (di[mem] <= tol2_units).sum(1)
            assert near.max() <= 3 and (len(mem) < 3 or near.min() == 2)       # itself and one or two neighbours
            # the mean of a fragment is not the mean of the whole
            whole = H.ordered_mean(cell[np.sort(mem), 2])
            if len(mem) > 2:
                assert H.ordered_mean(cell[np.sort(mem[:len(mem) // 2]), 2]) != whole
        # the result is a whole component's mean
        heights = [H.ordered_mean(cell[lab == root, 2]) for root in np.unique(lab) if (lab == root).sum() >= cfg["cluster_min_points"]]
        got = K.reference(name)["grid"][r, c]
        assert heights and got == (max(heights) if cfg.get("use_max_height") else min(heights))


@pytest.mark.parametrize("order", K.ORDERS)
def test_chain_index_orders(order):
    m = 9
    k = K.line_order(m, order)
    assert sorted(k.tolist()) == list(range(m))
    want = dict(asc=[0, 1, 2, 3, 4, 5, 6, 7, 8], desc=[8, 7, 6, 5, 4, 3, 2, 1, 0], zigzag=[0, 8, 1, 7, 2, 6, 3, 5, 4]).get(order)
    assert want is None or k.tolist() == want
    if order == "perm":                                         # goes against the spatial order somewhere, and with it somewhere
        k = K.line_order(257, order)
        assert (np.diff(k) > 0).any() and (np.diff(k) < 0).any()
    sizes = {len(K.case(f"chain_{order}_{m}")[0]) - 2 for m in K.CHAIN_SIZES}
    assert sizes == set(K.CHAIN_SIZES) and {K.HM_TILE - 1, K.HM_TILE, K.HM_TILE + 1} <= sizes


def test_tile_boundary_cells():
    for name in ("tile_cells_max0", "tile_cells_max1", "two_long_cells", "tol_eq_big"):
        pts, cfg = K.case(name)
        g = H.geometry(pts, cfg["resolution"])
        r, c, inside = H.bin_cells(pts, g)
        counts = np.bincount((r + c * g["rows"])[inside], minlength=g["rows"] * g["cols"])
        if name.startswith("tile"):
            assert counts.tolist() == [1, K.HM_TILE - 1, K.HM_TILE, K.HM_TILE + 1]
            assert all(len(s) == 3 for s in K.info(name)["cell_sizes"].values())
        elif name == "two_long_cells":                          # long, small, long in key order
            assert counts.tolist() == [1, 1100, 15, 1100] and counts[1] > K.HM_TILE < counts[3]
        else:
            assert counts.tolist() == [1, 1102, 1102, 0]


@pytest.mark.parametrize("name", ["tol_eq_small", "tol_eq_big"])
def test_tolerance_boundary(name):
    pts, cfg = K.case(name)
    inf, ref = K.info(name), K.reference(name)
    tol2 = f32(float(f32(cfg["cluster_tolerance"])) ** 2)
    assert tol2 == f32(0.0625)
    d2 = lambda a, b: ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])
    for rc in inf["joined"] + inf["split"]:
        cell, _ = K.cell_points(pts, cfg, *rc)
        if name == "tol_eq_big":
            assert len(cell) > K.HM_TILE
            links = [(cell[0], cell[-1])]                       # the pair: the cell's first and last point
            others = cell[1:-1]
            assert min(d2(cell[0], o) for o in others) > 1.0 and len(np.unique(H.components(others, 0.25))) == 1
        else:
            links = [(cell[k], cell[k + 1]) for k in range(len(cell) - 1)]
            if len(cell) == 3:
                assert d2(cell[0], cell[2]) > tol2              # joined through the middle point only
        got = [d2(a, b) for a, b in links]
        assert all(type(x) is f32 for x in got)
        if rc in inf["joined"]:
            assert all(x == tol2 for x in got)
        else:                                                   # the last link is one float of the coordinate longer
            assert all(x == tol2 for x in got[:-1]) and tol2 < got[-1] < tol2 * f32(1.00001)
    for rc, want in inf["want"].items():
        assert np.isnan(ref["grid"][rc]) if want is None else ref["grid"][rc] == want, rc


def test_tolerance_zero():
    pts, cfg = K.case("tol_zero")
    cell, _ = K.cell_points(pts, cfg, 1, 0)
    lab = H.components(cell, 0.0)
    assert lab.tolist() == [0, 1, 0, 3, 1, 0] and K.reference("tol_zero")["grid"][1, 0] == f32(0.5)


@pytest.mark.parametrize("name", ["ties_max0", "ties_max1"])
def test_ties_of_signed_zeros(name):
    pts, cfg = K.case(name)
    ref = K.reference(name)
    seen = set()
    for (r, c), d in K.info(name)["ties"].items():
        cell, _ = K.cell_points(pts, cfg, r, c)
        lab = H.components(cell, cfg["cluster_tolerance"])
        roots = np.unique(lab)
        kept = [int(x) for x in roots if (lab == x).sum() == 4]
        assert len(roots) == 3 and sorted(kept) == sorted(d["first"]) and (lab == roots[~np.isin(roots, kept)][0]).sum() > 4
        means = {x: H.ordered_mean(cell[lab == x, 2]) for x in kept}
        assert all(m == 0 for m in means.values())              # equal heights ...
        signs = {x: bool(np.signbit(m)) for x, m in means.items()}
        assert sorted(signs.values()) == [False, True]          # ... of different bits, from different point sets
        assert signs[min(kept)] == d["negative_wins"]
        assert {True, False} == {bool(np.signbit(z)) for z in cell[cell[:, 2] == 0, 2]}       # zeros of both signs among the members
        got = ref["grid"][r, c]
        assert got == 0 and bool(np.signbit(got)) == d["negative_wins"]
        seen.add((d["first"], d["negative_wins"]))
    assert len(seen) == 8 and {f for f, _ in seen} == set(K.TIE_PAIRS)


@pytest.mark.parametrize("name", ["best_lane_max0", "best_lane_max1"])
def test_best_component_in_a_late_lane(name):
    pts, cfg = K.case(name)
    ref = K.reference(name)
    for (r, c), d in K.info(name)["best"].items():
        cell, _ = K.cell_points(pts, cfg, r, c)
        lab = H.components(cell, cfg["cluster_tolerance"])
        p = d["position"]
        assert lab[p] == p and (lab == p).sum() == 4 and lab[0] == 0 and (p % 256) // 64 > 0 and p % 64 > 0
        assert ref["grid"][r, c] == d["height"]
        assert H.ordered_mean(cell[lab == 0, 2]) != d["height"]
    assert {(d["position"] % 256) // 64 for d in K.info(name)["best"].values()} == {1, 2, 3}


@pytest.mark.parametrize("name", ["size_limits_max0", "size_limits_max1", "cluster_min_zero"])
def test_cluster_size_limits(name):
    pts, cfg = K.case(name)
    inf, ref = K.info(name), K.reference(name)
    lo, hi = cfg["cluster_min_points"], cfg["cluster_max_points"]
    for rc, want in inf["cell_sizes"].items():
        cell, _ = K.cell_points(pts, cfg, *rc)
        lab = H.components(cell, cfg["cluster_tolerance"])
        assert sorted(sizes_of(lab)) == sorted(want)
        ok = [inf["heights"][s] for s in want if lo <= s <= hi]
        if ok:
            assert ref["grid"][rc] == (max(ok) if cfg["use_max_height"] else min(ok))
        else:
            assert np.isnan(ref["grid"][rc])
    if lo == 3:
        assert (lo - 1, lo, hi, hi + 1) == (2, 3, 6, 7) == tuple(sorted(inf["cell_sizes"][(1, 0)]))
        assert np.isnan(ref["grid"][0, 1]) and ref["n_valid_cells"] == 2          # every component rejected: NaN, not counted
    else:
        assert ref["grid"][1, 0] == inf["heights"][2] and ref["n_valid_cells"] == 4        # the corner's single point too


@pytest.mark.parametrize("name", ["cell_min_points", "cell_max_points"])
def test_cell_point_limits(name):
    pts, cfg = K.case(name)
    inf, ref = K.info(name), K.reference(name)
    assert sorted(inf["cell_counts"].values()) == [4, 5, 6] and cfg["use_cluster"] == 1
    for rc, m in inf["cell_counts"].items():
        assert len(K.cell_points(pts, cfg, *rc)[0]) == m
        assert np.isnan(ref["grid"][rc]) != (rc in inf["valid"])
    assert len(inf["valid"]) == 2


def test_many_cells_layout():
    pts, cfg = K.case("many_cells")
    inf, ref = K.info("many_cells"), K.reference("many_cells")
    assert (ref["rows"], ref["cols"]) == (65, 64) and ref["rows"] * ref["cols"] > K.HM_GROUPS and cfg["fill_holes"] == 0
    g = H.geometry(pts, cfg["resolution"])
    r, c, inside = H.bin_cells(pts, g)
    counts = np.bincount((r + c * 65)[inside], minlength=65 * 64)
    assert (counts == 0).sum() > 500 and (counts > 0).sum() > 3000
    keys = inf["keys"]
    assert sorted(k % K.HM_GROUPS for k in keys) == [7, 7, 20, 20, 33, 33] and all(k % K.HM_GROUPS < 64 for k in keys)
    assert [int(counts[k]) for k in keys] == [1100, 15, 1300, 15, 1100, 15]
    assert counts[inf["refused"]] > cfg["max_points_per_cell"] >= counts[inf["long"]].max() > K.HM_TILE
    grid = ref["grid"]
    for k in keys:
        cell, _ = K.cell_points(pts, cfg, k % 65, k // 65)
        n_comp = len(np.unique(H.components(cell, cfg["cluster_tolerance"])))
        if k == inf["refused"]:
            assert np.isnan(grid[k % 65, k // 65])
        else:
            assert n_comp == (2 if k in inf["long"] else 3) and not np.isnan(grid[k % 65, k // 65])
    assert np.isnan(grid).any() and ref["n_valid_cells"] > 1000


# ---- B. keys and the sort -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.names("sort_"))
def test_sort_width_grids(name):
    pts, cfg = K.case(name)
    inf, ref = K.info(name), K.reference(name)
    rows, cols = inf["shape"]
    n_cells = rows * cols
    assert (ref["rows"], ref["cols"]) == (rows, cols) and f"sort_{n_cells}" == name
    assert ref["length"][0] < float(pts[-1, 0]) and ref["length"][1] < float(pts[-1, 1])        # the size rounded down
    assert ref["n_binned"] == ref["n_filtered"] - inf["n_dropped"] < ref["n_filtered"]
    assert not np.isnan(ref["grid"][0, 0]) and not np.isnan(ref["grid"][rows - 1, cols - 1])
    key_bits = 1
    while (1 << key_bits) < n_cells + 1:
        key_bits += 1
    assert key_bits == {255: 8, 256: 9, 257: 9, 65535: 16, 65536: 17}[n_cells]
    g = H.geometry(pts, cfg["resolution"])
    a = -(((pts[:, :2].astype(np.float64) - 0.5 * g["length"]) - g["position"]) / g["resolution"])
    assert (a[:, 0] == rows).any() and (a[:, 1] == cols).any()                  # an index equal to the size, exactly
    assert ((a[:, 0] < rows) & (a[:, 0] > rows - 0.07)).any()                   # ... and one just inside the last row


@pytest.mark.parametrize("name", K.names("far_"))
def test_far_from_the_origin(name):
    pts, cfg = K.case(name)
    ref = K.reference(name)
    ex, ey = K.info(name)["extent"]
    assert (ref["rows"], ref["cols"]) == (H.c_round(ex / cfg["resolution"]), H.c_round(ey / cfg["resolution"]))
    assert abs(ref["position"][0]) > 65536 and abs(ref["position"][1]) > 32766
    near = H.height_map((pts.astype(np.float64) - [K.FAR_SHIFT[0], K.FAR_SHIFT[1], 0]).astype(f32), **cfg)
    assert near["n_binned"] > 0 and ref["n_binned"] > 0


@pytest.mark.parametrize("name", K.names("thin_"))
def test_thin_grids(name):
    ref = K.reference(name)
    assert (ref["rows"], ref["cols"]) == K.info(name)["shape"] and min(ref["rows"], ref["cols"]) == 1
    assert 0 < ref["n_valid_cells"] < ref["rows"] * ref["cols"]


# ---- C. fill --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.names("fill_"))
def test_fill_cases(name):
    pts, cfg = K.case(name)
    inf, ref = K.info(name), K.reference(name)
    v, grid = inf["values"], ref["grid"]
    valid = ~np.isnan(v)
    assert grid.shape == v.shape and np.array_equal(bits(grid[valid]), bits(v[valid])) and ref["n_valid_cells"] == int(valid.sum())
    assert ref["n_filled_cells"] == int((~np.isnan(grid)).sum() - valid.sum())
    in_window = lambda r, c: int(valid[max(r - 5, 0):min(r + 5, v.shape[0]), max(c - 5, 0):min(c + 5, v.shape[1])].sum())
    for r, c in zip(*np.nonzero(~valid)):                       # which holes are filled: those with four valid cells in the window
        assert np.isnan(grid[r, c]) == (in_window(r, c) < 4), (r, c)
    if "k" in inf:
        assert int(valid.sum()) == inf["k"] and min(v.shape) < 10
        if inf["k"] == 3:
            assert ref["n_filled_cells"] == 0
        elif v.shape in ((3, 3), (4, 4)):
            assert not np.isnan(grid).any()                     # every hole is filled
        else:
            assert 0 < ref["n_filled_cells"] < v.size - 4       # the far holes' windows do not reach the four
    if "filled" in inf:
        (fr, fc), (sr, sc) = inf["filled"], inf["stays"]
        assert in_window(fr, fc) == 4 and not np.isnan(grid[fr, fc]) and np.isnan(grid[sr, sc])
        if name != "fill_no_chain":                             # the four lie in one row (column): at + 5 of `stays`, within [-5, +5) of `filled`
            by_rows = name in ("fill_asym_rows", "fill_border_top", "fill_border_bottom")
            line = int(np.nonzero((valid[1:] if by_rows else valid[:, 1:].T).sum(1) == 4)[0][0]) + 1
            f, s = (fr, sr) if by_rows else (fc, sc)
            assert line == s + 5 and f - 5 <= line < f + 5 and (line == f - 5 or "border" in name)
            assert int(valid.sum()) == 5
    if "want" in inf:
        assert grid[inf["hole"]] == inf["want"]
    if name == "fill_scan_order":
        r, c = inf["hole"]
        d = sorted((i - r) ** 2 + (j - c) ** 2 for i, j in zip(*np.nonzero(valid)) if r - 5 <= i < r + 5 and c - 5 <= j < c + 5)
        assert len(d) == 8 and d[3] == d[4] == d[7]             # more than four at the fourth-nearest distance


def test_components_against_scipy_on_chains():
    # tests/test_heightmap_cpu.py holds H.components against scipy on random clouds; the same on the designed chains
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    for name in ("chain_perm_257", "chain_zigzag_1025", "two_chains_300_max0", "tile_cells_max0"):
        pts, cfg = K.case(name)
        for (r, c) in cluster_cells(name):
            cell, _ = K.cell_points(pts, cfg, r, c)
            _, df = exact_d2(cell)
            n_comp, lab = connected_components(sp.csr_matrix(df <= f32(float(f32(cfg["cluster_tolerance"])) ** 2)), directed=False)
            mine = H.components(cell, cfg["cluster_tolerance"])
            assert len(np.unique(mine)) == n_comp
            for k in range(n_comp):
                members = np.nonzero(lab == k)[0]
                assert (mine[members] == members[0]).all()
