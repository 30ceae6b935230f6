"""Case builders for the 5-NN grid search at its margins (numpy only, no GPU).

The search of lio_knn_global / lio_knn_range (lio_s2m_device.h) is exact as long as three things hold: the fp32 cell
arithmetic of lio_cell_coord puts every map point within the search bound into the (2k+1)^2 rows (3x3 for a tight table)
around the query's row, the (d2, index) order breaks ties the way FLANN does, and the host picks grids and tables
(lio_plan_grid and lio_plan_tables, lio_gridplan.h) whose margins cover the rounding.  This module restates the host arithmetic
(`grid_of`; tests/test_nn_cases_cpu.py holds it against the library's own plan, field for field), the device's cell formula (`cell_coord_f32`) and FLANN's squared distance (`d2_f32`) bit for bit, and builds
the maps and scans on which those claims are tight: exact lattices, fifth neighbours exactly at the gate and at a table's
acceptance bound, queries outside the grid, maps kilometres long and a few metres wide, and the size caps.

Every builder returns (map, scan, pose0, cfg, note): `cfg` holds ScanToMap settings that belong to the case (the gate, the
cell division, ...), `note` what the case engineered (indices of probe queries and of the map points they hinge on), for
tests/test_nn_cases_cpu.py to verify under the oracle and tests/test_gpu_nn_margins.py to run on the device.
"""
import numpy as np

F = np.float32
FRAC = (0.6, 0.3, 0.15)            # tight tables: cell = reach * 1.001, reach = FRAC[l] * gate radius (lio_plan_tables)
ROW_ALIGN = 8                      # LIO_ROW_ALIGN
MI = 1024.0 * 1024.0
POSE0 = np.zeros(6, F)             # identity: the transformed query IS the scan point, bit for bit


# ------------------------------------------------------------------------------------------------ device / host arithmetic
def cell_coord_f32(v, origin, inv_cell, n):
    """lio_cell_coord: floorf((v - origin) * inv_cell) in fp32, clamped to [-4, n + 3]."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((v - F(origin)) * F(inv_cell))
    c = np.fmin(np.fmax(c, F(-4.0)), F(n + 3))
    return c.astype(np.int64)


def d2_f32(q, m):
    """FLANN L2_Simple in fp32: ((dx*dx) + dy*dy) + dz*dz."""
    q = np.asarray(q, F); m = np.asarray(m, F)
    d = q - m
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _ulp(x):
    return F(np.spacing(F(abs(x))))


def grid_of(map_xyz, cfg=None, long_map_rule=True):
    """The host arithmetic of lio_plan_grid and lio_plan_tables (lio_gridplan.h) for a map and ScanToMap settings, as
    lio_s2m_set_map runs them (environment overrides not modelled).  g["occupied"] = the occupied cells the device would count
    for the automatic table choice, -1 where it counts none.

    long_map_rule=False leaves out the rule "a grid is used only while the fp32 spacing at its far end along y and z is at most
    half of its slack": the grid the library laid out before it had that rule, tables at any extent.  The tests use it to
    show what the rule is for, and that maps under a kilometre get the same grid either way."""
    cfg = dict(cfg or {})
    gate = F(cfg.get("max_sq_dist", 1.0))
    kdiv = cfg.get("cell_div", 2)
    if kdiv not in (1, 2, 3):
        kdiv = 2
    m = np.asarray(map_xyz, F).reshape(-1, 3)
    n = len(m)
    fin = (np.abs(m) <= F(1.0e15)).all(1) if n else np.zeros(0, bool)
    if fin.any():
        mn, mx = m[fin].min(0), m[fin].max(0)
    else:
        mn = mx = np.zeros(3, F)
    root = F(np.sqrt(gate))
    cell_size = F(cfg.get("cell_size", 0.0))
    cell = (cell_size if cell_size > 0 else root * F(1.001)) / F(kdiv)
    max_batch = cfg.get("max_batch", 1)
    xsub = cfg["x_sub"] if cfg.get("x_sub", 0) > 0 else (4 if max_batch >= 8 else 1)
    gate_reach = F(F(root * F(1.0001)) + F(1e-6))
    steps = 0
    while True:
        inv = F(1.0) / cell
        o = mn - F(0.5) * cell
        e = (mx.astype(np.float64) - o.astype(np.float64)) * np.float64(inv)
        dims = np.floor(e) + 2.0
        ok = dims.prod() * xsub <= 256.0 * MI
        if ok and long_map_rule:
            slack = F(kdiv) * cell - gate_reach
            for a in ((0, 1, 2) if cfg.get("use_lds", 0) else (1, 2)):       # (the LDS-staged search walks cx - k .. cx + k)
                ok = ok and bool(_ulp(F(mx[a] - o[a]) + cell) <= F(0.5) * slack)
        if ok:
            break
        cell = cell * F(1.5)
        steps += 1
    nx, ny, nz = (int(d) for d in dims)
    g = dict(k=kdiv, cell=cell, inv_cell=inv, origin=o, nx=nx, ny=ny, nz=nz, n_cells=nx * ny * nz, xs=xsub, nxf=nx * xsub,
             inv_cell_x=inv * F(xsub), gate=gate, gate_reach=gate_reach, grow_steps=steps, mn=mn, mx=mx)
    tight = cfg.get("tight_rows", 0)
    n_tb = min(tight, 3) if tight > 0 else 0
    ppc, try_lvl, occ = F(0.0), -1, -1
    if tight == 0 and max_batch >= 8:
        n_tb = 1
        if n > 0:
            c = [cell_coord_f32(m[fin, a], o[a], inv, d) for a, d in enumerate((nx, ny, nz))]
            inside = (c[0] >= 0) & (c[0] < nx) & (c[1] >= 0) & (c[1] < ny) & (c[2] >= 0) & (c[2] < nz)
            occ = len(np.unique(((c[2] * ny + c[1]) * nx + c[0])[inside]))
            if occ > 0:
                ppc = F(n) / F(occ)
                spacing = cell / F(np.sqrt(ppc))
                while n_tb < 3 and root * F(FRAC[n_tb]) >= F(1.26) * spacing:
                    n_tb += 1
                for l in range(n_tb):
                    if root * F(FRAC[l]) >= F(2.2) * spacing:
                        try_lvl = l
    if float(g["n_cells"]) * xsub > 64.0 * MI:
        n_tb = 0
    tables, len_b, rows_b = [], 0, 0
    nn = max(n, 1)
    for l in range(3):
        if l >= n_tb:
            break
        reach = root * F(FRAC[l]); cb = reach * F(1.001)
        tinv = F(1.0) / cb
        oy, oz = mn[1] - F(0.5) * cb, mn[2] - F(0.5) * cb
        tny = np.floor((np.float64(mx[1]) - np.float64(oy)) * np.float64(tinv)) + 2.0
        tnz = np.floor((np.float64(mx[2]) - np.float64(oz)) * np.float64(tinv)) + 2.0
        recs = float(nn) * ((2 * kdiv + 1) ** 2 + 9.0 * (l + 1)) + ROW_ALIGN * (float(ny) * nz + rows_b + tny * tnz)
        if float(g["n_cells"]) * xsub + len_b + tny * tnz * g["nxf"] > 192.0 * MI or recs > 2040.0 * MI:
            n_tb = l
            break
        if long_map_rule:
            slack = cb - reach / F(1.0001)
            if not (_ulp(F(mx[1] - oy) + cb) <= F(0.5) * slack and _ulp(F(mx[2] - oz) + cb) <= F(0.5) * slack):
                n_tb = l
                break
        r = reach / F(1.0002)
        tables.append(dict(reach=reach, cell=cb, inv_cell=tinv, oy=oy, oz=oz, ny=int(tny), nz=int(tnz),
                           try_b2=F(F(r * r) * F(0.999999)), row0=g["n_cells"] * xsub + len_b))
        rows_b += int(tny) * int(tnz)
        len_b += int(tny) * int(tnz) * g["nxf"]
    g.update(n_tb=n_tb, tables=tables, pts_per_cell=ppc, occupied=occ, buckets=g["n_cells"] * xsub + len_b,
             tb_try=(try_lvl if 0 <= try_lvl < n_tb else (n_tb - 1 if try_lvl >= n_tb else -1)))
    return g


def axis_grid(g, axis, table=None):
    """(origin, inv_cell, n, k) of the main grid (table=None) or of tight table l along y (axis 1) or z (axis 2)."""
    if table is None:
        return g["origin"][axis], g["inv_cell"], (g["nx"], g["ny"], g["nz"])[axis], g["k"]
    t = g["tables"][table]
    return (t["oy"], t["inv_cell"], t["ny"], 1) if axis == 1 else (t["oz"], t["inv_cell"], t["nz"], 1)


def cell_gap(grid, q, m):
    """cell(m) - cell(q) under fp32 for the 1-D grid (origin, inv_cell, n, k); the search sees m iff |gap| <= k."""
    o, inv, n, _ = grid
    return cell_coord_f32(m, o, inv, n) - cell_coord_f32(q, o, inv, n)


def margin_emulation(extent, gate, which, long_map_rule, n_samples=1 << 20, seed=0):
    """CPU emulation (not a measurement on hardware): a y axis of length `extent` whose origin lies `extent` below the
    queries; random queries, each with a map point straight above it at the largest distance the search still promises to
    cover -- (reach - 1e-6) / 1.0001 for tight table `which` (the bounded search walks the table when Rx <= reach), just
    under the gate radius for the main grid (which = "main", cell_div 1, 2, 3).  Returns (grid exists, number of pairs
    the fp32 cell arithmetic puts more than k cells apart)."""
    rng = np.random.default_rng(seed)
    corners = np.array([[0.0, -extent, 0.0], [4.0, 4.0, 4.0]], F)
    out = []
    for kdiv in ((1, 2, 3) if which == "main" else (2,)):
        g = grid_of(corners, dict(max_sq_dist=gate, cell_div=kdiv, tight_rows=3, x_sub=1), long_map_rule)
        if which == "main":
            grid, reach = axis_grid(g, 1), F(np.sqrt(F(gate))) * F(1.0 - 1e-6)
        else:
            if which >= g["n_tb"]:
                out.append((False, 0))
                continue
            grid, reach = axis_grid(g, 1, which), (g["tables"][which]["reach"] - F(1e-6)) / F(1.0001)
        q = rng.uniform(0.0, 3.0, n_samples).astype(F)
        m = (q + reach).astype(F)
        keep = (m.astype(np.float64) - q.astype(np.float64)) <= np.float64(reach)      # the true distance is inside the bound
        out.append((True, int((np.abs(cell_gap(grid, q[keep], m[keep])) > grid[3]).sum())))
    return any(e for e, _ in out), sum(c for _, c in out)


# ------------------------------------------------------------------------------------------------ pieces
def _plane(rng, lo, size, step, axes=(0, 1, 2), noise=0.004):
    """a noisy square grid of points: axes[0], axes[1] span the plane at lo + [0, size), axes[2] is its normal"""
    u = np.stack(np.meshgrid(np.arange(0, size, step), np.arange(0, size, step)), -1).reshape(-1, 2)
    p = np.zeros((len(u), 3))
    p[:, axes[0]] = lo[axes[0]] + u[:, 0]; p[:, axes[1]] = lo[axes[1]] + u[:, 1]; p[:, axes[2]] = lo[axes[2]]
    return (p + rng.normal(0, noise, p.shape)).astype(F)


def _point_at_d2(q, direction, target, exclude=()):
    """A map point near q + direction * sqrt(target) whose fp32 squared distance to q has exactly the bits of `target`:
    the major coordinate is stepped over neighbouring floats, a minor one tunes the last bits."""
    q = np.asarray(q, F); target = F(target)
    direction = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    base = (q.astype(np.float64) + direction * np.sqrt(np.float64(target))).astype(F)
    i = int(np.argmax(np.abs(direction)))
    j = min((a for a in range(3) if a != i and a not in exclude), key=lambda a: abs(direction[a]))   # (a zero component)
    si = np.arange(-48, 49)[:, None] * np.float64(np.spacing(base[i]))
    sj = np.arange(0, 4097)[None, :] * max(np.float64(np.spacing(base[j])), 2.0e-6)          # (changes d2 by its square only)
    m = np.empty(si.shape[:1] + sj.shape[1:] + (3,), F)
    m[...] = base
    m[..., i] = (np.float64(base[i]) + si).astype(F)
    m[..., j] = (np.float64(base[j]) + sj).astype(F)
    hit = np.argwhere(d2_f32(q, m).view(np.uint32) == target.view(np.uint32))
    if not len(hit):
        raise ValueError("no fp32 point at the requested squared distance")
    best = hit[np.argmin(np.abs(hit[:, 0] - 48) + hit[:, 1])]
    return m[best[0], best[1]].copy()


def _query_and_point(rng, lo, jitter, direction, target):
    """a query in lo + [0, jitter)^3 and its map point at exactly d2 = target (another draw where fp32 has none)"""
    for _ in range(50):
        q = (np.asarray(lo, np.float64) + rng.uniform(0, jitter, 3)).astype(F)
        try:
            return q, _point_at_d2(q, direction, target)
        except ValueError:
            continue
    raise ValueError("no fp32 point at the requested squared distance")


def _next(x, steps):
    x = F(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F(np.inf) if steps > 0 else F(-np.inf))
    return x


_DIRS = [(0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 1), (1, 1, 0), (-1, 0, -1), (0, -1, 1)]


def _closer_four(q, direction, r):
    """four map points around q at 0.2 .. 0.35 r, on offsets that fp32 holds exactly, none along `direction`"""
    d = np.asarray(direction, np.float64)
    perp = np.cross(d, (1.0, 0.3, 0.1) if abs(d[0]) < 0.9 * np.linalg.norm(d) else (0.2, 1.0, 0.1))
    perp /= np.linalg.norm(perp)
    perp2 = np.cross(d / np.linalg.norm(d), perp)
    out = [q + F(np.round(f * r * 4096) / 4096) * v.astype(F) for f, v in ((0.2, perp), (0.25, -perp), (0.3, perp2), (0.35, -perp2))]
    return np.array(out, F)


def _support(rng, lo, size=3.0, step=0.05):
    """a plane patch with scan points on it: enough accepted correspondences for a Gauss-Newton step"""
    plane = _plane(rng, lo, size, step)
    scan = (plane[rng.choice(len(plane), 400, replace=False)] + rng.normal(0, 0.01, (400, 3))).astype(F)
    return plane, scan


def _finish(rng, map_parts, scan_parts, cfg, note):
    """concatenate, permute the map order (ties must not follow the construction order), translate the note's indices"""
    m = np.concatenate(map_parts).astype(F)
    perm = rng.permutation(len(m))
    inv = np.empty(len(m), np.int64); inv[perm] = np.arange(len(m))
    for key in ("fifth", "hinge", "decoy"):
        if key in note:
            note[key] = inv[np.asarray(note[key], np.int64)]
    return m[perm], np.concatenate(scan_parts).astype(F), POSE0.copy(), cfg, note


# ------------------------------------------------------------------------------------------------ builders
def lattice_ties(spacing=0.25, cell_div=2, x_sub=1, aligned=False, seed=0):
    """An exact lattice (coordinates are multiples of 1/8 or 1/16: every d2 is exact, equal distances have equal bits).
    Queries at lattice points, face centres and body centres: up to 6, 12 and 8 candidates tie for the last places of the
    five, and they come from different cells, rows and x buckets.  aligned=True (gate 0.49, cell_size 1.0) puts the cell faces
    of the main grid ON lattice planes for cell_div 1 and 2 (origin = min - cell / 2 = a multiple of 1/4); the tight tables'
    cell (reach * 1.001) is no multiple of the spacing, so their faces cut the lattice at every phase instead."""
    rng = np.random.default_rng(seed)
    n = 17
    ax = np.arange(n) * spacing
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(F)
    half = F(spacing / 2)
    inner = lat[(lat < ax[-1]).all(1)]
    pick = lambda k: inner[rng.choice(len(inner), k, replace=False)]
    scan = np.concatenate([lat[rng.choice(len(lat), 900, replace=False)],                     # lattice points: d2 = 0, then 6 at s^2
                           pick(500) + np.array([half, half, 0], F), pick(250) + np.array([0, half, half], F),
                           pick(250) + np.array([half, 0, half], F),                           # face centres: 4 at s^2/2, 8 next
                           pick(700) + half,                                                   # body centres: 8 at 3 s^2/4
                           lat[rng.choice(len(lat), 200)] + np.array([half, 0, 0], F)])        # edge centres: 2, then 8
    cfg = dict(cell_div=cell_div, x_sub=x_sub)
    if aligned:
        cfg.update(max_sq_dist=0.49, cell_size=1.0)
    note = dict(kind="lattice", spacing=spacing)
    return _finish(rng, [lat], [scan], cfg, note)


def gate_edge(gate=1.0, cell_div=2, seed=1):
    """Per probe query: four close map points and a fifth whose fp32 d2 is exactly the gate, one ulp below, one ulp above
    (`d2_5 < max_sq_dist` is strict: only the middle one passes), along +-y, +-z, +-x and diagonals.  note["fifth"][i] is the
    map index of probe i's fifth point, note["rel"][i] in (-1, 0, +1) its ulp offset from the gate, note["cell_off"][i] the
    largest cell offset of the fifth from its query in the main grid (k = the outermost cell the search visits)."""
    rng = np.random.default_rng(seed)
    gate = F(gate); r = float(np.sqrt(gate))
    plane, sscan = _support(rng, (-8.0, -8.0, -3.0))
    maps, queries, fifth, rel = [plane], [], [], []
    n0 = len(plane)
    pitch = 2.0 * r + 1.5
    for i, (d, e) in enumerate([(d, e) for d in _DIRS for e in (0, -1, 1)]):
        q, m5 = _query_and_point(rng, np.array([i % 6, (i // 6) % 6, i // 36], np.float64) * pitch, 0.4, d, _next(gate, e))
        maps.append(np.concatenate([_closer_four(q, d, r), m5[None]]))
        queries.append(q); rel.append(e); fifth.append(n0 + 5 * i + 4)
    m_all = np.concatenate(maps)
    g = grid_of(m_all, dict(max_sq_dist=gate, cell_div=cell_div))
    q = np.array(queries, F)
    off = np.max([np.abs(cell_gap(axis_grid(g, a), q[:, a], m_all[fifth, a])) for a in range(3)], 0)
    note = dict(kind="gate", fifth=fifth, rel=np.array(rel), probes=np.arange(len(q)) + len(sscan), cell_off=off, gate=gate)
    return _finish(rng, maps, [sscan, q], dict(max_sq_dist=float(gate), cell_div=cell_div), note)


def _dense_patch(rng, size=3.0, step=0.03):
    """the recipe of test_row_tables_follow_the_handle_and_the_map_density, smaller: an auto batch handle builds all three
    tables on it and tries the finest one first"""
    lo = np.zeros(3)
    return np.concatenate([_plane(rng, lo, size, step), _plane(rng, lo + (0, 0, 2.5), size, step)])


def table_edge(bounded=False, seed=2, far_axis=None, extent=0.0):
    """On a dense patch (three tight tables, first try = the finest one for an auto batch handle).

    bounded=False, iteration 0: per table l, probes whose fifth neighbour has d2 exactly tb_try_b2[l], one ulp below (both
    accepted by that table's try) and one ulp above (the try fails, the next table up answers); and probes near the top face
    of their cell with four points in the row and a fifth, farther than the acceptance bound, two cells up in y or in z:
    the try must fail rather than return four.
    bounded=True, iterations 1+: scan points at every height from 2 cm to 0.8 m over the planes and a pose that moves by a
    few centimetres, so that the bound R = sqrt(d5) + movement of the bounded search falls on both sides of each
    tb_reach[l], densely (use tight_rows=3 or an auto batch handle, record_corr_iter=2).  far_axis / extent: one more map point
    `extent` metres down that axis, so that the patch lies at the far end of a long grid -- just under the extent at which
    the long-map rule drops a table, the bounded search walks that table with the least margin it is ever given."""
    rng = np.random.default_rng(seed)
    dense = _dense_patch(rng)
    if bounded:
        base = dense[rng.choice(len(dense), 2800, replace=False)].astype(np.float64)
        h = rng.uniform(0.02, 0.8, (2800, 1)) * np.array([0.0, 0.0, 1.0])
        scan = (base + h + rng.normal(0, 0.003, base.shape)).astype(F)
        scan = np.concatenate([scan, (dense[rng.choice(len(dense), 200)] + rng.normal(0, 0.01, (200, 3))).astype(F)])
        parts = [dense]
        if far_axis is not None:
            parts.append((-extent * np.eye(3)[far_axis])[None].astype(F))
        m, s, _, cfg, note = _finish(rng, parts, [scan], dict(), dict(kind="bounded", extent=extent))
        return m, s, np.array([0.003, -0.002, 0.004, 0.025, -0.02, 0.015], F), cfg, note
    g = grid_of(np.concatenate([dense, [[-1.0, -1.0, -1.0], [9.0, 9.0, 9.0]]]).astype(F), dict(tight_rows=3))
    sscan = (dense[rng.choice(len(dense), 600, replace=False)] + rng.normal(0, 0.01, (600, 3))).astype(F)
    maps, queries, fifth, rel, level = [dense, np.array([[-1.0, -1.0, -1.0], [9.0, 9.0, 9.0]], F)], [], [], [], []
    n0 = len(dense) + 2
    i = 0
    for l in range(3):
        t = g["tables"][l]
        for d in _DIRS[:6]:
            for e in (0, -1, 1):
                q, m5 = _query_and_point(rng, [4.5 + 1.5 * (i % 3), 1.5 * ((i // 3) % 6), 4.5 + 1.5 * (i // 18)], 0.3, d, _next(t["try_b2"], e))
                maps.append(np.concatenate([_closer_four(q, d, float(np.sqrt(t["try_b2"]))), m5[None]]))
                queries.append(q); rel.append(e); level.append(l); fifth.append(n0 + 5 * i + 4)
                i += 1
    # four in the row, the fifth two cells up (y, then z), the query just under the top face of its cell
    for l in range(3):
        t = g["tables"][l]
        for a, o, nn_ in ((1, t["oy"], t["ny"]), (2, t["oz"], t["nz"])):
            q = (np.array([4.5 + 1.5 * (i % 3), 1.5 * ((i // 3) % 6), 4.5 + 1.5 * (i // 18)]) + rng.uniform(0, 0.3, 3)).astype(F)
            c = cell_coord_f32(q[a], o, t["inv_cell"], nn_)
            q[a] = F(np.float64(o) + (c + 0.97) * np.float64(t["cell"]))
            d = np.eye(3)[a]
            up = q.copy(); up[a] = F(np.float64(o) + (c + 2.02) * np.float64(t["cell"]))
            maps.append(np.concatenate([_closer_four(q, d, float(t["reach"])), up[None]]))
            queries.append(q); rel.append(2); level.append(l); fifth.append(n0 + 5 * i + 4)
            i += 1
    q = np.array(queries, F)
    note = dict(kind="table", fifth=fifth, rel=np.array(rel), level=np.array(level), probes=np.arange(len(q)) + len(sscan))
    return _finish(rng, maps, [sscan, q], dict(), note)


def outside_grid(variant="box", gate=1.0, seed=3):
    """Queries outside the map's bounding box: by less than the gate radius and by more, off every face, edge and corner; far
    enough out that lio_cell_coord clamps (-4 / n + 3), up to 1e9 m.  variant "one" / "five": a map of one point, of five."""
    rng = np.random.default_rng(seed)
    r = float(np.sqrt(F(gate)))
    if variant in ("one", "five"):
        m = np.array([[1.0, 2.0, 3.0]], F) if variant == "one" else \
            (np.array([1.0, 2.0, 3.0]) + np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0.05]])).astype(F)
        scan = np.concatenate([m + F(0.01), m[0] + rng.uniform(-0.3, 0.3, (60, 3)), m[0] + rng.uniform(-3, 3, (60, 3)),
                               rng.uniform(-1e6, 1e6, (10, 3))]).astype(F)
        return _finish(rng, [m], [scan], dict(max_sq_dist=gate), dict(kind="outside"))
    size = 4.0
    faces = [_plane(rng, (0.0, 0.0, 0.0), size, 0.05), _plane(rng, (0.0, 0.0, size), size, 0.05),
             _plane(rng, (0.0, 0.0, 0.0), size, 0.05, axes=(0, 2, 1)), _plane(rng, (0.0, size, 0.0), size, 0.05, axes=(0, 2, 1)),
             _plane(rng, (0.0, 0.0, 0.0), size, 0.05, axes=(1, 2, 0)), _plane(rng, (size, 0.0, 0.0), size, 0.05, axes=(1, 2, 0))]
    m = np.concatenate(faces)
    scan = [(m[rng.choice(len(m), 500, replace=False)] + rng.normal(0, 0.01, (500, 3)))]
    for out in (0.5 * r, 0.97 * r, 1.5 * r, 2.6 * r, 7.0, 1.0e4, 1.0e9):
        for s in np.stack(np.meshgrid(*[(-1, 0, 1)] * 3), -1).reshape(-1, 3):                 # 6 faces, 12 edges, 8 corners
            if not s.any():
                continue
            for _ in range(3):
                p = rng.uniform(0.2, size - 0.2, 3)
                p = np.where(s < 0, -out, np.where(s > 0, size + out, p))
                scan.append(p[None])
    return _finish(rng, [m], scan, dict(max_sq_dist=gate), dict(kind="outside"))


def long_strip(axis=1, extent=8200.0, gate=1.0, seed=4, n_probes=8, n_search=200000, compact=False):
    """A corridor `extent` metres long along `axis` and 4 m across: a dense patch at the far end (it only stretches the grid: the
    origin lies `extent` below everything else), a dense patch near the zero end for the registration itself, and probes
    in the empty space between the planes of the near end.

    A probe is a query q, four close map points, a map point m straight up the long axis just inside a search bound, and
    one decoy beside q (off the long axis) that is farther than m and still inside the bound.  The true five are the close
    four and m.  If fp32 cell arithmetic puts m one cell too far, the try finds the close four and the decoy -- five inside
    the bound -- and returns them: the miss shows in the neighbour set.  (With m and only four others a miss would leave four
    in the row, the try would fail and a wider search would repair it: that arrangement cannot show the fault at iteration 0.)
    There is one set of probes per search bound: tight table 0, 1, 2 (acceptance bound sqrt(tb_try_b2[l])) and the main grid
    (the gate).  q is searched for with the emulation under the grid WITHOUT the long-map rule: note["gap"][i] is cell(m) -
    cell(q) there, note["k"][i] the offset the search visits; where the search found no q with gap > k it keeps the
    candidate closest to it.

    Along x the row search takes the run [cell(qx - Rx), cell(qx + Rx)] of fine cells: the table probes of an x strip are
    searched for against that form (k = 0: m beyond the run's last cell).  The LDS-staged search walks cx - k .. cx + k of
    the main grid: the main-grid probes of an x strip are searched for against that form, like those of y and z.
    compact=True: the main-grid probes only, five copies of each and no other scan point -- one workgroup whose cell
    region fits the LDS staging (at most 256 rows, 4096 cells), so that the staged search is what answers."""
    rng = np.random.default_rng(seed)
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    root = float(np.sqrt(F(gate)))

    def put(pa, pb, pc):
        p = np.zeros(np.broadcast(pa, pb, pc).shape + (3,))
        p[..., a] = pa; p[..., b] = pb; p[..., c] = pc
        return p

    zone = n_probes * (1.0 + 1.0 + 1.7 + 2.7) * max(root, 0.7) + 2.0
    lo_near = np.zeros(3); lo_near[a] = -(zone + 6.0)
    lo_far = np.zeros(3); lo_far[a] = -extent
    top = np.zeros(3); top[c] = 4.0
    near = np.concatenate([_plane(rng, lo_near, 4.0, 0.035, axes=(a, b, c)), _plane(rng, lo_near + top, 4.0, 0.035, axes=(a, b, c))])
    far = _plane(rng, lo_far, 4.0, 0.035, axes=(a, b, c))
    corners = np.array([put(-extent, 0.0, 0.0), put(1.5, 4.0, 4.0)], F)
    far[:, a] = np.maximum(far[:, a], F(-extent))              # (the corner point stays the minimum whatever the noise)
    skeleton = np.concatenate([near, far, corners]).astype(F)
    cfg = dict(max_sq_dist=float(gate))
    g = grid_of(skeleton, dict(cfg, max_batch=64), long_map_rule=False)
    bounds = [(l, l, F(np.sqrt(np.float64(g["tables"][l]["try_b2"])))) for l in range(g["n_tb"] - 1, -1, -1)]
    bounds.append(("main", None, F(np.sqrt(F(gate)))))
    if compact:
        bounds = bounds[-1:]
    maps, queries, hinge, decoy, gaps, ks, kinds = [skeleton], [], [], [], [], [], []
    n0, i, pos = len(skeleton), 0, -zone
    for name, tbl, bound in bounds:
        pitch = (1.0 if tbl in (1, 2) else (1.7 if tbl == 0 else 2.7)) * max(root, 0.7)
        fine_x = axis == 0 and tbl is not None
        if fine_x:
            grid = (g["origin"][0], g["inv_cell_x"], g["nxf"], None)
        else:
            grid = axis_grid(g, axis, tbl)
        delta, d_decoy = np.float64(bound) * (1.0 - 1.0e-4), np.float64(bound) * (1.0 - 0.4e-4)
        for _ in range(n_probes):
            qa = rng.uniform(pos + 0.2 * pitch, pos + 0.4 * pitch, n_search).astype(F)
            ma = (qa.astype(np.float64) + delta).astype(F)
            keep = (ma.astype(np.float64) - qa.astype(np.float64)) < d_decoy * (1.0 - 1e-5)
            if fine_x:
                # x: the candidate run ends at cell(qx + Rx); m must not lie beyond it (Rx = the table's reach / the gate reach)
                rx = g["tables"][tbl]["reach"]
                gap = cell_coord_f32(ma, *grid[:3]) - cell_coord_f32(qa + rx, *grid[:3])
                k = 0
            else:
                gap = cell_gap(grid, qa, ma); k = grid[3]
            t = (ma - F(grid[0])) * F(grid[1]) - (qa - F(grid[0])) * F(grid[1])
            score = np.where(keep, gap.astype(np.float64) * 10.0 + t, -np.inf)
            j = int(np.argmax(score))
            q = put(np.float64(qa[j]), 2.0 + rng.uniform(0, 0.2), 2.0 + rng.uniform(0, 0.2)).astype(F)
            m = q.copy(); m[a] = ma[j]
            d = np.eye(3)[a]
            dec = q.copy(); dec[b] = F(np.float64(q[b]) + d_decoy)
            maps.append(np.concatenate([_closer_four(q, d, float(bound)), m[None], dec[None]]))
            queries.append(q); hinge.append(n0 + 6 * i + 4); decoy.append(n0 + 6 * i + 5)
            gaps.append(int(gap[j])); ks.append(k); kinds.append(-1 if tbl is None else tbl)
            i += 1; pos += pitch
    sscan = (near[rng.choice(len(near), 800, replace=False)] + rng.normal(0, 0.01, (800, 3))).astype(F)
    q = np.array(queries, F)
    rep = 1
    if compact:
        sscan, rep = sscan[:0], 5
        q = np.repeat(q, rep, axis=0)
    note = dict(kind="strip", hinge=np.repeat(hinge, rep), decoy=np.repeat(decoy, rep), gap=np.repeat(gaps, rep), k=np.repeat(ks, rep),
                table=np.repeat(kinds, rep), probes=np.arange(len(q)) + len(sscan), bound=[float(x[2]) for x in bounds], axis=axis,
                extent=extent, compact=compact)
    return _finish(rng, maps, [sscan, q], cfg, note)


def _corner_box(rng, dims, cfg):
    """a few points at the corners of the box [0, dims], a plane patch with scan points inside it"""
    corners = np.stack(np.meshgrid(*[(0.0, float(d)) for d in dims]), -1).reshape(-1, 3)
    plane, scan = _support(rng, (1.0, 1.0, 1.0), size=2.0, step=0.1)
    scan = np.concatenate([scan, corners[:4] + 0.3, rng.uniform(0, 1, (50, 3)) * np.array(dims)])
    return _finish(rng, [corners.astype(F), plane], [scan.astype(F)], cfg, dict(kind="size"))


def size_fallbacks(which, seed=5):
    """Maps of a few hundred points whose bounding box alone trips a size rule of lio_plan_grid / lio_plan_tables.  note["expect"] = what
    grid_of must give (and the device profile report): grow_steps, n_tb.
      grow1 / grow3   the `cell *= 1.5` loop runs once / three times (cells * x_sub > 256 Mi)
      below64 / above64   n_cells * x_sub just below / just above 64 Mi: one tight table / none
      third192        tight_rows = 3: the first two tables fit, the third alone trips the 192 Mi-bucket cap
    Every side stays under a kilometre, so the long-map rule does not interfere."""
    rng = np.random.default_rng(seed)
    if which == "grow1":
        dims, cfg, expect = (350.0, 350.0, 350.0), dict(), dict(grow_steps=1, n_tb=0)
    elif which == "grow3":
        dims, cfg, expect = (800.0, 800.0, 800.0), dict(), dict(grow_steps=3, n_tb=0)
    elif which in ("below64", "above64"):
        cfg = dict(tight_rows=1)
        side = 202.0                       # 405 or 406 cells of 0.5005 m on the two equal sides; the third side is tuned
        n_side = grid_of(np.array([[0, 0, 0], [side] * 3], F), cfg)["nx"]
        want = int(64 * MI // (n_side * n_side)) + (1 if which == "above64" else 0)
        third = (want - 2 + 0.3) * 0.5005
        dims, expect = (side, side, third), dict(grow_steps=0, n_tb=1 if which == "below64" else 0)
    elif which == "third192":
        dims, cfg, expect = (10.0, 500.0, 500.0), dict(tight_rows=3), dict(grow_steps=0, n_tb=2)
    else:
        raise KeyError(which)
    m, s, p, cfg, note = _corner_box(rng, dims, cfg)
    note["expect"] = expect
    return m, s, p, cfg, note


# ------------------------------------------------------------------------------------------------ the list
STRIP_EXTENTS = (900.0, 3000.0, 8200.0, 17000.0)
STRIP_GATES = (1.0, 0.49)


def all_cases():
    """name -> (builder, kwargs); the tests parametrise over the names and build each case once."""
    cases = {}
    for sp, kd, xs in ((0.25, 1, 1), (0.125, 2, 4), (0.25, 3, 8), (0.125, 1, 8), (0.25, 2, 1), (0.125, 3, 4)):
        cases[f"lattice_{sp}_k{kd}_x{xs}"] = (lattice_ties, dict(spacing=sp, cell_div=kd, x_sub=xs))
    cases["lattice_aligned_k1"] = (lattice_ties, dict(spacing=0.25, cell_div=1, x_sub=4, aligned=True))
    cases["lattice_aligned_k2"] = (lattice_ties, dict(spacing=0.125, cell_div=2, x_sub=1, aligned=True))
    for gate in (0.49, 1.0, 4.0):
        cases[f"gate_{gate}"] = (gate_edge, dict(gate=gate))
    cases["table_edge"] = (table_edge, dict())
    cases["table_bounded"] = (table_edge, dict(bounded=True))
    for v in ("box", "one", "five"):
        cases[f"outside_{v}"] = (outside_grid, dict(variant=v))
    for axis in (1, 2, 0):
        for extent in STRIP_EXTENTS:
            for gate in STRIP_GATES:
                cases[f"strip_{'xyz'[axis]}_{int(extent)}_g{gate}"] = (long_strip, dict(axis=axis, extent=extent, gate=gate))
    for extent in STRIP_EXTENTS:                                   # x strips for the LDS-staged search (cx - k .. cx + k)
        for gate in STRIP_GATES:
            cases[f"strip_x_{int(extent)}_g{gate}_compact"] = (long_strip, dict(axis=0, extent=extent, gate=gate, compact=True))
    for axis in (1, 2):                                            # the bounded search just under each table's last extent
        for extent in (1000.0, 2040.0, 4090.0):
            cases[f"strip_bounded_{'xyz'[axis]}_{int(extent)}"] = (table_edge, dict(bounded=True, far_axis=axis, extent=extent))
    for w in ("grow1", "grow3", "below64", "above64", "third192"):
        cases[f"size_{w}"] = (size_fallbacks, dict(which=w))
    return cases


_BUILT = {}


def build_case(name):
    """the case, built once per process and handed out unchanged (callers must not write into the arrays)"""
    if name not in _BUILT:
        fn, kw = all_cases()[name]
        out = fn(**kw)
        for arr in out[:3]:
            arr.setflags(write=False)
        _BUILT[name] = out
    return _BUILT[name]
