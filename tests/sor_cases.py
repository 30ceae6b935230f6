"""Designed inputs for the outlier filter (lio_sor_filter, csrc/lio_localmap.hip): the edges of its shell walk (sor_nearest),
of who takes part, of its statistics and of its workgroup hand-off.  numpy only.
build_case(name) -> (cloud [n, 4] float32, mean_k, stddev_mul, note); every case is seeded, built once and cached.
tests/test_sor_cases_cpu.py proves on the restatement alone (localmap_restate: knn_d2, sor_grid, walk) that a case hits what it
names; tests/test_gpu_sor_edges.py runs them on the device.  n <= 2000 except wg_257, the size case.

"Framed" clouds (shell_exit*, cell_edges) touch the six faces of the box [0, 32]^3 and are padded until they hold 4 m points
in 3 m cells of the trial grid (edge 32 / 64 = 0.5).  At mean_k 3 the filter asks for float32(4) / float32(3) points per occupied
cell, points per occupied cell is float32(4 m) / float32(3 m) -- the same bits -- so the edge is exactly 0.5, inv_cell 2, the
grid 65^3 with its origin at 0 and a cell index is the integer part of twice the coordinate: shells can be designed by hand,
and the grid does not move with the probes (the builders assert that on sor_grid itself).

Every case must leave the restatement's threshold bracket empty (test_sor_cases_cpu.py asserts it), so that kept sets are
compared as sets.  Three inputs cannot, and say so in their note (bracket="sign"): equal_spacing_nan, equal_spacing_zero and
one_cell_copies have every dist_i equal, hence a NaN threshold or one equal to every dist_i; for them the condition is that
no order of summation can change the sign of the variance (the sums are exact, or the rounding of dist * dist outweighs any
fp64 summation error a thousandfold)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_restate as L   # noqa: E402
from icp_restate import grid_cells   # noqa: E402

F = np.float32
FLT_MAX = np.finfo(np.float32).max
INF = F(np.inf)
FRAME = np.array([[0, 13, 29], [32, 7, 3], [11, 0, 21], [19, 32, 9], [5, 27, 0], [23, 17, 32]], np.float32)
AXES = [(a, s) for a in range(3) for s in (1, -1)]
FAR = np.array([5.0e5, -3.0e5, 100.0])
_CACHE = {}


def xyzi(xyz, seed):
    xyz = np.asarray(xyz, F)
    w = np.random.default_rng(seed).uniform(0, 255, (len(xyz), 1)).astype(F)
    return np.concatenate([xyz[:, :3], w], 1)


def up(v, k=1):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, INF if k > 0 else -INF)
    return v


def d2_of(q, p):
    """The kernel's fp32 squared distance ((dx dx) + dy dy) + dz dz."""
    q, p = np.asarray(q, F), np.asarray(p, F)
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return ((dx * dx) + dy * dy) + dz * dz


def same_grid(G, H):
    return all(np.array_equal(np.asarray(G[k]), np.asarray(H[k])) for k in G)


# ------------------------------------------------------------------------------------------------------------------ framed
def framed(points, mean_k=3):
    """FRAME + points + padding so that n = 4 m and the occupied cells of the trial grid are 3 m.  The padding lives in the
    block [25, 31)^3, which the designed points leave free: one point per new cell, then second and third points in those
    cells.  -> (xyz float32, G) with G held to edge 0.5 at the origin."""
    assert mean_k == 3
    body = np.concatenate([FRAME, np.asarray(points, F).reshape(-1, 3)], 0)
    assert body.min() >= 0 and body.max() <= 32 and not ((body > 24.5) & (body < 31.5)).all(1).any()
    cells = np.floor(body.astype(np.float64) * 2).astype(np.int64)
    n0, occ0 = len(body), len(np.unique(cells, axis=0))
    m = max((occ0 + 3) // 3, n0 - occ0)
    singles, extra = 3 * m - occ0, m - n0 + occ0
    assert singles >= 1 and 0 <= extra <= 3 * singles and singles <= 1728
    j = np.arange(singles)
    pad = np.stack([25.25 + 0.5 * (j % 12), 25.25 + 0.5 * ((j // 12) % 12), 25.25 + 0.5 * (j // 144)], 1)
    j = np.arange(extra)
    more = pad[j % singles] + np.stack([0.0625 * (1 + j // singles), 0 * j, 0 * j], 1)
    xyz = np.concatenate([body, pad.astype(F), more.astype(F).reshape(-1, 3)], 0)
    G = L.sor_grid(xyz, mean_k)
    assert len(xyz) == 4 * m and G["occupied"] == 3 * m, (len(xyz), G["occupied"], m)
    assert G["edge"] == F(0.5) and G["inv_cell"] == F(2) and not G["origin"].any() and (G["nx"], G["ny"], G["nz"]) == (65, 65, 65)
    return xyz, G


def _place(q, a, s, b, target):
    """A point at q + s * dx along axis a and a small dy along axis b whose fp32 d2 from q is exactly `target`."""
    q = np.asarray(q, F)
    t = np.float64(target)
    for dy0 in (0.002, 0.003, 0.0045, 0.001):
        p = q.copy()
        p[a] = F(np.float64(q[a]) + s * np.sqrt(t - dy0 * dy0))
        dx = q[a] - p[a]
        rem = t - np.float64(dx * dx)
        if rem <= 0:
            continue
        pb = F(np.float64(q[b]) + np.sqrt(rem))
        for u in sorted(range(-3000, 3001), key=abs):
            p[b] = up(pb, u) if abs(u) < 2 else F(pb + F(u) * np.spacing(pb))
            if d2_of(q, p) == F(target):
                return p
    raise AssertionError("no point with that squared distance")


def exit_bound(G, q, r):
    """What sor_nearest compares its worst entry with before shell r: ((r - 1) e - slack)^2 * 0.99999f in fp32."""
    e, o = F(G["edge"]), np.asarray(G["origin"], F)
    span = max(max(abs(q[0] - o[0]), abs(q[1] - o[1])), abs(q[2] - o[2]))
    slack = F(1.0e-3) * e + F(1.0e-5) * span
    lb = F(r - 1) * e - slack
    return lb * lb * F(0.99999)


def shell_exit(mirror=False):
    """Framed, mean_k 3 (a list of four: the query, A1, A2 and the contested last entry).  One probe per axis direction and
    r in {2, 3}, each in a lane of its own, 8 apart.  The query sits 2^-12 inside the face of its cell that looks along the
    axis.  T = the bound of the exit test before shell r for this query.
    plain:  A3, against the axis in shell 0 or 1, has d2 = T exactly -- the largest worst entry with which the walk may
            still leave before shell r -- and N, along the axis in shell r - 1, has d2 one ulp below T: N is the true third
            neighbour.  For r = 3 a bound one shell too generous ("one_shell_early") leaves before N's shell 2 and keeps A3.
            The walk ends before shell r (shells = r).
    mirror: A3 has d2 one ulp above T and N one ulp above that: the list keeps A3, the test before shell r fails by one ulp
            and the walk goes through shell r (shells = r + 1)."""
    pts, probes = [], []
    slots = [(6.0, 6.0), (6.0, 14.0), (6.0, 22.0), (14.0, 6.0), (14.0, 14.0), (14.0, 22.0),
             (22.0, 6.0), (22.0, 14.0), (22.0, 22.0), (14.0, 10.0), (22.0, 10.0), (6.0, 10.0)]
    G0 = dict(edge=F(0.5), origin=np.zeros(3, F))
    delta = 2.0 ** -12
    for j, (r, (a, s)) in enumerate([(r, ax) for r in (2, 3) for ax in AXES]):
        b, c = (a + 1) % 3, (a + 2) % 3
        q = np.zeros(3, F)
        q[a] = F(16.0 + (0.5 - delta if s > 0 else delta))
        q[b], q[c] = F(slots[j][0] + 0.25), F(slots[j][1] + 0.25)
        T = exit_bound(G0, q, r)
        W = up(T) if mirror else T
        A1, A2 = q.copy(), q.copy()
        A1[c] += F(0.0625); A2[c] -= F(0.09375)
        A3 = _place(q, a, -s, b, W)
        N = _place(q, a, s, b, up(W, 1 if mirror else -1))
        i0 = len(FRAME) + len(pts)
        pts += [q, A1, A2, A3, N]
        probes.append(dict(q=i0, A3=i0 + 3, N=i0 + 4, r=r, axis=a, sign=s, T=T, shells=r + 1 if mirror else r))
    xyz, G = framed(pts)
    cells = grid_cells(G, xyz)
    for p in probes:                                              # the shells the points were designed for
        cq = cells[p["q"]]
        assert np.abs(cells[p["N"]] - cq).max() == p["r"] - 1 and np.abs(cells[p["A3"]] - cq).max() <= 1
        assert np.abs(cells[p["q"] + 1:p["q"] + 3] - cq).max() == 0
        assert exit_bound(G, xyz[p["q"]], p["r"]) == p["T"]
    note = dict(what="shell_exit", probes=probes, mirror=mirror, wrong=None if mirror else "one_shell_early", grid=G)
    return xyzi(xyz, 201 + mirror), 3, 1.0, note


def cell_edges():
    """Framed, mean_k 3.  Per axis, groups of points at ox + k e (0, 16 and 32 = the box's maximum, the last cell nx - 1 = 64 by
    the shared formula): the boundary itself, one ulp below and one ulp above where the box allows it (nothing lies below its
    minimum or above its maximum).  A group's members are each other's nearest neighbours across the boundary, and each group
    has a partner 0.4375 away along the axis, in the neighbouring cell.  Then the corner (32, 32, 32) with its three one-ulp
    neighbours, and the origin corner."""
    pts, groups = [], []
    lane = 0
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k, ulps in ((0.0, (0, 1)), (16.0, (-1, 0, 1)), (32.0, (-1, 0))):
            o1, o2 = 2.25 + 4 * (lane % 6), 2.25 + 4 * (lane // 6)
            lane += 1
            i0 = len(FRAME) + len(pts)
            for u in ulps:
                p = np.zeros(3, F)
                p[a] = up(F(k), u) if k else F(u) * F(2.0 ** -149)
                p[b], p[c] = o1, o2
                pts.append(p)
            t = np.zeros(3, F)
            t[a] = k - 0.4375 if k else 0.4375
            t[b], t[c] = o1, o2
            pts.append(t)
            groups.append(dict(first=i0, n=len(ulps), axis=a, k=int(k * 2), ulps=ulps))
    top = F(32.0)
    i0 = len(FRAME) + len(pts)
    pts += [[top, top, top], [up(top, -1), top, top], [top, up(top, -1), top], [top, top, up(top, -1)]]
    groups.append(dict(first=i0, n=4, axis=None, k=64, ulps=None))
    i0 = len(FRAME) + len(pts)
    tiny = F(2.0 ** -149)
    pts += [[0, 0, 0], [tiny, 0, 0], [0, tiny, 0], [0, 0, tiny]]
    groups.append(dict(first=i0, n=4, axis=None, k=0, ulps=None))
    xyz, G = framed(np.array(pts, F))
    for g in groups:
        g["ids"] = list(range(g["first"], g["first"] + g["n"]))
    cells = grid_cells(G, xyz)
    for g in groups:                                              # the boundary point opens cell k, the point below it closes k - 1
        if g["axis"] is not None:
            got = [int(cells[i, g["axis"]]) for i in g["ids"]]
            assert got == [g["k"] + (-1 if u < 0 else 0) for u in g["ulps"]], (g, got)
    assert cells.max() == 64 and cells.min() == 0
    note = dict(what="cell_edges", groups=groups, grid=G)
    return xyzi(xyz, 203), 3, 1.0, note


# ------------------------------------------------------------------------------------------------------------ slack_origin
def _first_in(G, c, y, z):
    """The smallest fp32 x whose computed x cell is >= c (the cell formula is monotone in x)."""
    def cell(x):
        return grid_cells(G, np.array([[x, y, z]], F))[0, 0]
    lo = F(np.float64(G["origin"][0]) + (c - 1) * np.float64(G["edge"]))
    hi = F(np.float64(G["origin"][0]) + (c + 1) * np.float64(G["edge"]))
    assert cell(lo) < c <= cell(hi)
    while np.nextafter(lo, INF) < hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if cell(mid) >= c:
            hi = mid
        else:
            lo = mid
    return hi


def slack_origin():
    """Where the slack of the exit bound is needed: a cloud that straddles the coordinate origin, x from -90 to +10, mean_k 1.
    The grid's origin is ox = -90 and its edge sits at the clamp ext / 500 = 0.2 (every filler location is repeated 64
    times, so points per occupied trial cell stay far above 61 * 2/3 whatever the probes do): 501 cells along x.  Near
    x = +2 .. +10 the floats are 2.4e-7 .. 9.5e-7 apart, but (x - ox) is rounded at the spacing of 92 .. 100 (7.6e-6) and its
    product with inv_cell at that of 460 .. 500: computed boundaries of neighbouring cells come closer together than e by
    more than the 5e-6 e which the factor 0.99999 gives away.  The builder takes, among the x cells 460 .. 497, the pair of
    boundaries (c + 1, c + 2) with the shortest gap; q is the last float of cell c, p the first float of cell c + 2 (shell 2,
    the true nearest); X, off along y in a cell of shell <= 1, has its fp32 d2 between d2(p) and e^2 * 0.99999f.  An exit
    bound of (r - 1) e without the slack leaves before shell 2 and answers X."""
    rng = np.random.default_rng(214)
    locs = np.stack([np.linspace(-88.0, 9.0, 28), rng.uniform(0.2, 1.8, 28), rng.uniform(0.2, 1.8, 28)], 1)
    frame = np.array([[-90.0, 0, 0], [10.0, 2, 2]])
    y = z = 1.0

    def cloud(p, X, qx):
        keep = np.abs(locs[:, 0] - qx) > 1.5                   # nothing else near the probe
        fill = np.repeat(locs[keep], 64, 0)
        return np.concatenate([frame, fill, [[qx, y, z], p, X]], 0).astype(F)

    G = L.sor_grid(cloud([5.0, y, z], [5.0, y + 0.2, z], 5.0), 1)
    assert G["nx"] == 501 and G["edge"] == F(100.0) / F(500.0)
    e = np.float64(G["edge"])
    best = None
    for c in range(460, 498):
        b1, b2 = _first_in(G, c + 1, y, z), _first_in(G, c + 2, y, z)
        q = np.nextafter(b1, -INF)
        gap = np.float64(b2) - np.float64(q)
        if best is None or gap < best[0]:
            best = (gap, c, q, b2)
    gap, c, qx, px = best
    lim = F(G["edge"] * G["edge"]) * F(0.99999)                 # what the exit compares the worst d2 with when slack = 0
    d2p = d2_of([qx, y, z], [px, y, z])
    note = dict(what="slack_origin", c=c, gap=float(gap), edge=float(e), margin=float(1.0 - gap / e),
                decides=bool(np.float64(d2p) < np.float64(lim)), wrong="no_slack", r=2)
    if not note["decides"]:                                       # (kept as a plain exactness case, the margin recorded)
        Xy = F(y + 0.2)
    else:
        want = (np.float64(d2p) + np.float64(lim)) / 2
        Xy = F(y + np.sqrt(want))
        assert d2p < d2_of([qx, y, z], [qx, Xy, z]) <= lim
    xyz = cloud([px, y, z], [qx, Xy, z], np.float64(qx))
    n = len(xyz)
    note.update(q=n - 3, P=n - 2, X=n - 1, grid=G)
    assert same_grid(G, L.sor_grid(xyz, 1)), "the grid moved with the probes"
    return xyzi(xyz, 214), 1, 1.0, note


# -------------------------------------------------------------------------------------------------------- plain geometry
def lattice_ties(mean_k):
    """9^3 lattice, spacing 0.5, shuffled, one point twice.  An interior point has 6 neighbours at 0.5, 12 at sqrt(0.5), 8 at
    sqrt(0.75): at mean_k 6 the list is exactly full with the first ring while equal distances wait in later shells; at
    mean_k 10 its worst entry ties with 8 points it leaves out.  The result is a function of the multiset only."""
    rng = np.random.default_rng(202)
    g = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * 0.5
    pts = np.concatenate([g, g[[364]]], 0)
    pts = pts[rng.permutation(len(pts))]
    return xyzi(pts, 202), mean_k, 1.0, dict(what="lattice_ties")


def _n513():
    rng = np.random.default_rng(205)
    return rng.uniform(-6, 6, (513, 3)) * np.array([1, 1, 0.2])


def big_coords():
    """300 ordinary points in [-8, 8]^2 x [-1.6, 1.6] and four records with a coordinate beyond 1e15 m: they are finite, the crop would keep them,
    the filter leaves them out (NaN mean_dist, dropped, not counted).  The first sits outside the cloud on its other two axes:
    the box is taken per axis, so it widens the box in y and z and still takes no part.  note["clean"]: the cloud without them."""
    rng = np.random.default_rng(206)
    body = (rng.uniform(-8, 8, (300, 3)) * np.array([1, 1, 0.2])).astype(F)
    bad = np.array([[1.0e16, 12.0, -11.0], [0.25, -3.0e20, 0.25], [0.25, 0.25, FLT_MAX], [np.nextafter(F(1.0e15), INF), 0.5, 0.5]], F)
    xyz = np.concatenate([bad[:1], body[:100], bad[1:3], body[100:], bad[3:]], 0)
    cloud = xyzi(xyz, 206)
    bad_ids = np.array([0, 101, 102, 303])                     # by construction, not by the restatement's mask
    ok = np.ones(len(xyz), bool)
    ok[bad_ids] = False
    assert np.isfinite(xyz).all() and (np.abs(xyz[ok]) < 10).all() and (np.abs(xyz[~ok]).max(1) > 1.0e15).all()
    return cloud, 10, 1.0, dict(what="big_coords", bad=bad_ids, clean=cloud[ok])


def big_coords_edge():
    """A point at exactly +1e15 m does take part: the box is 1e15 m long, at mean_k 1 the edge sits at the clamp ext / 500 and
    the 300 ordinary points share one cell; the far point walks all 500 shells.  Its neighbour one ulp beyond 1e15 takes no
    part."""
    rng = np.random.default_rng(207)
    body = (rng.uniform(-8, 8, (300, 3)) * np.array([1, 1, 0.2])).astype(F)
    edge = np.array([[F(1.0e15), 0.5, -0.5], [np.nextafter(F(1.0e15), INF), 0.5, 0.5]], F)
    xyz = np.concatenate([body[:150], edge, body[150:]], 0)
    cloud = xyzi(xyz, 207)
    ok = np.ones(len(xyz), bool)
    ok[151] = False
    assert xyz[150, 0] == F(1.0e15) and xyz[151, 0] > F(1.0e15) and np.isfinite(xyz).all()
    return cloud, 1, 1.0, dict(what="big_coords_edge", bad=np.array([151]), clean=cloud[ok], far=150)


def far_offset():
    """A 513-point cloud (two workgroups and a point) 5e5 m from the coordinate origin: one ulp is 0.03 .. 0.06 m there."""
    return xyzi((_n513() + FAR).astype(F), 208), 10, 1.0, dict(what="far_offset")


def long_thin():
    """4 km x 2 m x 0.4 m, 800 points: the grid is one row of cells."""
    rng = np.random.default_rng(209)
    pts = rng.uniform(0, 1, (800, 3)) * np.array([4000.0, 2.0, 0.4]) + np.array([-1200.0, 3.0, 0.0])
    return xyzi(pts, 209), 10, 1.0, dict(what="long_thin")


def one_cell_tiny():
    """40 points inside an extent <= 1e-6 m: no trial grid is laid (occupied -1), edge 1, one cell."""
    rng = np.random.default_rng(210)
    base = np.array([1.0, 2.0, 3.0], F)
    pts = np.stack([up(base[0], 0) + F(2.0 ** -23) * rng.integers(0, 8, 40).astype(F),
                    base[1] + F(2.0 ** -22) * rng.integers(0, 4, 40).astype(F),
                    base[2] + F(2.0 ** -22) * rng.integers(0, 4, 40).astype(F)], 1).astype(F)
    assert (pts.max(0) - pts.min(0)).max() <= 1.0e-6
    return xyzi(pts, 210), 10, 1.0, dict(what="one_cell_tiny")


def one_cell_copies():
    """40 copies of one point: every dist_i is 0, the sums are exactly 0, var 0, threshold 0, all kept (0 <= 0).  Every dist_i
    equals the threshold, so the bracket rule cannot hold; all sums are exact zeros in any order instead."""
    pts = np.tile(np.array([[4.5, -2.25, 0.75]], F), (40, 1))
    return xyzi(pts, 211), 10, 1.0, dict(what="one_cell_copies", bracket="sign")


def equal_spacing(spacing):
    """257 pairs (514 points: two workgroups and a pair) on a 16 m lattice, mean_k 1: every point's neighbour is its partner at
    the same float d, so every dist_i is d and var = (sq_sum - sum^2 / n) / (n - 1) has the sign of fl32(d * d) - d^2.
    d = 1 + 3 * 2^-12: d * d = 1 + 6 * 2^-12 + 9 * 2^-24 rounds DOWN (a tie, to even): var < 0, a NaN threshold, nothing kept.
    d = 0.3125: d * d is exact and so is every partial sum (d has 3 significant bits): var is exactly 0 in any order of
    summation, the threshold is d, all 514 kept.  The bracket rule cannot hold here (every dist_i equals the threshold, or it
    is NaN); the sign condition replaces it and tests/test_sor_cases_cpu.py asserts it."""
    i = np.arange(257)
    a = np.stack([16.0 * (i % 17), 16.0 * (i // 17), np.zeros(257)], 1)
    b = a + np.array([spacing, 0.0, 0.0])
    pts = np.empty((514, 3))
    pts[0::2], pts[1::2] = a, b
    assert np.array_equal(pts.astype(F).astype(np.float64), pts)
    return xyzi(pts, 212), 1, 1.0, dict(what="equal_spacing", d=F(spacing), bracket="sign")


def crowded_cells(mean_k):
    """Three clusters of 300 points with sigma 0.02 m and 150 scattered points over 60 m: the trial grid sees a handful of
    crowded cells, the edge is coarse; a cluster point fills its list (33 entries at mean_k 32) from one cell, a scattered one
    walks tens of shells."""
    rng = np.random.default_rng(213)
    centres = np.array([[-5.0, 3.0, 0.5], [7.0, -4.0, 0.2], [0.5, 0.5, 1.0]])
    pts = np.concatenate([c + rng.normal(0, 0.02, (300, 3)) for c in centres] +
                         [rng.uniform(-30, 30, (150, 3)) * np.array([1, 1, 0.1])], 0)
    pts = pts[rng.permutation(len(pts))]
    return xyzi(pts, 213), mean_k, 1.0, dict(what="crowded_cells")


def wg_257():
    """THE SIZE CASE, not the workload's size: 65 793 points = 257 workgroups + 1 point, the first size at which k_sor_stats
    takes the second stride of its loop, lio_wg_scan_in_place its second chunk and the compaction more than 256 counts.  A
    jittered planar lattice, mean_k 1.  Its reference comes from knn_d2_fast; the walk is not emulated."""
    rng = np.random.default_rng(215)
    n = 257 * 256 + 1
    i = np.arange(n)
    pts = np.stack([0.25 * (i % 257), 0.25 * (i // 257), np.zeros(n)], 1) + rng.uniform(-0.08, 0.08, (n, 3)) * np.array([1, 1, 0.25])
    pts = pts[rng.permutation(n)]
    return xyzi(pts, 215), 1, 1.0, dict(what="wg_257", large=True)


CASES = {
    "slack_origin": slack_origin,
    "shell_exit": shell_exit,
    "shell_exit_mirror": lambda: shell_exit(mirror=True),
    "cell_edges": cell_edges,
    "lattice_ties_k6": lambda: lattice_ties(6),
    "lattice_ties_k10": lambda: lattice_ties(10),
    "big_coords": big_coords,
    "big_coords_edge": big_coords_edge,
    "far_offset": far_offset,
    "long_thin": long_thin,
    "one_cell_tiny": one_cell_tiny,
    "one_cell_copies": one_cell_copies,
    "equal_spacing_nan": lambda: equal_spacing(1.0 + 3.0 * 2.0 ** -12),
    "equal_spacing_zero": lambda: equal_spacing(0.3125),
    "crowded_cells_k32": lambda: crowded_cells(32),
    "crowded_cells_k1": lambda: crowded_cells(1),
    "wg_257": wg_257,
}
NAMES = list(CASES)
WALKED = [n for n in NAMES if n != "wg_257"]


def build_case(name):
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def reference(name):
    """The restatement's answer for one case, computed once (wg_257: through knn_d2_fast)."""
    key = ("ref", name)
    if key not in _CACHE:
        cloud, k, mul, note = build_case(name)
        _CACHE[key] = L.sor(cloud, k, mul, knn=L.knn_d2_fast if note.get("large") else L.knn_d2)
    return _CACHE[key]
