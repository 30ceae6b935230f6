"""Designed inputs for the loop-closure ICP (lio_icp.hip): the edges of its shell search, its rigid step, its convergence
criteria and its workgroup hand-off.  build_case(name) -> (src, tgt, cfg overrides, guess, note); every case is seeded.
tests/test_icp_cases_cpu.py proves on the restatement alone (icp_restate, grid_of) that a case hits what it names;
tests/test_gpu_icp_edges.py runs them on the device.

Most targets are "framed": six points that touch the six faces of the box [0, 32]^3 and designed points of which no two
share a cell of the trial grid (edge 0.5).  Then points-per-occupied-cell is exactly 1, the edge is 0.5 * sqrt(4) = 1,
inv_cell = 1, the grid is 33^3 and cell indices are the integer parts: shells can be designed by hand (the CPU test holds
grid_of to exactly that for every framed case, and cell_edges takes its boundaries from grid_of itself).  Coordinates are small
multiples of powers of two, so every fp32 distance below is exact unless a note says otherwise."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restate as R   # noqa: E402

F = np.float32
FLT_MAX = np.finfo(np.float32).max
FRAME = np.array([[0, 13, 29], [32, 7, 3], [11, 0, 21], [19, 32, 9], [5, 27, 0], [23, 17, 32]], np.float32)
FAR = np.array([2.0e5, -3.0e5, 1.0e3], np.float32)          # far_origin's translation
AXES = [(a, s) for a in range(3) for s in (1, -1)]


def framed(points):
    return np.concatenate([FRAME, np.asarray(points, np.float32).reshape(-1, 3)], 0)


def unit(a, s=1.0):
    v = np.zeros(3)
    v[a] = s
    return v


def ulp_steps(v, k):
    """v moved by k fp32 ulps (k may be negative)."""
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


# ---------------------------------------------------------------------------------------------------------------- search
def lattice_ties(shift=None):
    """13^3 lattice, spacing 0.5, shuffled, one point twice; queries at centres of lattice cells (8 tied), of faces (4) and
    of edges (2).  edge = 6/32 * sqrt(4 * 2197/2198): lattice and grid are not aligned, tied points fall into different
    shells."""
    rng = np.random.default_rng(101)
    g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * 0.5
    tgt = np.concatenate([g, g[[700]]], 0)
    tgt = tgt[rng.permutation(len(tgt))]
    base = rng.integers(0, 12, (900, 3)).astype(np.float64) * 0.5
    kind = np.repeat([3, 2, 1], 300)                         # how many coordinates sit at a half step
    src = base.copy()
    for i, k in enumerate(kind):
        ax = rng.permutation(3)[:k]
        src[i, ax] += 0.25
    dup = g[700]
    src = np.concatenate([src, [dup, dup + [0.25, 0, 0], dup + [0.25, 0.25, 0.25]]], 0)
    mult = np.concatenate([2 ** kind, [2, 3, 9]])           # the duplicate counts twice where it is among the tied ...
    off = np.abs(src[:900] - dup)                            # ... which it also is for a drawn query half a step from it on its half-step axes only
    mult[:900] += ((off == 0.25) | (off == 0)).all(1) & ((off == 0.25).sum(1) == kind)
    if shift is not None:
        src, tgt = src + shift.astype(np.float64), tgt + shift.astype(np.float64)
    note = dict(what="ties", multiplicity=mult, min_multi_shell=50)
    return src.astype(F), tgt.astype(F), dict(max_iters=1), None, note


def cell_edges(shift=None):
    """Framed.  Probes at ox + k e (ox and e from grid_of), one ulp below, one above, for k = 0, 16, 33 = nx, on each axis and
    on all three; each axis probe has a target point 1 - 2^-10 away on the low side or 1 + 2^-10 away on the high side, in the neighbouring cell."""
    pts, src, probes = [], [], []
    lane = 0
    for k in (0, 16, 33):
        for a in range(3):
            for far in (False, True):
                o1, o2 = 2.5 + 4 * (lane % 7), 2.5 + 4 * (lane // 7)
                lane += 1
                b, c = (a + 1) % 3, (a + 2) % 3
                q = np.zeros(3); q[a] = k; q[b] = o1; q[c] = o2
                d = 1.0 + 2.0 ** -10 if far else 1.0 - 2.0 ** -10
                if k == 33 and not far:
                    d = 1.0                                      # (the box ends at 32: the point on its face, in cell 32)
                t = q.copy()
                t[a] = k + d if (far and k < 33) else k - d
                if t[a] < 0:
                    t[a] = k + d
                pts.append(t)
                for u in (-1, 0, 1):
                    p = q.astype(F)
                    p[a] = ulp_steps(F(k), u) if k else (F(0) if u == 0 else F(u) * F(2.0 ** -149))
                    probes.append(dict(src=len(src), axes=[a], k=k, ulp=u))
                    src.append(p)
        q = np.full(3, float(k))
        t = q + (1 + 2.0 ** -10) * (1 if k == 0 else -1) * np.array([1.0, 0.25, 0.25])
        t = np.clip(t, 0, 32)
        pts.append(t)
        for u in (-1, 0, 1):
            p = np.array([ulp_steps(F(k), u) if k else (F(0) if u == 0 else F(u) * F(2.0 ** -149))] * 3, F)
            probes.append(dict(src=len(src), axes=[0, 1, 2], k=k, ulp=u))
            src.append(p)
    tgt = framed(pts).astype(np.float64)
    src = np.array(src, np.float64)
    if shift is not None:
        tgt = (tgt + shift).astype(F).astype(np.float64)
        src = src + shift.astype(np.float64)
    # the probes sit at ox + k e of the grid that grid_of lays over this very target (one ulp at the far origin is
    # 2^-6 .. 2^-5, at the near one a denormal for k = 0), in fp32 arithmetic
    G = R.grid_of(tgt.astype(F))
    for p in probes:
        for a in p["axes"]:
            src[p["src"], a] = ulp_steps(G["origin"][a] + F(p["k"]) * G["edge"], p["ulp"])
    note = dict(what="cell_edges", probes=probes, edge=1.0, origin=np.zeros(3) if shift is None else shift.astype(np.float64),
                n_frame=len(FRAME))
    return src.astype(F), tgt.astype(F), dict(max_iters=1), None, note


def _shell_exit_points(mirror):
    """One probe per axis direction (+-x, +-y, +-z) and r in 1..3, each in a lane of its own.  The query sits 1/16 inside the
    face of its cell c that looks along the axis.  C, the nearest, lies r + 2 cells along the axis at d = r + 1.125; B in a
    shell-(r + 1) cell (r + 1 cells along the axis, off to the side) at d + 2^-6; A in a shell-r cell on the far side (r
    cells against the axis, off to two sides) at d + 2^-5: the walk meets A, then B, then C, and must not stop before C.
    mirror: C moves into the query's own cell or its neighbour (d = 3/16), so the walk may stop before B's and A's shells.
    -> (queries, target points, per probe the source index and the target indices of A, B, C)."""
    eps, eta, delta = 2.0 ** -4, 2.0 ** -4, 2.0 ** -6
    pts, src, probes = [], [], []
    lanes = {(1, 1): (8, 8), (1, -1): (8, 24), (2, 1): (24, 8), (2, -1): (24, 24), (3, 1): (8, 16), (3, -1): (24, 16)}
    for r in (1, 2, 3):
        for a, s in AXES:
            b, d = (a + 1) % 3, (a + 2) % 3
            c = np.zeros(3)
            c[a], c[b], c[d] = 16.0, lanes[r, s][0], lanes[r, s][1]       # room for r + 2 cells along the axis, its own lane across
            q = c + 0.5
            q[a] = c[a] + (1 - eps if s > 0 else eps)
            dC = r + 1 + eps + eta
            C = q + unit(a, s) * dC
            dB = dC + delta
            da = r + 0.5 + eps
            tB = np.round(np.sqrt(dB * dB - da * da) * 1024) / 1024
            B = q + unit(a, s) * da + unit(b) * tB
            dA = dC + 2 * delta
            da = r - 0.5 + (1 - eps)
            tA = np.round(np.sqrt((dA * dA - da * da) / 2) * 1024) / 1024
            A = q - unit(a, s) * da - unit(b) * tA + unit(d) * tA
            if mirror:                                       # the nearest first: the walk may stop before B's and A's shells
                C = q + unit(a, s) * (eps + 2.0 ** -3)
            i0 = len(FRAME) + len(pts)
            pts += [A, B, C]
            probes.append(dict(src=len(src), A=i0, B=i0 + 1, C=i0 + 2, r=r, axis=a, sign=s))
            src.append(q)
    return np.array(src), pts, probes


def shell_exit(mirror=False):
    src, pts, probes = _shell_exit_points(mirror)
    # slack probes (r = 2 along +x and -x): X in shell 1 at 1 + 3 * 2^-12, P in shell 2 at 1 + 2^-11 -- between (r - 1) e
    # and (r - 1) e + slack (slack >= 1e-3), so a walk that ADDS the slack to its bound stops before P's shell
    slack = []
    for j, s in enumerate((1, -1)):
        c = np.array([28.0, 28.0, 12.0 + 8 * j])
        q = c + 0.5
        q[0] = c[0] + (1 - 2.0 ** -13 if s > 0 else 2.0 ** -13)
        P = q + unit(0, s) * (1 + 2.0 ** -11)
        X = q - unit(0, s) * 0.5 + unit(1) * np.round(np.sqrt((1 + 2.0 ** -11 + 2.0 ** -12) ** 2 - 0.25) * 2 ** 14) / 2 ** 14
        if mirror:
            X, P = q + unit(1) * 0.25, X
        i0 = len(FRAME) + len(pts)
        pts += [X, P]
        slack.append(dict(src=len(src), X=i0, P=i0 + 1, r=2, axis=0, sign=s))
        src = np.concatenate([src, [q]], 0)
    note = dict(what="shell_exit", probes=probes, slack=slack, mirror=mirror, edge=1.0)
    return src.astype(F), framed(pts), dict(max_iters=1), None, note


def gate_edge(gate):
    """Framed.  Per axis three pairs whose fp32 d2 is the largest fp32 <= gate^2 (as a double), one ulp below it and one
    above.  The query sits 1/16 inside the far face of its cell, so for gate 1.3 the partner lies two cells on (shell 2), for
    gate 0.5 in the next cell.  gate 0.5: gate^2 is a float and d2 == gate^2 exactly; gate 1.3: gate^2 is not representable.
    No pair can lie in a cell that the `reach` exit skips and yet pass the gate: a skipped shell r has (r - 1) e - slack >
    1.0001 gate, its points are more than (r - 1) e away, and slack >= 1e-3 e dwarfs the 2^-23 relative rounding of d2."""
    g2 = np.float64(gate) ** 2
    at = F(g2)
    if np.float64(at) > g2:
        at = np.nextafter(at, F(0))
    want = [np.nextafter(at, F(0)), at, np.nextafter(at, F(np.inf))]
    pts, src, probes = [], [], []
    lane = 0
    for a in range(3):
        for w, side in zip(want, (-1, 0, 1)):
            # d2 = fl(fl(dx^2) + fl(dy^2)): dx on the 2^-19 grid of the coordinates near 16 .. 32 brings fl(dx^2) to a few ulps
            # below w, a small dy on the 2^-22 grid of the lane coordinate supplies the rest
            o1, o2 = 2.5 + 4 * (lane % 7), 2.5 + 4 * (lane // 7)
            lane += 1
            b, c = (a + 1) % 3, (a + 2) % 3
            q = np.zeros(3, F); q[a] = F(16.9375); q[b] = F(o1); q[c] = F(o2)
            found = None
            dx0 = np.floor(np.sqrt(np.float64(w)) * 2.0 ** 19) / 2.0 ** 19
            for j in range(0, 8):
                dx = dx0 - j * 2.0 ** -19
                ta = F(np.float64(q[a]) + dx)
                ddx = F(q[a] - ta)
                a2 = F(ddx * ddx)
                rem = np.float64(w) - np.float64(a2)
                if rem < 0:
                    continue
                for dy in (np.round(np.sqrt(rem) * 2.0 ** 22) + np.arange(-2, 3)) / 2.0 ** 22:
                    tb = F(np.float64(q[b]) + dy)
                    ddy = F(q[b] - tb)
                    if F(F(a2 + F(ddy * ddy)) + F(0)) == w:
                        found = (ta, tb)
                        break
                if found:
                    break
            assert found is not None, (gate, a, side)
            t = q.copy()
            t[a], t[b] = found
            probes.append(dict(src=len(src), tgt=len(FRAME) + len(pts), side=side))
            pts.append(t); src.append(q)
    why = ("no pair can lie in a cell beyond `reach` and yet inside the gate: a shell r that the reach exit skips has (r - 1) e - slack > "
           "1.0001 gate, its points are more than (r - 1) e less one fp32 spacing of (q - origin) away, and slack >= 1e-3 e + 1e-5 |q - origin| "
           "dwarfs both that spacing and the 2^-23 relative rounding of d2, so their d2 exceeds gate^2")
    note = dict(what="gate_edge", probes=probes, gate=gate, at=float(at), edge=1.0, beyond_reach=why)
    return np.array(src, F), framed(pts), dict(max_iters=1, max_corr_dist=float(gate), min_corr=1), None, note


def outside(wide):
    """Framed target plus a 5^3 block of points in the middle; sources 1, 10 and 1 000 cells outside on each face, edge
    and corner direction.  wide: a gate of 1e5 admits them all; else a gate of 0.75 admits none of them (a handful of
    inside points keep the step defined).  The fitness pass has no gate either way."""
    blk = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.0 + 14.0
    tgt = framed(blk)
    dirs = [np.array(d, np.float64) for d in np.ndindex(3, 3, 3)]
    src = []
    for d in dirs:
        d = d - 1
        if not d.any():
            continue
        for k in (1, 10, 1000):
            base = np.where(d > 0, 32.0, np.where(d < 0, 0.0, 13.25))
            src.append(base + np.where(d > 0, k + 0.25, np.where(d < 0, -(k - 0.75), 0.0)))      # cells 32 + k and -k
    n_out = len(src)
    src += list(blk[::9] + 0.125)
    note = dict(what="outside", n_out=n_out, wide=wide, edge=1.0)
    return np.array(src, F), tgt, dict(max_iters=2, max_corr_dist=1.0e5 if wide else 0.75), None, note


def clamp(kind):
    rng = np.random.default_rng(103)
    if kind == "tiny":                                       # extent 1.2e-4 m: e = 3.8e-6 m; sources 10 .. 30 m away are 2.6e6 .. 8e6 cells off
        tgt = (rng.integers(0, 1024, (600, 3)) * 2.0 ** -23 + 1.0).astype(F)       # [1, 1 + 1.2e-4), on the fp32 grid of [1, 2)
        src = np.concatenate([tgt[:40] + F(10.0), tgt[40:80] - F(30.0), tgt[80:120] + np.array([0, 25.0, -15.0], F),
                              tgt[120:160] + np.array([2.0 ** -20, 0, 0], F)], 0)
        return src, tgt, dict(max_iters=2, max_corr_dist=100.0), None, dict(what="clamp", min_cell=1.0e6, n_far=120)
    src = rng.uniform(-2, 2, (300, 3)).astype(F)
    one = np.array([[0.5, -0.25, 1.0]], F)
    tgt = one if kind == "one_point" else np.repeat(one, 500, 0)
    return src, tgt, dict(max_iters=2, max_corr_dist=100.0), None, dict(what="one_point", n_tgt=len(tgt))


def flat_grids(kind):
    rng = np.random.default_rng(104)
    u, v = np.meshgrid(np.arange(40) * 0.25, np.arange(40) * 0.25, indexing="ij")
    u, v = u.ravel(), v.ravel()
    if kind == "plane":
        tgt = np.stack([u, v, np.full_like(u, 0.75)], 1)
    elif kind == "line":
        tgt = np.stack([np.arange(1500) * 0.03125, np.full(1500, -2.0), np.full(1500, 0.75)], 1)
    else:                                                    # tilted: z = x / 4 + y / 8, exact in fp32
        tgt = np.stack([u, v, u / 4 + v / 8], 1)
    pick = rng.permutation(len(tgt))[:400]
    off = rng.choice([-1.0, 1.0], 400)[:, None] * rng.choice([0.0625, 0.5, 3.0], 400)[:, None] * np.array([[0, 0, 1.0]])
    src = tgt[pick] + off + np.array([0.0625, 0.03125, 0])
    note = dict(what="flat", kind=kind)
    if kind == "line":
        note["rank"] = 1                                     # pairs with a collinear target: the covariance has rank 1, as in degenerate_step
    return src.astype(F), tgt.astype(F), dict(max_iters=3, max_corr_dist=5.0), None, note


def far_long():
    """4 km along x, 2 m wide, sources at the far end."""
    rng = np.random.default_rng(105)
    tgt = np.stack([np.arange(4001) * 1.0, (np.arange(4001) % 5) * 0.5, (np.arange(4001) % 3) * 0.25], 1)
    tgt[:, 0] += -0.3
    src = tgt[-900:] + rng.uniform(-0.2, 0.2, (900, 3))
    return src.astype(F), tgt.astype(F), dict(max_iters=2, max_corr_dist=2.0), None, dict(what="far_long")


def _first_in(G, c, y, z):
    """The smallest fp32 x whose computed x cell is >= c (the cell formula is monotone in x)."""
    def cell(x):
        return R.grid_cells(G, np.array([[x, y, z]], F))[0, 0]
    lo = F(np.float64(G["origin"][0]) + (c - 1) * np.float64(G["edge"]))
    hi = F(np.float64(G["origin"][0]) + (c + 1) * np.float64(G["edge"]))
    assert cell(lo) < c <= cell(hi)
    while np.nextafter(lo, F(np.inf)) < hi:                   # bisection over the floats between lo and hi
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if cell(mid) >= c:
            hi = mid
        else:
            lo = mid
    return hi


def slack_origin():
    """Where the slack of the exit bound is needed: a 2 km target that straddles the coordinate origin.  The grid's origin is
    ox = -1000, so (q - ox) is rounded at the fp32 spacing of 1000 (1.2e-4) while q and p, near x = +30 .. +300, sit on a grid
    fifty times finer.  The computed boundaries of neighbouring x cells then come up to one such spacing closer than e, more
    than the factor 0.99999 gives away (5e-6 e = 4.7e-5).  The builder takes, among the x cells 108 .. 139, the pair of
    boundaries (c + 1, c + 2) with the shortest gap; q is the last float of cell c, p the first float of cell c + 2 (shell 2,
    the true nearest, d(p) = the gap < e sqrt(0.99999)); X in q's own cell at a distance between d(p) and e sqrt(0.99999).
    An exit bound of (r - 1) e without the slack stops before shell 2 and answers X.
    Every cell of the trial grid (64 x 1 x 1) holds random points, so the grid does not depend on where p and X sit."""
    rng = np.random.default_rng(114)
    base = np.stack([rng.uniform(-1000, 1000, 2800), rng.uniform(0, 20, 2800), rng.uniform(0, 20, 2800)], 1)
    frame = np.array([[-1000.0, 0, 0], [1000.0, 20, 20]])
    y = z = 10.0

    def target(p, X, qx):
        b = base.copy()
        b[np.abs(b[:, 0] - qx) <= 25.0, 0] += 60.0            # nothing else near the probe; the count stays, so the grid does
        return np.concatenate([frame, b, [p, X]], 0).astype(F), len(b) + 2

    tgt0, _ = target([30.0, y, z], [20.0, y, z], 25.0)
    G = R.grid_of(tgt0)
    e = np.float64(G["edge"])
    best = None
    for c in range(108, 140):
        b1, b2 = _first_in(G, c + 1, y, z), _first_in(G, c + 2, y, z)
        q = np.nextafter(b1, F(-np.inf))
        gap = np.float64(b2) - np.float64(q)
        if best is None or gap < best[0]:
            best = (gap, c, q, b2)
    gap, c, qx, px = best
    lim = F(F(G["edge"] * G["edge"]) * F(0.99999))             # what the exit compares the best d2 with when slack = 0
    # X: 5 m back in x (the same cell), off in y, its fp32 d2 in the upper half of (d2(p), lim]
    want = (np.float64(F(gap) * F(gap)) + np.float64(lim)) / 2
    xx = F(np.float64(qx) - 5.0)
    ddx = F(qx - xx)
    Xy = F(y + np.sqrt(want - np.float64(ddx * ddx)))
    tgt, iP = target([px, y, z], [xx, Xy, z], np.float64(qx))
    G2 = R.grid_of(tgt)
    assert all(np.array_equal(np.asarray(G[k]), np.asarray(G2[k])) for k in G), "the grid moved with the probe"
    src = np.concatenate([[[qx, y, z]], base[:60] + 0.05], 0)
    keep = np.abs(base[:60, 0] - np.float64(qx)) > 25.0
    src = np.concatenate([src[:1], src[1:][keep]], 0)
    note = dict(what="slack_origin", src=0, P=iP, X=iP + 1, r=2, c=c, gap=float(gap), edge=None)
    return src.astype(F), tgt, dict(max_iters=1, max_corr_dist=30.0, min_corr=1), None, note


def big_coords():
    """Finite coordinates beyond LIO_MAX_COORD: such a TARGET point takes no part (one of them on one axis only, next to
    the sources: the restatement must not pair with it either); such a SOURCE point is finite, is searched, finds a d2 that
    is huge or overflows to inf, fails the gate and, in the fitness pass, counts only while d2 is finite."""
    rng = np.random.default_rng(106)
    body = rng.uniform(-8, 8, (1500, 3)).astype(F)
    bad_t = np.array([[2.0e15, 0.25, 0.25], [0.25, -3.0e20, 0.25], [0.25, 0.25, FLT_MAX], [1.0e15, 0.5, -0.5],
                      [np.nextafter(F(1.0e15), F(np.inf)), 0, 0]], F)
    tgt = np.concatenate([bad_t[:3], body, bad_t[3:]], 0)
    src = np.concatenate([body[::5] + F(0.03125), np.array([[0.25, 0.25, 0.25], [0.3, 0.2, 0.25]], F),
                          np.array([[3.0e15, 0, 0], [0, -1.0e19, 0], [1.0e19, 1.0e19, 1.0e19], [0, 0, FLT_MAX], [-FLT_MAX, FLT_MAX, 0],
                                    [1.0e25, 0, 0]], F)], 0)
    note = dict(what="big_coords", n_bad_src=6, bad_tgt=[0, 1, 2, len(tgt) - 1], in_range_tgt=len(tgt) - 2)
    return src, tgt, dict(max_iters=2, max_corr_dist=1.0), None, note


# --------------------------------------------------------------------------------------------- reduction, guess, criteria
def small_street(n_t=4000, n_s=1000, seed=107):
    """A street-like small pair: ground, two walls and a few poles; the source is a displaced, noisy part of it."""
    rng = np.random.default_rng(seed)
    k = n_t // 4
    ground = np.stack([rng.uniform(-20, 20, 2 * k), rng.uniform(-6, 6, 2 * k), rng.normal(0, 0.02, 2 * k)], 1)
    wall_l = np.stack([rng.uniform(-20, 20, k // 2), np.full(k // 2, 6.0), rng.uniform(0, 4, k // 2)], 1)
    wall_r = np.stack([rng.uniform(-20, 20, k // 2), np.full(k // 2, -6.0), rng.uniform(0, 3, k // 2)], 1)
    px = rng.choice(np.arange(-18, 19, 6.0), k)
    poles = np.stack([px + rng.normal(0, 0.05, k), np.sign(rng.normal(size=k)) * 4.0 + rng.normal(0, 0.05, k), rng.uniform(0, 5, k)], 1)
    tgt = np.concatenate([ground, wall_l, wall_r, poles], 0)
    near = tgt[np.abs(tgt[:, 0]) < 12]
    src = near[rng.permutation(len(near))[:n_s]] + rng.normal(0, 0.01, (n_s, 3))
    return src.astype(F), tgt.astype(F)


def rigid(axis, deg, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    M[:3, 3] = t
    return M


WG_SIZES = (1, 63, 64, 65, 255, 256, 257, 512, 513, 1025)
LOOKAHEADS = (0, 1, 3, 64)


def wg_bounds(n):
    """The first n points of one source; the points at indices 0, 63, 64, 255, 256, 511, 512, 1024 (the first and last
    lanes of waves and workgroups) are 1.5 .. 2.5 m off, inside the gate: the largest residuals sit where a lost lane,
    wave or workgroup would lose them."""
    src, tgt = small_street(seed=108, n_s=1025)
    M = rigid([0.1, -0.2, 1.0], 1.0, [0.15, -0.1, 0.05])
    src = R.transform_points(M.astype(F), src)
    rng = np.random.default_rng(109)
    for i in (0, 63, 64, 255, 256, 511, 512, 1024):
        src[i] += (rng.choice([-1.0, 1.0], 3) * rng.uniform(0.9, 1.4, 3)).astype(F)
    return src[:n].copy(), tgt, dict(max_iters=3, max_corr_dist=4.0, min_corr=1), None, dict(what="wg", marked=[i for i in (0, 63, 64, 255, 256, 511, 512, 1024) if i < n])


def guess_case(kind):
    src, tgt = small_street(seed=110)
    M = rigid([1.0, -2.0, 0.5], 20.0, [1.5, -0.75, 0.4])
    src0 = R.transform_points(np.linalg.inv(M).astype(F), src)       # the source as it is before the guess brings it back
    if kind == "skew":
        g = (rigid([0.3, 0.1, 1.0], 1.5, [0.2, 0.1, -0.05]) @ M).astype(F)
        return src0, tgt, dict(max_iters=6, max_corr_dist=3.0), g, dict(what="guess", kind=kind)
    g = M.astype(F)
    return src0, tgt, dict(max_iters=6, max_corr_dist=3.0), g, dict(what="guess", kind=kind)


def criteria(kind):
    src, tgt = small_street(seed=111, n_t=3000, n_s=800)
    M = rigid([0.2, 0.1, 1.0], 2.0, [0.3, -0.2, 0.1]).astype(F)
    moved = R.transform_points(M, src)
    base = dict(max_iters=6, max_corr_dist=3.0)
    if kind == "similar1":
        return moved, tgt, dict(base, max_similar=1, fitness_eps=2e-2, rel_mse_eps=0.0, transform_eps=0.0, rotation_threshold=1.0), None, dict(what="criteria", kind=kind, state=R.ABS_MSE, iters=5)
    if kind == "similar3":
        return moved, tgt, dict(base, max_similar=3, fitness_eps=7e-2, rel_mse_eps=0.0, transform_eps=0.0, rotation_threshold=1.0), None, dict(what="criteria", kind=kind, state=R.ABS_MSE, iters=5)
    if kind == "zero_mse":                                   # an exact copy: mse = 0 at once, then |0 - 0| / 0
        return tgt[::4].copy(), tgt, dict(base, max_similar=2, transform_eps=0.0, rotation_threshold=1.0), None, dict(what="criteria", kind=kind, state=R.ABS_MSE, iters=4)
    if kind == "mse_only":
        return moved, tgt, dict(base, transform_eps=0.0, rotation_threshold=1.0, fitness_eps=5e-3, rel_mse_eps=0.0), None, dict(what="criteria", kind=kind, state=R.ABS_MSE)
    if kind == "iterations":
        return moved, tgt, dict(base, fitness_eps=0.0, rel_mse_eps=0.0, transform_eps=0.0, rotation_threshold=1.0), None, dict(what="criteria", kind=kind, state=R.ITERATIONS)
    if kind == "reset":
        return similar_reset_case()
    if kind == "drop":
        return drop_pairs_case()
    raise KeyError(kind)


def _block(nx, ny, nz, x0, y0=0.0, z0=0.0, h=2.0):
    return np.stack(np.meshgrid(x0 + np.arange(nx) * h, y0 + np.arange(ny) * h, z0 + np.arange(nz) * h, indexing="ij"), -1).reshape(-1, 3)


def similar_reset_case():
    """similar, not similar, similar -- by the transformation criterion alone (|t|^2 <= 0.01, cos >= 0.9; the MSE tests off).
    Block A (216 points) is its target block moved by 0.02 along x: a tiny first step (similar).  That step carries block
    B (216 points, 0.51 beyond its own target block, gate 0.5) into the gate; now half of the pairs pull by 0.49: a step
    of 0.245 (not similar).  Then A hangs 0.245 on one side and B 0.245 on the other: the steps vanish (similar, similar).
    With max_similar = 1 the counter must fall back to 0 at the large step: TRANSFORM at iteration 3, not at 2."""
    tA, tB = _block(6, 6, 6, 0.0), _block(6, 6, 6, 40.0)
    tgt = np.concatenate([tA, tB], 0)
    src = np.concatenate([tA + [0.02, 0, 0], tB + [0.51, 0, 0]], 0)
    cfg = dict(max_iters=6, max_corr_dist=0.5, max_similar=1, transform_eps=0.01, rotation_threshold=0.9, rel_mse_eps=0.0, fitness_eps=0.0)
    return src.astype(F), tgt.astype(F), cfg, None, dict(what="criteria", kind="reset", state=R.TRANSFORM, iters=4)


def drop_pairs_case():
    """NO_CORRESPONDENCES at iteration 2 (the third): gate 0.5, min_corr 225.  Block A1 (216 points) sits 0.45 short of its
    target block, A2 (8 points) 0.85 short of its own, cluster B (27 points) 0.1 beyond its own.  Iteration 0 pairs A1
    and B (243); its step of about +0.389 brings A2 into the gate (0.461) and B to 0.489.  Iteration 1 pairs all 251; its
    step of about +0.015 carries B to 0.504, out of reach.  Iteration 2 finds 224 < 225."""
    t1, t2, tb = _block(6, 6, 6, 0.0), _block(2, 2, 2, 30.0, 4.0, 4.0), _block(3, 3, 3, 60.0, 3.0, 3.0)
    tgt = np.concatenate([t1, t2, tb], 0)
    src = np.concatenate([t1 - [0.45, 0, 0], t2 - [0.85, 0, 0], tb + [0.1, 0, 0]], 0)
    cfg = dict(max_iters=6, max_corr_dist=0.5, min_corr=225, transform_eps=0.0, fitness_eps=0.0, rel_mse_eps=0.0)
    return src.astype(F), tgt.astype(F), cfg, None, dict(what="criteria", kind="drop", drop_at=2, n_corr=[243, 251, 224])


def degenerate_step(rank):
    rng = np.random.default_rng(112)
    if rank == 1:                                            # target points on a line; the source is the same line shifted along itself
        t = np.arange(64)[:, None] * np.array([[0.5, 0.25, 0.125]])
        tgt = t
        src = t[8:40] + np.array([[0.5, 0.25, 0.125]]) * 0.25
    elif rank == 2:                                          # coplanar pairs that are mirror images IN the plane (y -> -y): only a half turn about x serves
        x = np.arange(40) * 1.0
        y = rng.integers(26, 103, 40) * 2.0 ** -8 * rng.choice([-1.0, 1.0], 40)
        tgt = np.stack([x, y, np.zeros(40)], 1)
        src = tgt * np.array([[1.0, -1.0, 1.0]])
    else:                                                    # every pair is the same pair
        tgt = np.array([[1.0, 2.0, 3.0]] * 4 + [[9.0, 9.0, 9.0]])
        src = np.array([[1.25, 2.0, 3.0]] * 40)
    return src.astype(F), tgt.astype(F), dict(max_iters=1, max_corr_dist=10.0, min_corr=3), None, dict(what="degenerate", rank=rank)


def step_reflection():
    """Full rank with det(U) det(V) < 0: a thin slab and its mirror image in z, every point paired with its own image."""
    rng = np.random.default_rng(113)
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), indexing="ij"), -1).reshape(-1, 2)
    z = rng.integers(2, 13, len(g)) * 2.0 ** -8 * rng.choice([-1.0, 1.0], len(g))
    src = np.concatenate([g * 1.5, z[:, None]], 1)
    tgt = src * np.array([[1.0, 1.0, -1.0]])
    return src.astype(F), tgt.astype(F), dict(max_iters=1), None, dict(what="reflection")


CASES = {
    "lattice_ties": lattice_ties,
    "cell_edges": cell_edges,
    "shell_exit": lambda: shell_exit(False),
    "shell_exit_mirror": lambda: shell_exit(True),
    "gate_edge_half": lambda: gate_edge(0.5),
    "gate_edge_odd": lambda: gate_edge(1.3),
    "outside_wide": lambda: outside(True),
    "outside_tight": lambda: outside(False),
    "clamp_tiny": lambda: clamp("tiny"),
    "clamp_one_point": lambda: clamp("one_point"),
    "clamp_repeated": lambda: clamp("repeated"),
    "flat_plane": lambda: flat_grids("plane"),
    "flat_line": lambda: flat_grids("line"),
    "flat_tilted": lambda: flat_grids("tilted"),
    "far_lattice": lambda: lattice_ties(FAR),
    "far_edges": lambda: cell_edges(FAR),
    "far_long": far_long,
    "slack_origin": slack_origin,
    "big_coords": big_coords,
    "guess_skew": lambda: guess_case("skew"),
    "guess_answer": lambda: guess_case("answer"),
    "crit_similar1": lambda: criteria("similar1"),
    "crit_similar3": lambda: criteria("similar3"),
    "crit_zero_mse": lambda: criteria("zero_mse"),
    "crit_mse_only": lambda: criteria("mse_only"),
    "crit_iterations": lambda: criteria("iterations"),
    "crit_reset": lambda: criteria("reset"),
    "crit_drop": lambda: criteria("drop"),
    "degenerate_rank0": lambda: degenerate_step(0),
    "degenerate_rank1": lambda: degenerate_step(1),
    "degenerate_rank2": lambda: degenerate_step(2),
    "step_reflection": step_reflection,
}
for _n in WG_SIZES:
    CASES[f"wg_{_n}"] = (lambda n: lambda: wg_bounds(n))(_n)

NAMES = list(CASES)


def build_case(name):
    """-> (src [n, 3] float32, tgt [m, 3] float32, cfg overrides, guess 4x4 float32 or None, note)."""
    src, tgt, cfg, guess, note = CASES[name]()
    cfg = dict(dict(min_source_points=0, min_target_points=0), **cfg)
    return np.ascontiguousarray(src, F), np.ascontiguousarray(tgt, F), cfg, guess, note
