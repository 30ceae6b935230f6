"""Scan Context (SCManager of the reference, Scancontext.cpp = SC) restated in numpy from the semantics DESIGN.md section 4c
states -- independent of the library, as tests/icp_restate.py is for the ICP.  Every fixed-order sum is a sequential
np.cumsum(...)[-1] (np.sum adds pairwise); fp32 steps stay in np.float32 arrays."""
import math

import numpy as np

NO_POINT = np.float32(-1000.0)
DEFAULTS = dict(num_rings=20, num_sectors=60, max_radius=80.0, lidar_height=2.0, num_exclude_recent=30, num_candidates=3,
                search_ratio=0.1, dist_thres=0.3, tree_period=10)
BAND_CELL = 1e-4      # a coordinate this close to an integer: the cell is not pinned (fp32 atan differs by a few ulp)
BAND_RANGE = 1e-3     # metres around max_radius


def seq_sum(a, axis=0):
    a = np.asarray(a, np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), np.float64)
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def c_round(x):
    f = math.floor(x)
    return int(f + 1) if x - f >= 0.5 else int(f)


def theta(x, y):
    """xy2theta SC:23-36 on float32 arrays: fp32 quotient and atan, the rest in fp64, rounded to float32."""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    k = 180.0 / np.pi
    out = np.zeros(x.shape, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q1 = (x >= 0) & (y >= 0); q2 = (x < 0) & (y >= 0); q3 = (x < 0) & (y < 0); q4 = (x >= 0) & (y < 0)
        out[q1] = k * np.arctan(y[q1] / x[q1]).astype(np.float64)
        out[q2] = 180.0 - k * np.arctan(y[q2] / (-x[q2])).astype(np.float64)
        out[q3] = 180.0 + k * np.arctan(y[q3] / x[q3]).astype(np.float64)
        out[q4] = 360.0 - k * np.arctan((-y[q4]) / x[q4]).astype(np.float64)
    return out.astype(np.float32)


def coords(xyz, num_rings=20, num_sectors=60, max_radius=80.0, lidar_height=2.0, **_):
    """Per point: used (finite, not on the z axis), inside (range <= max_radius), ring / sector (0-based), zf, the ring and
    sector coordinates u_r / u_s in fp64, the fp32 range."""
    p = np.asarray(xyz, np.float32)[:, :3]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    used = np.isfinite(p).all(1) & ~((x == 0) & (y == 0))
    xs, ys = np.where(used, x, np.float32(1)), np.where(used, y, np.float32(1))
    with np.errstate(over="ignore"):
        rng = np.sqrt(xs * xs + ys * ys)                      # float32 throughout
    ang = theta(xs, ys)
    inside = used & ~(rng.astype(np.float64) > max_radius)
    u_r = rng.astype(np.float64) / max_radius * num_rings
    u_s = ang.astype(np.float64) / 360.0 * num_sectors
    with np.errstate(invalid="ignore", over="ignore"):
        ring = np.clip(np.ceil(np.where(inside, u_r, 1.0)), 1, num_rings).astype(np.int64) - 1
        sector = np.clip(np.ceil(u_s), 1, num_sectors).astype(np.int64) - 1
        zf = (np.where(used, z, np.float32(0)).astype(np.float64) + lidar_height).astype(np.float32)
    return dict(used=used, inside=inside, ring=ring, sector=sector, zf=zf, u_r=u_r, u_s=u_s, range=rng)


def boundary_near(c, max_radius=80.0, **_):
    """The used points whose cell the fp32 atan of another libm could move (tests/test_gpu_sc.py explains the bands)."""
    near = lambda u: np.abs(u - np.round(u)) < BAND_CELL
    return c["used"] & (near(c["u_s"]) | near(c["u_r"]) | (np.abs(c["range"].astype(np.float64) - max_radius) < BAND_RANGE))


def _fold(ring, sector, zf, R, S):
    raw = np.full((R, S), NO_POINT, np.float32)
    np.maximum.at(raw, (ring, sector), zf)                    # cell < zf, then cell = zf: the maximum, from -1000
    return raw


def _fill(raw):
    out = raw.copy()
    out[out == NO_POINT] = 0
    return out


def make_desc(xyz, **cfg):
    """makeScancontext SC:151-195 -> float32 [rings, sectors]."""
    g = {**DEFAULTS, **cfg}
    c = coords(xyz, **g)
    m = c["inside"]
    return _fill(_fold(c["ring"][m], c["sector"][m], c["zf"][m], g["num_rings"], g["num_sectors"]))


def desc_bounds(xyz, **cfg):
    """(lo, hi, share): lo = the descriptor of the points that are not boundary-near; hi lets every boundary-near point count in
    each cell it could fall into (both sides of the nearby ring / sector boundary, the sector wrap, the last ring for a
    point within the band of max_radius, which may as well be dropped).  A cell whose only possible points lie below zero
    may read 0 (left empty) or that negative value: the pair is ordered so that lo <= hi covers both."""
    g = {**DEFAULTS, **cfg}
    R, S = g["num_rings"], g["num_sectors"]
    c = coords(xyz, **g)
    nb = boundary_near(c, **g)
    sure = c["inside"] & ~nb
    raw_lo = _fold(c["ring"][sure], c["sector"][sure], c["zf"][sure], R, S)
    raw_hi = raw_lo.copy()
    idx = np.nonzero(nb & (c["range"].astype(np.float64) <= g["max_radius"] + BAND_RANGE))[0]
    for i in idx:
        ur, us = c["u_r"][i], c["u_s"][i]
        kr, ks = int(np.round(ur)), int(np.round(us))
        rings = {kr, kr + 1} if abs(ur - kr) < BAND_CELL else {int(np.ceil(ur))}
        if abs(float(c["range"][i]) - g["max_radius"]) < BAND_RANGE:
            rings |= {R}
        secs = {ks, ks + 1} if abs(us - ks) < BAND_CELL else {int(np.ceil(us))}
        if abs(us - ks) < BAND_CELL and ks in (0, S):
            secs |= {1, S}
        for r in {min(max(r, 1), R) for r in rings}:
            for s in {min(max(s, 1), S) for s in secs}:
                raw_hi[r - 1, s - 1] = max(raw_hi[r - 1, s - 1], c["zf"][i])
    a, b = _fill(raw_lo), _fill(raw_hi)
    return np.minimum(a, b), np.maximum(a, b), float(nb.sum()) / max(int(c["used"].sum()), 1)


def ring_key(desc):
    """Row means SC:198-211 as the float vector of polarcontext_invkeys_mat_ (SC:241)."""
    d = np.asarray(desc, np.float64)
    return (seq_sum(d, axis=1) / d.shape[1]).astype(np.float32)


def sector_key(desc):
    d = np.asarray(desc, np.float64)
    return seq_sum(d, axis=0) / d.shape[0]


def dist_direct(a, b):
    """distDirectSC SC:69-90 on float64 [R, S] arrays."""
    n1, n2 = np.sqrt(seq_sum(a * a)), np.sqrt(seq_sum(b * b))
    ok = ~((n1 == 0) | (n2 == 0))
    if not ok.any():
        return float("nan")
    sim = seq_sum(a * b)[ok] / (n1[ok] * n2[ok])
    return float(1.0 - seq_sum(sim) / int(ok.sum()))


def fast_align(k1, k2):
    best, arg, norms = 10000000.0, 0, []
    for s in range(len(k1)):
        d = k1 - np.roll(k2, s)
        n = float(np.sqrt(seq_sum(d * d)))
        norms.append(n)
        if n < best:
            best, arg = n, s
    return arg, np.array(norms)


def distance(desc_a, desc_b, search_ratio=0.1, **_):
    """distanceBtnScanContext SC:116-148 -> (dist, align, info); info: the sector-key norms per shift, the searched shifts
    and their distances (what a test needs to see how close the runner-up is)."""
    a, b = np.asarray(desc_a, np.float64), np.asarray(desc_b, np.float64)
    S = a.shape[1]
    arg, norms = fast_align(sector_key(a), sector_key(b))
    radius = c_round(0.5 * search_ratio * S)
    shifts = sorted({arg} | {(arg + i) % S for i in range(1, radius + 1)} | {(arg - i + S) % S for i in range(1, radius + 1)})
    best, best_s, ds = 10000000.0, 0, []
    for s in shifts:
        d = dist_direct(a, np.roll(b, s, axis=1))
        ds.append(d)
        if d < best:
            best, best_s = d, s
    return best, best_s, dict(key_norms=norms, shifts=shifts, dists=np.array(ds), key_shift=arg)


def runner_up_gap(info):
    """How far the second-best value is from the best in both argmins of distance(): inf when there is no runner-up."""
    gaps = []
    for v in (info["key_norms"], info["dists"]):
        v = np.sort(v[~np.isnan(v)])
        gaps.append(v[1] - v[0] if len(v) > 1 else np.inf)
    return float(min(gaps))


def ring_d2(keys, q):
    """fp32 squared L2 in ascending dimension order of every key [n, R] against q [R]."""
    keys = np.asarray(keys, np.float32).reshape(-1, len(q))
    acc = np.zeros(len(keys), np.float32)
    for d in range(len(q)):
        e = np.float32(q[d]) - keys[:, d]
        acc = acc + e * e
    return acc


class Manager:
    """polarcontexts_ and detectLoopClosureID SC:253-344 with the counter and the stale prefix."""

    def __init__(self, **cfg):
        self.cfg = {**DEFAULTS, **cfg}
        self.descs, self.keys = [], []
        self.counter, self.prefix = 0, 0

    def add(self, desc):
        self.descs.append(np.asarray(desc, np.float32))
        self.keys.append(ring_key(desc))

    def detect(self, **over):
        g = {**self.cfg, **over}
        out = dict(loop_id=-1, yaw=np.float32(0), min_dist=10000000.0, align=0, nn_idx=0, n_searched=0, cand_idx=[], cand_d2=[],
                   cand_dist=[], cand_align=[], gaps=[])
        n = len(self.descs)
        if n < g["num_exclude_recent"] + 1:
            return out
        if self.counter % g["tree_period"] == 0:
            self.prefix = n - g["num_exclude_recent"]
        self.counter += 1
        d2 = ring_d2(np.stack(self.keys[:self.prefix]), self.keys[-1])
        order = np.lexsort((np.arange(self.prefix), d2))
        cand = order[:min(g["num_candidates"], self.prefix)]
        out.update(n_searched=self.prefix, cand_idx=[int(i) for i in cand], cand_d2=[d2[i] for i in cand], d2_sorted=d2[order])
        for i in cand:
            d, al, info = distance(self.descs[-1], self.descs[i], g["search_ratio"])
            out["cand_dist"].append(d); out["cand_align"].append(al); out["gaps"].append(runner_up_gap(info))
            if d < out["min_dist"]:
                out.update(min_dist=d, align=al, nn_idx=int(i))
        if out["min_dist"] < g["dist_thres"]:
            out["loop_id"] = out["nn_idx"]
        deg = np.float32(out["align"] * (360.0 / g["num_sectors"]))
        out["yaw"] = np.float32(np.float64(deg) * np.pi / 180.0)
        return out
