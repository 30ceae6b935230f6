"""Organised sweeps for markOccludedPoints + extractFeatures (FE:103-238) that no lidar produces: built directly from ring
lengths, a column rule, a range rule and a seed, without ray casting.  tests/test_feature_cases_cpu.py shows from the
oracle's outputs that every named case reaches the edge it is named for; tests/test_gpu_features_edges.py sends the same
cases through lio_extract_features and asks for the oracle's bits.

Ring windows follow cloudExtraction (synth.organize_scan): a ring of L points whose first point has index c gets
startRingIndex = c + 4 and endRingIndex = c + L - 6, so consecutive rings have start_B = end_A + 10 and the last point of
ring A (index end_A + 5 = start_B - 5) is the one cell that ring B's suppression walk can reach.  A ring of L points holds
end - start + 10 == L cells in its window [start-5, end+4].

All values are finite (NaN ranges make the reference's std::sort undefined).  Leaves stay >= 1e-4 (below that PCL's own
int64 product overflows)."""
import numpy as np

COL_RULES = ("ramp", "mod8", "gaps", "extreme")
RANGE_RULES = ("wall", "comb", "quantised", "steps", "uniform")
MAX_RING = 4096                      # points of the longest ring lio_extract_features accepts (FEAT_MAX_RING cells of LDS)
Q20 = 2.0 ** -20                     # ulp of a float32 in [8, 16): every `steps` range is a multiple of it, so differences are exact

# `steps` deltas, in units of Q20, a few float32 ulps either side of the two gates of markOccludedPoints: 0.3 = 314572.8 Q20
# (FE:114-130, depth difference) and 0.02 * 10 = 0.2 = 209715.2 Q20 (FE:133-137, both neighbours of a point at range 10).
# The nearest multiples are 0.2 and 0.8 Q20 away (6 and 25 ulps of 0.3, 13 and 54 of 0.2): no decimal literal's rounding decides.
STEP_BELOW, STEP_ABOVE = (314570, 314572), (314573, 314575)
BEAM_BELOW, BEAM_ABOVE = (209713, 209715), (209716, 209718)


def ring_indices(lengths):
    """startRingIndex / endRingIndex of cloudExtraction for rings of the given lengths."""
    start = np.zeros(len(lengths), np.int32)
    end = np.zeros(len(lengths), np.int32)
    count = 0
    for i, L in enumerate(lengths):
        start[i] = count - 1 + 5
        count += int(L)
        end[i] = count - 1 - 5
    return start, end


def sectors(start, end):
    """The six (sp, ep) of one ring, FE:156-157 (start >= 0, so floor and C division agree)."""
    s, e = int(start), int(end)
    return [((s * (6 - j) + e * j) // 6, (s * (5 - j) + e * (j + 1)) // 6 - 1) for j in range(6)]


def valid_sectors(start, end):
    if end < start:
        return []
    return [(sp, ep) for sp, ep in sectors(start, end) if sp < ep]           # FE:159


def key_count(start, end):
    """Elements std::sort FE:162 sees in one ring: the sum of ep - sp over its sectors."""
    return sum(ep - sp for sp, ep in valid_sectors(start, end))


def length_for_key_count(target, first=0):
    """The ring length whose sort sees exactly `target` elements, for a ring whose first point has index `first`."""
    for L in range(10, MAX_RING + 1):
        if key_count(first + 4, first + L - 6) == target:
            return L
    raise ValueError(target)


def _columns(L, rule, rng):
    i = np.arange(L)
    if rule == "ramp":
        return i.astype(np.int32)
    if rule == "mod8":
        return (i % 8).astype(np.int32)
    if rule == "gaps":                                  # steps of exactly 10 and 11: the two sides of `> 10`, FE:183/215
        col = np.cumsum(rng.choice([1, 10, 11], size=L, p=[0.5, 0.25, 0.25])) - 1
        assert L == 0 or col[-1] <= 32767
        return col.astype(np.int32)
    if rule == "extreme":                               # both ends of int16, in runs of seven
        return np.where((i // 7) % 2 == 0, -32768 + (i % 3), 32767 - (i % 3)).astype(np.int32)
    raise ValueError(rule)


def _steps(L, rng):
    """Range 10 with an event every 16 points: a lasting step up / back down by a delta next to 0.3, or a point whose two
    neighbours stand off by deltas next to 0.2.  Returns the ranges and the events as (index, kind, side):
    kind 'up' / 'down' = the step lies between index and index + 1; 'beam' = the point at index; side +1 = above the gate."""
    q = np.full(L, 10 * 2 ** 20, np.int64)
    events = []
    level = 0
    for n_ev, i in enumerate(range(24, L - 24, 16)):
        side = 1 if rng.integers(2) else -1
        if n_ev % 2 == 0:
            d = int(rng.choice(STEP_ABOVE if side > 0 else STEP_BELOW))
            if level == 0:
                q[i + 1:] += d; level = d; events.append((i, "up", side))
            else:
                q[i + 1:] -= level; events.append((i, "down", 1 if level >= STEP_ABOVE[0] else -1)); level = 0
        elif level == 0:
            above, below = BEAM_ABOVE, BEAM_BELOW
            a = int(rng.choice(above)) if side > 0 else int(rng.choice(below))
            b = int(rng.choice(above))
            if rng.integers(2):
                a, b = b, a
            q[i - 1] += a; q[i + 1] += b
            events.append((i, "beam", side))
    return (q * Q20).astype(np.float32), events


def _ranges(L, rule, rng):
    i = np.arange(L)
    if rule == "wall":                                  # flat, millimetre noise: every point is a surface candidate
        return (10.0 + 0.002 * rng.standard_normal(L)).astype(np.float32), []
    if rule == "comb":                                  # alternating near / far: curvature (6 * 0.25)^2 = 2.25 > edgeThreshold
        return (20.0 + 0.25 * (i % 2) + 0.001 * rng.standard_normal(L)).astype(np.float32), []   # everywhere, below both gates
    if rule == "quantised":                             # multiples of 0.25: curvatures are exact and tie
        r = 10.0 + 0.6 * np.sin(i * 0.037 + rng.uniform(0, 6.28)) + 0.08 * rng.standard_normal(L)
        return (np.round(r * 4) / 4).astype(np.float32), []
    if rule == "steps":
        return _steps(L, rng)
    if rule == "uniform":
        return rng.uniform(1.0, 50.0, L).astype(np.float32), []
    raise ValueError(rule)


def spikes(L, positions, rng):
    """A wall at 20 m whose points at `positions` (ring-relative) stand 0.15 m behind it: curvature 2.25 there, 0.0225 next
    to it, and both gates of markOccludedPoints stay shut."""
    r = 20.0 + 0.0005 * rng.standard_normal(L)
    r[np.asarray(positions, int)] += 0.15
    return r.astype(np.float32)


def _per_ring(rule, n):
    return [rule] * n if isinstance(rule, str) or not isinstance(rule, (list, tuple)) else list(rule)


def make_sweep(lengths, col_rule="ramp", range_rule="wall", seed=0, geom=None):
    """-> dict(cloud [n,4] xyzi, start_ring, end_ring, col, range, lengths, events).  col_rule / range_rule: a name, or
    one entry per ring (a name, or an array of that ring's values).  geom: {ring: (shape, scale, offset)} with shape
    'cone' (the default: one elevation per ring, azimuth by position) or 'sphere' (random directions); xyz = scale *
    range * direction + offset, so the per-ring voxel filter sees a box that follows the ranges."""
    lengths = [int(L) for L in lengths]
    rng = np.random.default_rng(seed)
    start, end = ring_indices(lengths)
    cols, rngs, xyz, events = [], [], [], []
    first = 0
    for i, (L, cr, rr) in enumerate(zip(lengths, _per_ring(col_rule, len(lengths)), _per_ring(range_rule, len(lengths)))):
        col = _columns(L, cr, rng) if isinstance(cr, str) else np.asarray(cr, np.int32)
        r, ev = _ranges(L, rr, rng) if isinstance(rr, str) else (np.asarray(rr, np.float32), [])
        assert len(col) == L and len(r) == L
        shape, scale, offset = (geom or {}).get(i, ("cone", 1.0, 0.0))
        if shape == "sphere":
            d = rng.standard_normal((L, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
        else:
            el = np.radians(-15.0 + 2.0 * (i % 16))
            az = 2 * np.pi * np.arange(L) / max(L, 1)
            d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.full(L, np.sin(el))], 1)
        xyz.append(scale * r[:, None].astype(np.float64) * d + offset)
        cols.append(col); rngs.append(r)
        events += [(first + k, kind, side) for k, kind, side in ev]
        first += L
    n = first
    cloud = np.zeros((n, 4), np.float32)
    if n:
        cloud[:, :3] = np.concatenate(xyz)
        cloud[:, 3] = rng.uniform(0, 255, n)
    assert np.isfinite(cloud).all()
    return {"cloud": cloud, "start_ring": start, "end_ring": end,
            "col": np.concatenate(cols).astype(np.int32) if n else np.zeros(0, np.int32),
            "range": np.concatenate(rngs).astype(np.float32) if n else np.zeros(0, np.float32),
            "lengths": lengths, "events": events}


# ---------------------------------------------------------------- what the oracle's outputs say about a sweep
def oracle_cfg(cfg):
    return {"edge_threshold": cfg.get("edgeThreshold", 1.0), "surf_threshold": cfg.get("surfThreshold", 0.1),
            "surf_leaf": cfg.get("surfLeafSize", 0.2)}


def run_oracle(oracle, sw, start=None, end=None, **cfg):
    return oracle.extract_features(sw["cloud"], sw["start_ring"] if start is None else start,
                                   sw["end_ring"] if end is None else end, sw["col"], sw["range"], **oracle_cfg(cfg))


def shared_cells(oracle, sw, **cfg):
    """Boundaries A|B where the last point of ring A (index end_A + 5) is picked only because ring B picked: it is 1, and 0
    once ring B is emptied.  -> list of (ring A, cell index)."""
    ref = run_oracle(oracle, sw, **cfg)
    start, end = sw["start_ring"], sw["end_ring"]
    live = [i for i in range(len(start)) if end[i] >= start[i]]
    found = []
    for a, b in zip(live[:-1], live[1:]):
        cell = int(end[a]) + 5
        if cell != int(start[b]) - 5 or ref["picked"][cell] != 1:
            continue
        s2, e2 = start.copy(), end.copy()
        s2[b], e2[b] = 4, -6
        if run_oracle(oracle, sw, s2, e2, **cfg)["picked"][cell] == 0:
            found.append((a, cell))
    return found


def sector_report(ref, sw, edge_thr):
    """Per valid sector: (ring, sp, ep, corners labelled, points above edge_thr, of those left unpicked and unlabelled)."""
    rows = []
    for i, (s, e) in enumerate(zip(sw["start_ring"], sw["end_ring"])):
        for sp, ep in valid_sectors(s, e):
            sl = slice(sp, ep + 1)
            above = ref["curvature"][sl] > np.float32(edge_thr)
            left = above & (ref["picked"][sl] == 0) & (ref["label"][sl] == 0)
            rows.append((i, sp, ep, int((ref["label"][sl] == 1).sum()), int(above.sum()), int(left.sum())))
    return rows


def visits_of_picks(ref, sp, ep, lab):
    """Visit numbers (0-based) at which one sector's pass labelled its picks: lab 1 = the corner pass FE:165 (element ep,
    then the sorted range descending), lab -1 = the surface pass FE:197 (the sorted range ascending, then element ep)."""
    order = [sp + int(k) for k in np.argsort(ref["curvature"][sp:ep], kind="stable")] + [ep]
    if lab == 1:
        order.reverse()
    return [v for v, ind in enumerate(order) if ref["label"][ind] == lab]


def candidate_lists(ref, sw):
    """Per ring, the positions FE:224-229 hands to the voxel filter: sp..ep of every valid sector with label <= 0."""
    out = []
    for s, e in zip(sw["start_ring"], sw["end_ring"]):
        out.append([k for sp, ep in valid_sectors(s, e) for k in range(sp, ep + 1) if ref["label"][k] <= 0])
    return out


# ---------------------------------------------------------------- the named cases
def _case(cid, sw, **cfg):
    return {"id": cid, "sweep": sw, "cfg": cfg}


SHARED_RINGS = [4000, 12, 30, 4086, 13, 700]
SHARED_SEEDS = (32, 38, 39)                              # of seeds 0..39 the three with at least two such boundaries
# The issue's ring list only lets a short ring A precede a ring B that picks (a 12- or 13-point ring has no sector).  This
# one puts long rings in front of 30-point rings, whose first sector is [start, start + 2]: the long ring's write-back comes last.
SHARED_LONG_RINGS = [4000, 30, 4086, 30, 3000, 30, 30]
SHARED_LONG_SEEDS = (9, 11, 21)                          # all six boundaries each


def shared_cell_cases():
    return ([_case(f"shared_cell-{s}", make_sweep(SHARED_RINGS, "mod8", "wall", s)) for s in SHARED_SEEDS]
            + [_case(f"shared_cell_long-{s}", make_sweep(SHARED_LONG_RINGS, "mod8", "wall", s)) for s in SHARED_LONG_SEEDS])


CAP_SPIKES = (19, 20, 21, 20, 1, 0)                      # spikes per sector of the second ring of corner_cap


def corner_cap_cases():
    rng = np.random.default_rng(5)
    L = 1810                                             # end - start = 1800: sectors of 300 positions
    secs = sectors(1800 + 4, 1800 + L - 6)               # the spike ring comes second, after an 1800-point comb ring
    pos = [sp + 10 + 12 * k - 1800 for (sp, ep), m in zip(secs, CAP_SPIKES) for k in range(m)]
    sw = make_sweep([1800, L], "ramp", ["comb", spikes(L, pos, rng)], seed=5)
    return [_case("corner_cap", sw)]


CHUNK_SIZES = (63, 64, 65, 127, 128, 129)


def chunk_edges_cases():
    lengths = [6 * (m + 1) + 10 for m in CHUNK_SIZES]    # end - start = 6 (m + 1): six sectors with ep - sp = m
    return [_case("chunk_edges-wall", make_sweep(lengths, "ramp", "wall", 11)),
            _case("chunk_edges-comb", make_sweep(lengths, "mod8", "comb", 12), edgeThreshold=0.1),
            _case("chunk_edges-quantised", make_sweep(lengths, "gaps", "quantised", 13), edgeThreshold=0.1)]


KEY_COUNTS = (1, 2, 3, 2047, 2048, 2049)
LIST_LENGTHS = (255, 256, 257)


def sort_sizes_cases():
    lengths, first = [], 0
    for k in KEY_COUNTS:
        lengths.append(length_for_key_count(k, first))
        first += lengths[-1]
    lists = [n + 10 for n in LIST_LENGTHS]               # a wall ring has no corner: its list is every position of its
    return [_case("sort_sizes-keys", make_sweep(lengths, "ramp", "quantised", 21)),                    # sectors, end - start
            _case("sort_sizes-keys-comb", make_sweep(lengths, "mod8", "comb", 22)),
            _case("sort_sizes-lists", make_sweep(lists, "ramp", "wall", 23))]


def longest_ring_cases():
    M = MAX_RING
    return [_case("longest_ring-alone", make_sweep([M], "mod8", "wall", 31)),
            _case("longest_ring-first", make_sweep([M, 12, 700], "ramp", "comb", 32)),
            _case("longest_ring-last", make_sweep([700, 12, M], "mod8", "quantised", 33)),
            _case("longest_ring-between", make_sweep([12, M, 12], "extreme", "steps", 34))]


def too_long_sweep():
    return make_sweep([12, MAX_RING + 1, 12], "mod8", "wall", 35)


def ties_cases():
    sw = make_sweep([1800, 700], "ramp", "quantised", 41)
    thr = tie_value(sw)
    return [_case("ties", sw, edgeThreshold=thr, surfThreshold=thr)]


def tie_value(sw):
    """The most frequent non-zero curvature of a quantised sweep (exact in float32: every term is a multiple of 0.25)."""
    r = sw["range"].astype(np.float32)
    n = len(r)
    d = np.zeros(n, np.float32)
    for k in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5):
        d[5:n - 5] += r[5 + k:n - 5 + k]
    d[5:n - 5] -= r[5:n - 5] * np.float32(10)            # every partial sum is exact, so the order does not matter
    c = d * d
    vals, counts = np.unique(c[c > 0], return_counts=True)
    return float(vals[np.argmax(counts)])


ONE_VOXEL_GEOM = {1: ("cone", 1e-3, 0.1), 3: ("sphere", 100.0, 0.0)}


def one_voxel_cases():
    # leaf 0.2: ring 1 lies within 0.1 +- 0.011 (one voxel), ring 3 spans +-1000 m (10^4 voxels a side: PCL's index overflows
    # and the ring passes through), rings 0, 2, 4 are filtered normally
    sw = make_sweep([700, 400, 700, 400, 300], "ramp", "wall", 51, geom=ONE_VOXEL_GEOM)
    return [_case("one_voxel-0.2", sw, surfLeafSize=0.2),
            _case("one_voxel-1e-4", sw, surfLeafSize=1e-4),          # every ring but ring 1 passes through
            _case("one_voxel-50", sw, surfLeafSize=50.0)]            # the normal rings collapse to a few voxels as well


def n_scan_cases():
    rng = np.random.default_rng(61)
    sparse = np.zeros(1024, int)
    sparse[rng.choice(1024, 20, replace=False)] = rng.choice([12, 70, 400, 1800], 20)
    sparse[[0, 1023]] = 70, 400                          # the first and the last ring are among the live ones
    return [_case("n_scan-1", make_sweep([1800], "ramp", "quantised", 62)),
            _case("n_scan-6", make_sweep([4000] * 6, "ramp", ["wall", "comb", "quantised", "steps", "uniform", "wall"], 63)),
            _case("n_scan-128", make_sweep(rng.choice([0, 11, 70, 130], 128), "mod8", "quantised", 64)),
            _case("n_scan-1024", make_sweep(sparse, "gaps", "quantised", 65))]


def steps_cases():
    return [_case("steps", make_sweep([1800, 700], "ramp", "steps", 71))]


def strides_sweep():
    return make_sweep([400, 0, 1800, 12, 70], "ramp", ["wall", "wall", "comb", "wall", "quantised"], 81)


CASES = {"shared_cell": shared_cell_cases, "corner_cap": corner_cap_cases, "chunk_edges": chunk_edges_cases,
         "sort_sizes": sort_sizes_cases, "longest_ring": longest_ring_cases, "ties": ties_cases,
         "one_voxel": one_voxel_cases, "n_scan": n_scan_cases, "steps": steps_cases}
_BUILT, _REFS = {}, {}


def cases(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def reference(oracle, case):
    """The oracle's outputs for a named case, computed once per process and shared (treat as read-only)."""
    if case["id"] not in _REFS:
        _REFS[case["id"]] = run_oracle(oracle, case["sweep"], **case["cfg"])
    return _REFS[case["id"]]


# ---------------------------------------------------------------- fuzz
FUZZ_LENGTHS = (0, 3, 11, 12, 13, 70, 400, 1800, 4000)


def fuzz_trial(t):
    """Trial t of the seeded fuzz -> (sweep, cfg, the parameters as a string for the assertion message)."""
    rng = np.random.default_rng(1000 + t)
    lengths = []
    for L in rng.choice(FUZZ_LENGTHS, int(rng.integers(1, 41))):
        if sum(lengths) + int(L) <= 30000:
            lengths.append(int(L))
    col = str(rng.choice(COL_RULES))
    rr = str(rng.choice(RANGE_RULES))
    cfg = {"edgeThreshold": float(rng.choice([0.05, 0.1, 1.0])), "surfThreshold": float(rng.choice([0.05, 0.1, 1.0])),
           "surfLeafSize": float(rng.choice([0.05, 0.2, 0.4, 2.0]))}
    what = f"trial {t}: rings {lengths}, columns {col}, ranges {rr}, seed {2000 + t}, {cfg}"
    return make_sweep(lengths, col, rr, 2000 + t), cfg, what


# ---------------------------------------------------------------- device against oracle, bit for bit
def diff_report(out, ref, sw):
    """'' when the five outputs agree bit for bit, else what differs (for `picked`: the indices, and whether each is the
    last point of a ring, i.e. an end + 5 cell)."""
    msgs = []
    for k in ("curvature", "picked", "label"):
        a, b = out[k], ref[k]
        same = a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        if not same:
            idx = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0] if a.shape == b.shape else np.zeros(0, int)
            msg = f"{k}: {len(idx)} of {len(b)} differ, first at {idx[:12].tolist()}"
            if k == "picked":
                cells = {int(e) + 5 for s, e in zip(sw["start_ring"], sw["end_ring"]) if e >= s}
                msg += "; " + ", ".join(f"{int(i)} (device {int(a[i])}, oracle {int(b[i])}, "
                                        f"{'an end+5 cell' if int(i) in cells else 'NOT an end+5 cell'})" for i in idx[:12])
            msgs.append(msg)
    for k in ("corner", "surface"):
        a, b = out[k], ref[k]
        if a.shape != b.shape:
            msgs.append(f"{k}: {a.shape[0]} points, oracle {b.shape[0]}")
        elif not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            rows = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0]
            msgs.append(f"{k}: {len(rows)} of {len(b)} points differ, first at {rows[:12].tolist()}")
    return "\n".join(msgs)


def compare(pkg, ref, sw, what="", **cfg):
    """lio_extract_features on the sweep against the oracle's `ref`: curvature, picked, label, corner and surface bit-identical."""
    out = pkg.extract_features(sw["cloud"], sw["start_ring"], sw["end_ring"], sw["col"], sw["range"], **cfg)
    rep = diff_report(out, ref, sw)
    assert not rep, f"{what}\n{rep}"
    return out
