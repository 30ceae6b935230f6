"""Sweeps for projectPointCloud + deskewPoint (IP:502-615) and the range-image build that no lidar produces: every case is
built directly from a seed -- point fields, a hand-written IMU rotation table and a config -- without ray casting and
without imuDeskewInfo.  tests/test_deskew_cases_cpu.py shows from the inputs and the oracle's outputs that every named
case reaches the edge it is named for; tests/test_gpu_deskew_edges.py sends the same cases through lio_deskew,
lio_deskew_pc2 and lio_range_image and asks for the oracle's bits.

A case is a dict: id, kind ('deskew' | 'ri' | 'pc2'), x, y, z, intensity, ring (uint16), time (float32), imu (the tuple
imuPointerCur, imuTime, imuRotX, imuRotY, imuRotZ), t0 (timeScanCur), cfg (lio_deskew_config fields), for 'ri' cases H
and minRange, for 'pc2' cases blob + layout (the fields above are then what cachePointCloud IP:226-285 makes of the
blob), nan (only the nan_* cases may hold or produce NaN) and expect (what the CPU file proves).

Point times: a table entry is written as t0 + (double)tau_k for a float32 tau_k, so a point whose time field is tau_k
lands on the entry exactly -- the sum the kernel forms, IP:550, is the same fp64 addition."""
import math

import numpy as np

F32 = np.float32
OPEN = dict(N_SCAN=16, downsampleRate=1, point_filter_num=1, lidarMinFront=0.0, lidarMinBack=0.0, lidarMinLeft=0.0,
            lidarMinRight=0.0, lidarMaxRange=1000.0, lidarMaxIntensity=1.0e9, deskew_flag=1)      # no gate shuts
BOX = dict(OPEN, lidarMinFront=1.0, lidarMinBack=5.0, lidarMinLeft=2.0, lidarMinRight=2.0, lidarMaxIntensity=100.0)
T0_BIG = 1.7e9 + 0.123                                    # fp64 ulp 2^-22 s = 2.4e-7 s: t0 + (double)time loses bits


def cfg(base=OPEN, **kw):
    return dict(base, **kw)


def step(v, j):
    """The float32 j ulps above (j > 0) or below v."""
    v = F32(v)
    for _ in range(abs(j)):
        v = np.nextafter(v, F32(np.inf if j > 0 else -np.inf))
    return v


def range_f32(x, y, z):
    """pointDistance, common_lib.cpp:27-31, in float32 operations."""
    x, y, z = F32(x), F32(y), F32(z)
    return np.sqrt(x * x + y * y + z * z)


# ---------------------------------------------------------------- the column rule of the range image, literally
def c_round(v):
    """C round(): halves away from zero."""
    return math.copysign(math.floor(abs(v) + 0.5), v)


def column_of(x, y, H):
    """-> (horizonAngle as float32, the column before the `col >= H` wrap, the column or -1)."""
    at = F32(math.atan2(float(F32(x)), float(F32(y))))
    at180 = at * F32(180)
    h = F32(float(at180) / math.pi)
    res = F32(360.0 / float(F32(H)))
    if h != h:                                              # NaN x or y: dropped before the (int), which is undefined for it
        return h, None, -1
    raw = int(-c_round((float(h) - 90.0) / float(res)) + float(H // 2))
    col = raw - H if raw >= H else raw
    return h, raw, (col if 0 <= col < H else -1)


# ---------------------------------------------------------------- IMU tables and point times
def make_table(t0, taus, seed, amp=0.3):
    """imuTime[k] = t0 + (double)tau_k, rotations a noisy ramp of up to `amp` rad in yaw.  -> (imu tuple, taus)."""
    taus = np.asarray(taus, F32)
    k = len(taus)
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, k)
    T = t0 + taus.astype(np.float64)
    RX = 0.2 * amp * s + 0.003 * rng.standard_normal(k)
    RY = -0.1 * amp * s + 0.003 * rng.standard_normal(k)
    RZ = amp * s + 0.003 * rng.standard_normal(k)
    return (k - 1, T, RX, RY, RZ), taus


def taus_70():
    return (0.01 + 0.002 * np.arange(70)).astype(F32)


KINDS = ("before", "on_entry", "on_last", "inside", "after")


def times_of(kinds, taus, rng):
    """One float32 time per entry of `kinds`, placed relative to the table's taus."""
    lo, hi = float(taus[0]), float(taus[-1])
    out = np.zeros(len(kinds), F32)
    for i, kind in enumerate(kinds):
        if kind == "before":
            out[i] = rng.uniform(lo - 0.02, lo - 1e-3)
        elif kind == "after":
            out[i] = rng.uniform(hi + 1e-3, hi + 0.02)
        elif kind == "on_last":
            out[i] = taus[-1]
        elif kind == "on_entry":
            out[i] = taus[int(rng.integers(0, len(taus) - 1))]
        else:
            k = int(rng.integers(0, len(taus) - 1))
            a, b = float(taus[k]), float(taus[k + 1])
            out[i] = a + (b - a) * rng.uniform(0.2, 0.8)
    return out


def mixed_times(n, taus, rng):
    return times_of(rng.choice(KINDS, n), taus, rng)


def branch_counts(case, idx=None):
    """How many of the points `idx` (default: all) take each way through findRotation IP:502-527 -- from the inputs alone.
    before: front == 0 (entry 0 taken as is); after: past the last entry (the last taken as is); on_last: equal to the
    last entry (interpolated with ratioFront 1); on_entry: equal to an earlier entry (ratioFront 0); inside; nan."""
    cur, T = case["imu"][0], np.asarray(case["imu"][1])[:case["imu"][0] + 1]
    t = np.asarray(case["time"], F32)
    if idx is not None:
        t = t[idx]
    pt = case["t0"] + t.astype(np.float64)
    nan = np.isnan(pt)
    front = np.searchsorted(T[:cur], pt, side="right")      # the first entry of the first `cur` that is > pt
    before = (front == 0) & ~nan
    after = (front == cur) & (pt > T[cur])
    on_last = pt == T[cur]
    on_entry = np.isin(pt, T[:cur]) & ~before
    inside = ~(nan | before | after | on_last | on_entry)
    return {"before": int(before.sum()), "after": int(after.sum()), "on_last": int(on_last.sum()),
            "on_entry": int(on_entry.sum()), "inside": int(inside.sum()), "nan": int(nan.sum())}


# ---------------------------------------------------------------- point fields
def cloud(n, rng, n_scan=16):
    """n points that pass every gate of BOX: |x| >= 2.5, range < 100, intensity < 90, ring < n_scan."""
    x = rng.uniform(2.5, 60.0, n) * rng.choice([-1.0, 1.0], n)
    y = rng.uniform(-60.0, 60.0, n)
    z = rng.uniform(-3.0, 8.0, n)
    return {"x": x.astype(F32), "y": y.astype(F32), "z": z.astype(F32),
            "intensity": rng.uniform(0.0, 90.0, n).astype(F32), "ring": rng.integers(0, n_scan, n).astype(np.uint16)}


def drop(f, idx, rng, n_scan=16):
    """Make the points `idx` fail one gate of BOX each: the vehicle box, the ring, or the intensity."""
    idx = np.asarray(idx, int)
    why = rng.integers(0, 3, len(idx))
    b = idx[why == 0]
    f["x"][b] = rng.uniform(-1.9, 1.9, len(b)); f["y"][b] = rng.uniform(-4.9, 0.9, len(b))
    r = idx[why == 1]
    f["ring"][r] = rng.integers(n_scan, n_scan + 30, len(r))
    i = idx[why == 2]
    f["intensity"][i] = rng.uniform(101.0, 200.0, len(i))


def _case(cid, kind, f, time, imu, t0, c, nan=False, **extra):
    n = len(f["x"])
    case = {"id": cid, "kind": kind, "nan": nan, "t0": float(t0), "imu": imu, "cfg": c, "expect": {},
            "x": np.ascontiguousarray(f["x"], F32), "y": np.ascontiguousarray(f["y"], F32),
            "z": np.ascontiguousarray(f["z"], F32), "intensity": np.ascontiguousarray(f["intensity"], F32),
            "ring": np.ascontiguousarray(f["ring"], np.uint16), "time": np.ascontiguousarray(time, F32)}
    assert all(len(case[k]) == n for k in ("y", "z", "intensity", "ring", "time")) and n <= 70000
    case.update(extra)
    return case


# ---------------------------------------------------------------- time_*: the ways through findRotation
def time_cases():
    out = []
    for cid, kinds, seed in (("time_before", ["before"], 101), ("time_on_entries", None, 102), ("time_after", ["after"], 103),
                             ("time_mixed", list(KINDS), 104)):
        rng = np.random.default_rng(seed)
        n = 5000 if cid == "time_mixed" else 400
        imu, taus = make_table(100.0, taus_70(), seed)
        if kinds is None:                                   # three entries: the first, one in the middle, the last
            t = taus[np.array([0, 34, 69])[np.arange(n) % 3]]
        else:
            t = times_of(rng.choice(kinds, n), taus, rng)
        out.append(_case(cid, "deskew", cloud(n, rng), t, imu, 100.0, cfg()))
    rng = np.random.default_rng(105)                        # the smallest table that deskews: imuPointerCur == 1
    imu, taus = make_table(100.0, [0.01, 0.09], 105)
    out.append(_case("time_table2", "deskew", cloud(400, rng), mixed_times(400, taus, rng), imu, 100.0, cfg()))
    rng = np.random.default_rng(106)                        # the largest the API takes: imuPointerCur == 1999
    imu, taus = make_table(100.0, 0.001 + 5e-5 * np.arange(2000), 106)
    out.append(_case("time_table2000", "deskew", cloud(3000, rng), mixed_times(3000, taus, rng), imu, 100.0, cfg()))
    # t0 near 1.7e9: the sum keeps 2^-22 s, so times a few float32 ulps (4e-9 s) off tau_k land ON the entry as well
    rng = np.random.default_rng(107)
    imu, taus = make_table(T0_BIG, taus_70(), 107)
    t = mixed_times(400, taus, rng)
    near = np.arange(0, 400, 5)
    for i, k in zip(near, rng.integers(0, 70, len(near))):
        t[i] = next(v for v in (step(taus[k], j) for j in (1, -1, 2, -2)) if T0_BIG + float(v) == imu[1][k])
    c = _case("time_t0_1.7e9", "deskew", cloud(400, rng), t, imu, T0_BIG, cfg())
    c["expect"]["near"] = near
    out.append(c)
    return out


# ---------------------------------------------------------------- first_*: where the first survivor sits
def _first_case(cid, n, first, seed):
    rng = np.random.default_rng(seed)
    f = cloud(n, rng)
    keep = np.zeros(n, bool)
    if first is not None:
        keep[first] = True
        keep[first + 1:] = rng.random(n - first - 1) < 0.5
    drop(f, np.nonzero(~keep)[0], rng)
    imu, taus = make_table(100.0, taus_70(), seed)
    c = _case(cid, "deskew", f, mixed_times(n, taus, rng), imu, 100.0, cfg(BOX))
    c["expect"].update(first=first, keep=np.nonzero(keep)[0])
    return c


def first_cases():
    out = [_first_case(f"first_{k}", 3000, k, 200 + i) for i, k in enumerate((0, 255, 256, 1023))]
    out.append(_first_case("first_last", 4097, 4096, 210))           # n - 1: lane 0 of a workgroup of its own
    out.append(_first_case("first_last_lane", 4096, 4095, 211))      # n - 1 in the last lane of the last workgroup
    out.append(_first_case("first_none", 1000, None, 212))
    return out


# ---------------------------------------------------------------- compact_*: order-preserving compaction
def _compact_case(n, seed):
    rng = np.random.default_rng(seed)
    f = cloud(n, rng)
    wg = np.arange(n) // 256
    mode = np.array([1, 0, 2, 2, 0, 0, 1, 2])[wg % 8] if n > 257 else np.full(n, 2)   # 0: none survive, 1: all, 2: some
    keep = np.where(mode == 2, rng.random(n) < 0.5, mode == 1)
    if n > 257:
        keep[-1] = True                                               # the last, partial workgroup is not empty
    drop(f, np.nonzero(~keep)[0], rng)
    imu, taus = make_table(100.0, taus_70(), seed)
    c = _case(f"compact_{n}", "deskew", f, mixed_times(n, taus, rng), imu, 100.0, cfg(BOX))
    c["expect"].update(keep=np.nonzero(keep)[0])
    return c


def compact_cases():
    return [_compact_case(n, 300 + i) for i, n in enumerate((255, 256, 257, 65536, 65537))]


# ---------------------------------------------------------------- keep_*: every comparison of IP:596-609 is strict
def _pairs_case(cid, pts, c, seed):
    """pts: (x, y, z, intensity, ring, kept?) rows; a few ordinary points in front and behind."""
    rng = np.random.default_rng(seed)
    a, b = cloud(3, rng), cloud(3, rng)
    for o in (a, b):                                        # within 25 m a side: range < 37
        o["x"], o["y"] = np.clip(o["x"], -25, 25), np.clip(o["y"], -25, 25)
        o["ring"][:] = 0                                    # and on a ring every stride keeps
    cols = list(zip(*pts))
    f = {k: np.concatenate([a[k], np.asarray(cols[j], a[k].dtype), b[k]]) for j, k in enumerate(("x", "y", "z", "intensity", "ring"))}
    n = len(f["x"])
    imu, taus = make_table(100.0, taus_70(), seed)
    case = _case(cid, "deskew", f, mixed_times(n, taus, rng), imu, 100.0, c)
    want = np.array([True] * 3 + [bool(k) for k in cols[5]] + [True] * 3)
    case["expect"].update(keep=np.nonzero(want)[0], dropped=np.nonzero(~want)[0])
    return case


def off_range(x, y, z, axis, up=True):
    """(x, y, z) with one coordinate moved by ulps until the float32 range is exactly one ulp above (below) the original's."""
    p = [F32(x), F32(y), F32(z)]
    want = step(range_f32(x, y, z), 1 if up else -1)
    for j in range(1, 64):
        q = list(p)
        q[axis] = step(p[axis], (j if p[axis] > 0 else -j) * (1 if up else -1))
        r = range_f32(*q)
        if r == want:
            return tuple(q)
        assert (r < want) if up else (r > want), (x, y, z)
    raise AssertionError((x, y, z))


def over_range(x, y, z, axis):
    return off_range(x, y, z, axis, True)


TRIPLES = ((30.0, 40.0, 0.0, 1), (0.0, -30.0, 40.0, 2), (-40.0, 0.0, 30.0, 0), (18.0, 24.0, 40.0, 2))   # range 50 exactly


def keep_cases():
    out = []
    pts = []
    for x, y, z, axis in TRIPLES:                                      # range == maxRange stays, one ulp above goes
        pts.append((x, y, z, 10.0, 3, True))
        pts.append(over_range(x, y, z, axis) + (10.0, 3, False))
    out.append(_pairs_case("keep_range", pts, cfg(lidarMaxRange=50.0), 401))
    up, dn = (lambda v: float(step(v, 1))), (lambda v: float(step(v, -1)))
    pts = [(0.5, 1.0, 0.2, 10.0, 1, True), (0.5, dn(1.0), 0.2, 10.0, 1, False),        # y < lidarMinFront
           (0.5, -5.0, 0.2, 10.0, 1, True), (0.5, up(-5.0), 0.2, 10.0, 1, False),      # -lidarMinBack < y
           (2.0, 0.0, 0.2, 10.0, 1, True), (dn(2.0), 0.0, 0.2, 10.0, 1, False),        # x < lidarMinLeft
           (-2.0, 0.0, 0.2, 10.0, 1, True), (up(-2.0), 0.0, 0.2, 10.0, 1, False),      # -lidarMinRight < x
           (0.0, 3.0, 0.2, 10.0, 1, True), (0.0, -3.0, 0.2, 10.0, 1, False),           # the box reaches 5 m back, 1 m forward
           (1.5, 4.9, 0.2, 10.0, 1, True), (1.5, -4.9, 0.2, 10.0, 1, False),
           (0.0, 0.0, 0.0, 10.0, 1, False), (-0.0, -0.0, 900.0, 10.0, 1, False)]       # the box has no z
    out.append(_pairs_case("keep_box", pts, cfg(BOX), 402))
    pts = [(5.0, 9.0, 1.0, 100.0, 2, True), (5.0, 9.0, 1.0, up(100.0), 2, False), (5.0, 9.0, 1.0, dn(100.0), 2, True),
           (5.0, 9.0, 1.0, -1.0e30, 2, True), (5.0, 9.0, 1.0, 3.0e38, 2, False)]
    out.append(_pairs_case("keep_intensity", pts, cfg(BOX), 403))
    pts = [(5.0, 9.0, 1.0, 10.0, r, r < 16 and r % 3 == 0) for r in (0, 1, 2, 3, 14, 15, 16, 17, 18, 32, 48, 255, 256, 32768, 65535)]
    out.append(_pairs_case("keep_ring", pts, cfg(downsampleRate=3), 404))
    c = _pairs_case("keep_rate_above_n_scan", [(5.0, 9.0, 1.0, 10.0, r, r == 0) for r in (0, 1, 15, 16, 17, 34, 0)],
                    cfg(downsampleRate=17), 405)
    ring = c["ring"]; ring[:3] = 0; ring[-3:] = 17                     # (the ordinary points: ring 0 stays, ring 17 goes)
    c["expect"].update(keep=np.nonzero(ring == 0)[0], dropped=np.nonzero(ring != 0)[0])
    out.append(c)
    rng = np.random.default_rng(406)                                   # point_filter_num > n: point 0 alone
    imu, taus = make_table(100.0, taus_70(), 406)
    c = _case("keep_filter_num_above_n", "deskew", cloud(300, rng), mixed_times(300, taus, rng), imu, 100.0, cfg(point_filter_num=301))
    c["expect"].update(keep=np.array([0]), dropped=np.arange(1, 300))
    out.append(c)
    rng = np.random.default_rng(407)                                   # the stride counts INPUT indices, dropped ones included
    f = cloud(300, rng)
    gone = np.arange(0, 300, 6)
    drop(f, gone, rng)
    c = _case("keep_filter_num_3", "deskew", f, mixed_times(300, taus, rng), imu, 100.0, cfg(BOX, point_filter_num=3))
    c["expect"].update(keep=np.arange(3, 300, 6), dropped=np.setdiff1d(np.arange(300), np.arange(3, 300, 6)))
    out.append(c)
    return out


# ---------------------------------------------------------------- nan_*: NaN passes every gate
def nan_cases():
    out = []
    rng = np.random.default_rng(501)
    imu, taus = make_table(100.0, taus_70(), 501)
    f = cloud(300, rng)
    f["x"][[7, 70, 299]] = np.nan                                      # 3 outputs each (x enters all three rows, IP:569-571)
    f["y"][[8]] = np.nan; f["z"][[9]] = np.nan
    f["intensity"][[10, 11]] = np.nan                                  # copied through, IP:572
    c = _case("nan_x", "deskew", f, mixed_times(300, taus, rng), imu, 100.0, cfg(BOX), nan=True)
    c["expect"].update(n_keep=300, nans=3 * 5 + 2)
    out.append(c)
    rng = np.random.default_rng(502)
    t = mixed_times(300, taus, rng)
    t[[5, 64, 255, 256]] = np.nan                                      # front runs to the last entry, the ratios are NaN
    c = _case("nan_time", "deskew", cloud(300, rng), t, imu, 100.0, cfg(BOX), nan=True)
    c["expect"].update(n_keep=300, nans=3 * 4, nan_times=4)
    out.append(c)
    rng = np.random.default_rng(503)                                   # NaN time at the FIRST survivor: transStartInverse is NaN
    f = cloud(300, rng)
    drop(f, [0, 1], rng)
    t = mixed_times(300, taus, rng)
    t[2] = np.nan
    c = _case("nan_time_first", "deskew", f, t, imu, 100.0, cfg(BOX), nan=True)
    c["expect"].update(n_keep=298, nans=3 * 298, nan_times=1)
    out.append(c)
    rng = np.random.default_rng(504)                                   # the last two stamps equal, points exactly on them: 0 / 0
    tau = taus_70(); tau[69] = tau[68]
    imu2, tau = make_table(100.0, tau, 504)
    t = times_of(rng.choice(["before", "inside", "on_entry"], 300), tau[:68], rng)
    on = np.array([3, 63, 128, 299])
    t[on] = tau[69]
    c = _case("nan_stamps_equal", "deskew", cloud(300, rng), t, imu2, 100.0, cfg(BOX), nan=True)
    c["expect"].update(n_keep=300, nans=3 * 4, on=on)
    out.append(c)
    return out


# ---------------------------------------------------------------- pc2_*: the conversions of cachePointCloud IP:226-285
def _blob(n, step_, fields, seed):
    """A PointCloud2 data blob: `fields` = (offset, array) pairs; every other byte is noise."""
    b = np.random.default_rng(seed).integers(0, 256, (n, step_), dtype=np.uint8)
    for off, a in fields:
        a = np.ascontiguousarray(a)
        b[:, off:off + a.dtype.itemsize] = a.view(np.uint8).reshape(n, a.dtype.itemsize)
    return b


PC2_UINT8, PC2_UINT16, PC2_INT32 = 2, 4, 5                 # sensor_msgs/PointField datatypes (include/liogpu.h)


def pc2_cases():
    out = []
    n = 600
    # Mulran: int32 ring, `dst.ring = src.ring` narrows to uint16 (IP:261); uint32 t taken as is (IP:262)
    rng = np.random.default_rng(601)
    f = cloud(n, rng)
    ring32 = f["ring"].astype(np.int32)
    ring32[0::7] = 65536 + (ring32[0::7] % 16)              # 65 539 -> 3: in range after narrowing
    ring32[1::7] = -1                                       # -> 65 535: out
    ring32[2::7] = 65536 + 16                               # -> 16: out (N_SCAN 16)
    ring32[3::7] = -65536 + 5                               # -> 5: in
    ticks = rng.integers(0, 140, n).astype(np.uint32)
    imu, taus = make_table(100.0, 10.0 + 2.0 * np.arange(60), 601)     # entries at even ticks 10 .. 128
    blob = _blob(n, 32, [(0, f["x"]), (4, f["y"]), (8, f["z"]), (16, f["intensity"]), (20, ticks), (24, ring32)], 601)
    f["ring"] = ring32.astype(np.uint16)
    c = _case("pc2_int32_ring", "pc2", f, ticks.astype(F32), imu, 100.0, cfg(BOX), blob=blob,
              layout=dict(point_step=32, off_x=0, off_intensity=16, off_ring=24, ring_type=PC2_INT32, off_time=20, time_type=2))
    c["expect"].update(keep=np.nonzero(f["ring"] < 16)[0], ring32=ring32)
    out.append(c)
    # Ouster: uint8 ring up to 255, uint32 nanoseconds above 2^31 (dst.time = src.t * 1e-9f, IP:243)
    for cid, n_scan, seed in (("pc2_uint8_ring_255_in", 256, 602), ("pc2_uint8_ring_255_out", 255, 603)):
        rng = np.random.default_rng(seed)
        f = cloud(n, rng, 256)
        f["ring"][::5] = 255
        ns = rng.integers(2 ** 31 + 1000, 2 ** 32 - 1000, n).astype(np.uint32)
        ns[:4] = [2 ** 31 + 1, 2 ** 32 - 1, 2 ** 31 + 129, 3000000000]
        imu, taus = make_table(T0_BIG, 2.4 + 0.027 * np.arange(60), seed)          # 2.4 .. 3.99 s: before, inside and after
        blob = _blob(n, 48, [(0, f["x"]), (4, f["y"]), (8, f["z"]), (16, f["intensity"]), (20, ns), (26, f["ring"].astype(np.uint8))], seed)
        c = _case(cid, "pc2", f, ns.astype(F32) * F32(1e-9), imu, T0_BIG, cfg(BOX, N_SCAN=n_scan), blob=blob,
                  layout=dict(point_step=48, off_x=0, off_intensity=16, off_ring=26, ring_type=PC2_UINT8, off_time=20, time_type=1))
        c["expect"].update(keep=np.nonzero(f["ring"] < n_scan)[0], ns=ns)
        out.append(c)
    # Robosense: double stamps, time = stamp - the first point's (IP:269, 281); 28-byte records put the double at
    # offsets 20, 48, 76, ...: 4-aligned, every other one not 8-aligned
    rng = np.random.default_rng(604)
    f = cloud(n, rng)
    base = 1.7e9 + 0.05                                     # the first point's stamp; fp64 keeps 2^-22 s of a stamp
    quant = lambda r: ((base + np.asarray(r, np.float64)) - base).astype(F32)      # noqa: E731  (what IP:281 recovers)
    taus = taus_70()
    imu, tq = make_table(T0_BIG, quant(taus), 604)
    rel = mixed_times(n, taus, rng)
    rel[0] = 0.0
    stamp = base + rel.astype(np.float64)
    assert stamp[0] == base and np.array_equal((stamp - stamp[0]).astype(F32), quant(rel))
    blob = _blob(n, 28, [(0, f["x"]), (4, f["y"]), (8, f["z"]), (12, f["intensity"]), (16, f["ring"]), (20, stamp)], 604)
    c = _case("pc2_f64_stamp_unaligned", "pc2", f, quant(rel), imu, T0_BIG, cfg(BOX), blob=blob,
              layout=dict(point_step=28, off_x=0, off_intensity=12, off_ring=16, ring_type=PC2_UINT16, off_time=20, time_type=3))
    c["expect"].update(keep=np.arange(n))
    out.append(c)
    return out


# ---------------------------------------------------------------- ri_*: the range image
RI = dict(N_SCAN=16, downsampleRate=1, lidarMaxRange=1000.0, deskew_flag=1)


def _ri_case(cid, f, H, seed, c=None, min_range=1.0, t0=100.0):
    rng = np.random.default_rng(seed)
    imu, taus = make_table(t0, taus_70(), seed)
    return _case(cid, "ri", f, mixed_times(len(f["x"]), taus, rng), imu, t0, dict(RI, **(c or {})), H=H, minRange=min_range)


def _fields(x, y, z, ring, rng):
    n = len(x)
    return {"x": np.asarray(x, F32), "y": np.asarray(y, F32), "z": np.asarray(z, F32),
            "intensity": rng.uniform(0.0, 255.0, n).astype(F32), "ring": np.asarray(ring, np.uint16)}


def grid_points(n_scan, H, rng, rings=None, fill=1.0):
    """One point at the centre of a fraction `fill` of the cells of the given rings, in shuffled order."""
    rings = np.arange(n_scan) if rings is None else np.asarray(rings)
    ring, col = np.meshgrid(rings, np.arange(H), indexing="ij")
    ring, col = ring.reshape(-1), col.reshape(-1)
    if fill < 1.0:
        sel = rng.random(len(ring)) < fill
        ring, col = ring[sel], col[sel]
    order = rng.permutation(len(ring))
    ring, col = ring[order], col[order]
    a = np.radians(90.0 - (col - H // 2) * (360.0 / H))     # horizonAngle of the column's centre, measured from +y
    r = rng.uniform(3.0, 80.0, len(ring))
    f = _fields(r * np.sin(a), r * np.cos(a), rng.uniform(-2.0, 2.0, len(ring)), ring, rng)
    f["col"] = col
    return f


def boundary_points(H, want, r=10.0):
    """Points whose horizonAngle sits exactly on a column boundary -- (horizonAngle - 90) / ang_res_x == k + 0.5, a tie of
    round() -- each with its nearest float neighbours on either side.  H must make 360 / H exact in float32.
    -> list of (tie point, lower neighbour, upper neighbour) as (x, y)."""
    res = float(F32(360.0 / H))
    assert res == 360.0 / H
    found = []
    for k in range(-H + 3, 0, max(1, H // 97)):             # (horizonAngle - 90) / res lies in (-H * 3/4, H / 4]
        h_tie = 90.0 + (k + 0.5) * res
        if not -179.0 < h_tie < 179.0 or float(F32(h_tie)) != h_tie:
            continue
        a = math.radians(h_tie)
        y, x0 = F32(r * math.cos(a)), F32(r * math.sin(a))
        by_h = {}
        for j in range(-40, 41):
            x = step(x0, j)
            by_h.setdefault(float(column_of(x, y, H)[0]), (float(x), float(y)))
        if h_tie in by_h:
            lo = max((h for h in by_h if h < h_tie), default=None)
            hi = min((h for h in by_h if h > h_tie), default=None)
            if lo is not None and hi is not None:
                found.append((by_h[h_tie], by_h[lo], by_h[hi]))
        if len(found) == want:
            break
    assert len(found) == want, (H, len(found))
    return found


def ri_cases():
    out = []
    # axes, diagonals, the pole (0, 0, z), and both zeros on the -y half-axis (atan2 = +pi and -pi: the same column,
    # once directly and once through `col -= H`)
    rng = np.random.default_rng(701)
    xy = [(10, 0), (-10, 0), (0, 10), (0, -10), (-0.0, -10), (10, 10), (-10, 10), (10, -10), (-10, -10), (0, 0), (-0.0, 0.0),
          (0.0, -0.0), (-0.0, -0.0), (-7, 0.0), (-7, -0.0)]
    x = [p[0] for p in xy]; y = [p[1] for p in xy]
    f = _fields(x, y, rng.uniform(2.0, 5.0, len(xy)), np.arange(len(xy)) % 4, rng)
    out.append(_ri_case("ri_axes", f, 1800, 701, dict(N_SCAN=4)))
    f = _fields(x, y, rng.uniform(2.0, 5.0, len(xy)), np.arange(len(xy)) % 4, rng)
    out.append(_ri_case("ri_axes_odd_H", f, 1801, 702, dict(N_SCAN=4)))
    for H, seed in ((720, 703), (2048, 704)):
        trip = boundary_points(H, 12)
        pts = [p for t in trip for p in t]
        f = _fields([p[0] for p in pts], [p[1] for p in pts], np.zeros(len(pts)), np.zeros(len(pts)), np.random.default_rng(seed))
        c = _ri_case(f"ri_boundaries_{H}", f, H, seed, dict(N_SCAN=1))
        c["expect"]["triples"] = len(trip)
        out.append(c)
    # the wrap: azimuths within a few columns of the -x axis, where the rule gives H, H + 1, ... before `col -= H`
    rng = np.random.default_rng(705)
    a = np.radians(-90.0 + rng.uniform(-1.0, 1.0, 300))
    f = _fields(20.0 * np.sin(a), 20.0 * np.cos(a), rng.uniform(-1, 1, 300), rng.integers(0, 16, 300), rng)
    out.append(_ri_case("ri_wrap", f, 1800, 705))
    # grid sizes: one column, the widest grid, an odd width, one ring, 1024 rings
    rng = np.random.default_rng(706)
    a = rng.uniform(-np.pi, np.pi, 300)
    f = _fields(9.0 * np.sin(a), 9.0 * np.cos(a), rng.uniform(-1, 1, 300), rng.integers(0, 5, 300), rng)
    out.append(_ri_case("ri_H_1", f, 1, 706, dict(N_SCAN=4)))
    out.append(_ri_case("ri_H_32767", grid_points(4, 32767, np.random.default_rng(707), fill=0.1), 32767, 707, dict(N_SCAN=4)))
    out.append(_ri_case("ri_n_scan_1", grid_points(1, 1800, np.random.default_rng(708)), 1800, 708, dict(N_SCAN=1)))
    out.append(_ri_case("ri_n_scan_1024", grid_points(1024, 37, np.random.default_rng(709), fill=0.7), 37, 709, dict(N_SCAN=1024)))
    # the exclusive scan's 4096-cell tile: 64 x 64 = 4096 and 17 x 241 = 4097 cells, every one occupied
    out.append(_ri_case("ri_cells_4096", grid_points(64, 64, np.random.default_rng(710)), 64, 710, dict(N_SCAN=64)))
    out.append(_ri_case("ri_cells_4097", grid_points(17, 241, np.random.default_rng(711)), 241, 711, dict(N_SCAN=17)))
    # range gates: exactly minRange and exactly maxRange stay (both comparisons strict), one ulp outside goes
    pts = []
    for x, y, z, axis in TRIPLES:
        pts += [(x, y, z, True), over_range(x, y, z, axis) + (False,)]
    for x, y, z, axis in TRIPLES[:3]:                                  # a tenth of it: range 5 exactly
        pts += [(x / 10, y / 10, z / 10, True), off_range(x / 10, y / 10, z / 10, axis, up=False) + (False,)]
    rng = np.random.default_rng(712)
    f = _fields([p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], np.arange(len(pts)) % 16, rng)
    c = _ri_case("ri_range_gates", f, 1800, 712, dict(lidarMaxRange=50.0), min_range=5.0)
    c["expect"].update(keep=np.nonzero([p[3] for p in pts])[0])
    out.append(c)
    # thousands of points in one cell: the first INPUT index wins, whatever order the atomics land in
    rng = np.random.default_rng(713)
    g = grid_points(16, 1800, rng, fill=0.2)
    n = len(g["x"])
    dense = np.sort(rng.choice(np.arange(50, n), 5000, replace=False))
    a0 = math.radians(33.37)
    r = rng.uniform(3.0, 80.0, 5000)
    g["x"][dense] = r * math.sin(a0); g["y"][dense] = r * math.cos(a0); g["ring"][dense] = 7
    del g["col"]
    c = _ri_case("ri_dense_cell", g, 1800, 713)
    c["expect"].update(dense=dense)
    out.append(c)
    return out


def nan_ri_cases():
    # NaN x or y: no azimuth, the point is dropped (and must not land in the empty column 0); NaN z or NaN time: the point keeps
    # its cell and carries NaN into x, y, z (and, for z, into the range)
    rng = np.random.default_rng(801)
    f = grid_points(4, 360, rng, fill=0.5)
    free = f.pop("col") != 0                                # column 0 stays free: (int)NaN = 0 would put the NaN points there
    f = {k: v[free] for k, v in f.items()}
    n = len(f["x"])
    nx, ny, nz, nt = np.arange(10, 60, 7), np.arange(11, 60, 7), np.arange(12, 60, 7), np.arange(13, 60, 7)
    f["x"][nx] = np.nan; f["y"][ny] = np.nan; f["z"][nz] = np.nan
    c = _ri_case("nan_range_image", f, 360, 801, dict(N_SCAN=4))
    c["time"][nt] = np.nan
    c["nan"] = True
    c["expect"].update(n_cells=n - len(nx) - len(ny), nans=4 * len(nz) + 3 * len(nt), dropped=np.concatenate([nx, ny]))
    return [c]


CASES = {"time": time_cases, "first": first_cases, "compact": compact_cases, "keep": keep_cases, "nan": nan_cases,
         "pc2": pc2_cases, "ri": ri_cases, "nan_ri": nan_ri_cases}
_BUILT, _REFS = {}, {}


def cases(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def all_cases():
    return [c for name in CASES for c in cases(name)]


# ---------------------------------------------------------------- fuzz: the rules above, mixed
FUZZ_N = (1, 63, 64, 255, 256, 257, 4097, 20000)
FUZZ_TABLE = (2, 3, 70, 2000)


def fuzz_trial(t):
    """Trial t -> (case, the parameters as a string).  The case runs through lio_deskew and, with its H and minRange,
    through lio_range_image."""
    rng = np.random.default_rng(3000 + t)
    n = int(FUZZ_N[t % len(FUZZ_N)] if t < len(FUZZ_N) else rng.choice(FUZZ_N))
    k = int(FUZZ_TABLE[t % len(FUZZ_TABLE)] if t < 2 * len(FUZZ_TABLE) else rng.choice(FUZZ_TABLE))
    t0 = float(rng.choice([100.0, T0_BIG]))
    n_scan = int(rng.choice([16, 64]))
    imu, taus = make_table(t0, 0.01 + (0.14 / k) * np.arange(k), 4000 + t, amp=float(rng.choice([0.05, 0.3, 1.5])))
    f = cloud(n, rng, n_scan + 2)                           # rings N_SCAN and N_SCAN + 1 are out
    some = lambda p: np.nonzero(rng.random(n) < p)[0]       # noqa: E731
    drop(f, some(0.3), rng, n_scan)
    on = some(0.05)                                         # exactly on the range gate, and on the axes
    f["x"][on], f["y"][on], f["z"][on] = rng.choice([-30.0, 0.0, 30.0], len(on)), 40.0, 0.0
    ax = some(0.05)
    f["x"][ax] = 0.0
    c = cfg(BOX, N_SCAN=n_scan, downsampleRate=int(rng.choice([1, 2, 3, n_scan + 1])),
            point_filter_num=int(rng.choice([1, 1, 2, 3, n + 1])), lidarMaxRange=float(rng.choice([50.0, 1000.0])))
    H = int(rng.choice([1, 37, 720, 1800, 2048]))
    case = _case(f"fuzz-{t}", "deskew", f, mixed_times(n, taus, rng), imu, t0, c, H=H, minRange=float(rng.choice([0.0, 1.0, 5.0])))
    what = (f"trial {t}: n {n}, table {k}, t0 {t0!r}, N_SCAN {n_scan}, downsampleRate {c['downsampleRate']}, "
            f"point_filter_num {c['point_filter_num']}, maxRange {c['lidarMaxRange']}, H {H}, minRange {case['minRange']}")
    return case, what


# ---------------------------------------------------------------- the oracle on a case
def oracle_cfg(case):
    import oracle.oracle as om
    c = dict(OPEN, **case["cfg"])
    return om.DeskewConfig(imu_available=1 if case["imu"][0] > 0 else 0, trig_mode=0, **c)


def run_oracle(oracle, case, kind=None):
    """deskew / pc2 -> {cloud, keep}; ri -> {cloud, col, range, start_ring, end_ring}."""
    if (kind or case["kind"]) == "ri":
        xyz = np.stack([case["x"], case["y"], case["z"]], 1)
        return oracle.range_image(oracle_cfg(case), case["H"], case["minRange"], xyz, case["intensity"], case["ring"],
                                  case["time"], case["t0"], case["imu"])
    out, keep = oracle.project_point_cloud(oracle_cfg(case), case["x"], case["y"], case["z"], case["intensity"], case["ring"],
                                           case["time"], case["t0"], case["imu"])
    return {"cloud": out, "keep": keep}


def reference(oracle, case):
    """The oracle's outputs for a named case, computed once per process and shared (treat as read-only)."""
    if case["id"] not in _REFS:
        _REFS[case["id"]] = run_oracle(oracle, case)
    return _REFS[case["id"]]


# ---------------------------------------------------------------- the device on a case
def records(pkg, case):
    return pkg.pack_xyzirt(np.stack([case["x"], case["y"], case["z"]], 1), case["intensity"], case["ring"], case["time"])


def run_device(pkg, case, kind=None):
    kind = kind or case["kind"]
    if kind == "ri":
        c = case["cfg"]
        return pkg.range_image(records(pkg, case), case["t0"], case["imu"], N_SCAN=c["N_SCAN"], Horizon_SCAN=case["H"],
                               downsampleRate=c["downsampleRate"], lidarMinRange=case["minRange"],
                               lidarMaxRange=c["lidarMaxRange"], deskew_flag=c["deskew_flag"])
    dcfg = pkg.deskew_default_config(**case["cfg"])
    if kind == "pc2":
        return {"cloud": pkg.deskew_pc2(dcfg, case["blob"], len(case["x"]), pkg.PC2Layout(**case["layout"]), case["t0"], case["imu"])}
    return {"cloud": pkg.deskew(dcfg, records(pkg, case), case["t0"], case["imu"])}


# ---------------------------------------------------------------- bit for bit
def _diff_f32(name, a, b, nan_ok):
    if a.shape != b.shape:
        return f"{name}: {a.shape[0]} entries, reference {b.shape[0]}"
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    bad = ua != ub
    if nan_ok:                                              # NaN in the same elements, every other element bit-equal
        na, nb = np.isnan(a), np.isnan(b)
        bad = (na != nb) | (bad & ~(na & nb))
    elif np.isnan(a).any() or np.isnan(b).any():
        return f"{name}: NaN in a finite case ({int(np.isnan(a).sum())} device / {int(np.isnan(b).sum())} reference)"
    if bad.any():
        rows = np.unique(np.nonzero(bad)[0])
        i = int(rows[0])
        return f"{name}: {len(rows)} of {len(b)} entries differ, first at {rows[:12].tolist()}: {a[i].tolist()} vs reference {b[i].tolist()}"
    return ""


def diff_report(out, ref, nan_ok=False):
    """'' when the outputs agree (uint32 views equal; in a nan_* case NaN for NaN), else what differs."""
    msgs = [_diff_f32("cloud", out["cloud"], ref["cloud"], nan_ok)]
    if "col" in ref:
        msgs.append(_diff_f32("range", out["range"], ref["range"], nan_ok))
        for k in ("col", "start_ring", "end_ring"):
            if out[k].shape != ref[k].shape or not np.array_equal(out[k], ref[k]):
                bad = np.nonzero(out[k] != ref[k])[0] if out[k].shape == ref[k].shape else []
                msgs.append(f"{k}: {len(bad)} of {len(ref[k])} differ, first at {list(bad[:12])}")
    return "\n".join(m for m in msgs if m)


def compare(pkg, ref, case, what="", kind=None):
    out = run_device(pkg, case, kind)
    rep = diff_report(out, ref, case["nan"])
    assert not rep, f"{what or case['id']}\n{rep}"
    return out
