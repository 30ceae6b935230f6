"""The cases of tests/deskew_cases.py, the part that needs no GPU: for every named case the inputs and the oracle's own
outputs show that the case reaches the edge it is named for (so tests/test_gpu_deskew_edges.py cannot pass vacuously),
and the small cases pin lo_project_point_cloud and lo_range_image bit for bit against a literal Python transcription of
findRotation IP:502-527, deskewPoint + projectPointCloud IP:545-615 and the column rule.  Every test prints the counts
that prove its edge (pytest -s)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deskew_cases as D                                  # noqa: E402

F32 = np.float32


def _cases(name):
    return {c["id"]: c for c in D.cases(name)}


def _finite(ref):
    return all(np.isfinite(ref[k]).all() for k in ("cloud", "range") if k in ref)


def _survivors(oracle, c, want=None):
    """The oracle's survivors; `want` (default: expect['keep']) must be exactly them."""
    ref = D.reference(oracle, c)
    want = c["expect"]["keep"] if want is None else want
    assert np.array_equal(ref["keep"], want), c["id"]
    assert len(ref["cloud"]) == len(want)
    if not c["nan"]:
        assert _finite(ref), c["id"]
    return ref


# ---------------------------------------------------------------- edge proofs
def test_time_cases_take_every_branch(oracle):
    cs = _cases("time")
    counts = {cid: D.branch_counts(c) for cid, c in cs.items()}
    for cid, k in counts.items():
        print(cid, k)
        assert k["nan"] == 0 and sum(k.values()) == len(cs[cid]["x"])
        _survivors(oracle, cs[cid], np.arange(len(cs[cid]["x"])))           # no gate shuts: every point is deskewed
    assert counts["time_before"] == dict(before=400, after=0, on_last=0, on_entry=0, inside=0, nan=0)
    assert counts["time_after"] == dict(before=0, after=400, on_last=0, on_entry=0, inside=0, nan=0)
    assert counts["time_on_entries"] == dict(before=0, after=0, on_last=133, on_entry=267, inside=0, nan=0)
    c = cs["time_on_entries"]
    pt = c["t0"] + c["time"].astype(np.float64)
    assert [int((pt == c["imu"][1][k]).sum()) for k in (0, 34, 69)] == [134, 133, 133]
    for cid in ("time_mixed", "time_table2", "time_table2000", "time_t0_1.7e9"):
        assert min(counts[cid][k] for k in D.KINDS) >= 20, cid
    assert cs["time_table2"]["imu"][0] == 1 and len(cs["time_table2"]["imu"][1]) == 2
    assert cs["time_table2000"]["imu"][0] == 1999 and len(cs["time_table2000"]["imu"][1]) == 2000
    # t0 near 1.7e9: times that differ from every tau_k as float32 still land ON an entry once t0 is added
    c = cs["time_t0_1.7e9"]
    near = c["expect"]["near"]
    taus = D.taus_70()
    assert not np.isin(c["time"][near], taus).any()
    k = D.branch_counts(c, near)
    print("time_t0_1.7e9: off-entry float32 times that land on an entry:", k)
    assert k["on_entry"] + k["on_last"] == len(near) == 80
    small = dict(c, t0=100.0, imu=D.make_table(100.0, taus, 107)[0])        # the same times at a small t0 stay off
    k = D.branch_counts(small, near)
    assert k["on_entry"] + k["on_last"] == 0


def test_first_survivor_sits_where_the_case_says(oracle):
    cs = _cases("first")
    for cid, first in (("first_0", 0), ("first_255", 255), ("first_256", 256), ("first_1023", 1023), ("first_last", 4096),
                       ("first_last_lane", 4095)):
        c = cs[cid]
        ref = _survivors(oracle, c)
        n = len(c["x"])
        print(f"{cid}: n {n}, first survivor {int(ref['keep'][0])}, {len(ref['keep'])} survivors")
        assert int(ref["keep"][0]) == first == c["expect"]["first"]
        if cid.startswith("first_last"):
            assert first == n - 1 and len(ref["keep"]) == 1
            assert (first % 256 == 255) == (cid == "first_last_lane")
        else:
            assert len(ref["keep"]) > 500
            # the point after the first survivor takes another rotation: reading it instead would show
            assert c["time"][first] != c["time"][first + 1]
    assert 1023 % 256 == 255 and (1023 % 256) // 64 == 3 and 1023 % 64 == 63           # wave 3, lane 63
    ref = _survivors(oracle, cs["first_none"], np.zeros(0, int))
    assert len(ref["cloud"]) == 0 and len(cs["first_none"]["x"]) == 1000


def test_compaction_sizes_and_workgroup_patterns(oracle):
    cs = _cases("compact")
    assert sorted(len(c["x"]) for c in cs.values()) == [255, 256, 257, 65536, 65537]
    for cid, c in cs.items():
        ref = _survivors(oracle, c)
        n = len(c["x"])
        flags = np.zeros(n, bool); flags[ref["keep"]] = True
        per_wg = np.add.reduceat(flags, np.arange(0, n, 256))
        size = np.minimum(256, n - np.arange(0, n, 256))
        print(f"{cid}: {len(per_wg)} workgroups, {int((per_wg == 0).sum())} empty, {int((per_wg == size).sum())} full, "
              f"{len(ref['keep'])} survivors")
        assert len(per_wg) == (n + 255) // 256 and 0 < len(ref["keep"]) < n
        if n > 257:
            assert len(per_wg) in (256, 257)
            assert (per_wg == 0).sum() >= 60 and (per_wg == size).sum() >= 60 and ((per_wg > 0) & (per_wg < size)).sum() >= 60
            assert per_wg[-1] > 0


def test_keep_thresholds_are_strict(oracle):
    cs = _cases("keep")
    for cid, c in cs.items():
        ref = _survivors(oracle, c)
        print(f"{cid}: kept {ref['keep'].tolist()[:24]}, dropped {c['expect']['dropped'].tolist()[:24]}")
        assert len(c["expect"]["dropped"]) + len(ref["keep"]) == len(c["x"])
    c = cs["keep_range"]                                   # rows 3.. alternate on-threshold / one ulp above
    r = np.array([D.range_f32(c["x"][i], c["y"][i], c["z"][i]) for i in range(3, 3 + 2 * len(D.TRIPLES))])
    assert (r[0::2] == F32(50.0)).all() and (r[1::2] == D.step(50.0, 1)).all() and c["cfg"]["lidarMaxRange"] == 50.0
    assert np.isin(np.arange(3, 11, 2), c["expect"]["keep"]).all() and np.isin(np.arange(4, 11, 2), c["expect"]["dropped"]).all()
    c = cs["keep_box"]                                     # on the face: kept; one ulp inside: dropped
    g = c["cfg"]
    for i, (axis, face) in zip(range(3, 11, 2), (("y", g["lidarMinFront"]), ("y", -g["lidarMinBack"]),
                                                 ("x", g["lidarMinLeft"]), ("x", -g["lidarMinRight"]))):
        assert c[axis][i] == F32(face) and c[axis][i + 1] in (D.step(face, 1), D.step(face, -1)) and abs(c[axis][i + 1]) < abs(face)
        assert i in c["expect"]["keep"] and i + 1 in c["expect"]["dropped"]
    assert c["y"][11] == -c["y"][12] == 3.0 and 11 in c["expect"]["keep"] and 12 in c["expect"]["dropped"]     # the asymmetry
    c = cs["keep_intensity"]
    assert c["intensity"][3] == F32(c["cfg"]["lidarMaxIntensity"]) and c["intensity"][4] == D.step(100.0, 1)
    assert 3 in c["expect"]["keep"] and 4 in c["expect"]["dropped"]
    c = cs["keep_ring"]
    kept = set(c["ring"][c["expect"]["keep"]].tolist())
    assert c["cfg"]["N_SCAN"] == 16 and {0, 3, 15} <= kept and not kept & {16, 18, 48, 255, 65535}
    c = cs["keep_rate_above_n_scan"]
    assert c["cfg"]["downsampleRate"] > c["cfg"]["N_SCAN"] and set(c["ring"][c["expect"]["keep"]].tolist()) == {0}
    assert {15, 17, 34} <= set(c["ring"][c["expect"]["dropped"]].tolist())
    c = cs["keep_filter_num_above_n"]
    assert c["cfg"]["point_filter_num"] > len(c["x"]) and c["expect"]["keep"].tolist() == [0]
    c = cs["keep_filter_num_3"]
    assert (c["expect"]["keep"] % 3 == 0).all() and len(c["expect"]["keep"]) == 50


def test_nan_cases_hold_the_predicted_nans(oracle):
    cs = _cases("nan")
    for cid, c in cs.items():
        assert c["nan"]
        ref = D.reference(oracle, c)
        nans = int(np.isnan(ref["cloud"]).sum())
        print(f"{cid}: {len(ref['cloud'])} survivors, {nans} NaN of {ref['cloud'].size} outputs; branches {D.branch_counts(c)}")
        assert len(ref["cloud"]) == c["expect"]["n_keep"]                   # NaN passes every gate
        assert nans == c["expect"]["nans"] and 0 < nans < ref["cloud"].size
    c = cs["nan_x"]
    assert int(np.isnan(c["x"]).sum()) == 3 and np.isnan(D.reference(oracle, c)["cloud"][[7, 70, 299], :3]).all()
    assert D.branch_counts(cs["nan_time"])["nan"] == 4
    c = cs["nan_time_first"]
    ref = D.reference(oracle, c)
    assert int(ref["keep"][0]) == 2 and np.isnan(c["time"][2]) and np.isnan(ref["cloud"][:, :3]).all()
    assert np.isfinite(ref["cloud"][:, 3]).all()
    c = cs["nan_stamps_equal"]
    T = c["imu"][1]
    assert T[68] == T[69] and np.isfinite(c["time"]).all() and all(np.isfinite(c[k]).all() for k in "xyz")
    pt = c["t0"] + c["time"].astype(np.float64)
    assert np.array_equal(np.nonzero(pt == T[69])[0], c["expect"]["on"])
    assert np.isnan(D.reference(oracle, c)["cloud"][c["expect"]["on"], :3]).all()


def test_layout_cases_narrow_and_convert(oracle):
    cs = _cases("pc2")
    for cid, c in cs.items():
        ref = _survivors(oracle, c, np.intersect1d(c["expect"]["keep"], np.arange(len(c["x"]))))
        k = D.branch_counts(c)
        print(f"{cid}: {len(ref['keep'])} of {len(c['x'])} survive; branches {k}")
        assert k["before"] > 10 and k["after"] > 10 and k["inside"] > 10
    c = cs["pc2_int32_ring"]
    r32 = c["expect"]["ring32"]
    assert {65539, -1, 65552, -65531} <= set(r32.tolist())
    narrowed = dict(zip(r32.tolist(), c["ring"].tolist()))
    assert narrowed[65539] == 3 and narrowed[-1] == 65535 and narrowed[65552] == 16 and narrowed[-65531] == 5
    kept = set(r32[c["expect"]["keep"]].tolist())
    assert 65539 in kept and -65531 in kept and -1 not in kept and 65552 not in kept
    a, b = cs["pc2_uint8_ring_255_in"], cs["pc2_uint8_ring_255_out"]
    assert (a["ring"] == 255).sum() >= 120 and np.isin(np.nonzero(a["ring"] == 255)[0], a["expect"]["keep"]).all()
    assert not np.isin(np.nonzero(b["ring"] == 255)[0], b["expect"]["keep"]).any() and len(b["expect"]["keep"]) > 400
    for c in (a, b):
        assert c["expect"]["ns"].min() > 2 ** 31 and c["expect"]["ns"].max() == 2 ** 32 - 1
        assert c["time"].min() > 2.14 and c["time"].max() < 4.3
    c = cs["pc2_f64_stamp_unaligned"]
    off = c["layout"]["off_time"] + c["layout"]["point_step"] * np.arange(len(c["x"]))
    assert (off % 4 == 0).all() and (off % 8 != 0).sum() == len(off) // 2
    assert c["time"][0] == 0.0 and D.branch_counts(c)["on_entry"] > 10


def test_range_image_cases_reach_their_cells(oracle):
    cs = _cases("ri")
    refs = {cid: D.reference(oracle, c) for cid, c in cs.items()}
    for cid, ref in refs.items():
        assert _finite(ref), cid
        print(f"{cid}: {len(cs[cid]['x'])} points -> {len(ref['cloud'])} cells of {cs[cid]['cfg']['N_SCAN']} x {cs[cid]['H']}")

    def cols(c):
        return [D.column_of(x, y, c["H"]) for x, y in zip(c["x"], c["y"])]

    for cid, H in (("ri_axes", 1800), ("ri_axes_odd_H", 1801)):
        c = cs[cid]
        k = cols(c)
        print(f"{cid}: (horizonAngle, column before the wrap, column) = {[(float(a), b, d) for a, b, d in k]}")
        want = [90, -90, 0, 180, -180, 45, -45, 135, -135, 0, 0, 180, -180, -90, -90]     # atan2(x, y) of the fifteen points
        assert all(abs(float(r[0]) - w) < 1e-4 for r, w in zip(k, want))
        assert k[1][1] >= H and k[1][2] == 0                                # -x: through `col -= H` into column 0
        assert k[3][1] < H <= k[4][1] and abs(k[3][2] - k[4][2]) <= 1       # -y: directly (+180) and through the wrap (-180)
        assert k[9][2] == k[10][2] == k[2][2]                               # the pole (0, 0, z): atan2(0, 0) = 0, the +y column
        assert len(refs[cid]["cloud"]) >= 8
    k = cols(cs["ri_axes"])
    assert [r[1] for r in k[:5]] == [900, 1800, 1350, 450, 2250] and [r[2] for r in k[:5]] == [900, 0, 1350, 450, 450]
    for H in (720, 2048):
        c = cs[f"ri_boundaries_{H}"]
        k = cols(c)
        res = 360.0 / H
        ties = 0
        for t in range(c["expect"]["triples"]):
            (h0, _, c0), (h1, _, c1), (h2, _, c2) = k[3 * t:3 * t + 3]
            v = (float(h0) - 90.0) / res
            assert v - math.floor(v) == 0.5 and h1 < h0 < h2                 # a tie of round(), and a float either side
            assert c1 == c2 + 1 and c0 == c1                                 # two columns; the tie rounds away from zero
            ties += 1
        print(f"ri_boundaries_{H}: {ties} ties, neighbours in two columns each")
        assert ties == 12 and len(refs[c["id"]]["cloud"]) >= 20
    c = cs["ri_wrap"]
    k = cols(c)
    wrapped = [r for r in k if r[1] >= c["H"]]
    print(f"ri_wrap: {len(wrapped)} of {len(k)} points through col -= H, {sum(r[2] == 0 for r in wrapped)} into column 0")
    assert len(wrapped) > 100 and len(k) - len(wrapped) > 100 and any(r[1] == c["H"] and r[2] == 0 for r in wrapped)
    assert 0 in refs["ri_wrap"]["col"]
    assert set(refs["ri_H_1"]["col"].tolist()) == {0} and len(refs["ri_H_1"]["cloud"]) == 4
    assert {r[1] for r in cols(cs["ri_H_1"])} == {0, 1}
    assert cs["ri_H_32767"]["H"] == 32767 and refs["ri_H_32767"]["col"].max() > 32700 and len(refs["ri_H_32767"]["cloud"]) > 12000
    assert cs["ri_n_scan_1"]["cfg"]["N_SCAN"] == 1 and len(refs["ri_n_scan_1"]["cloud"]) == 1800
    c = cs["ri_n_scan_1024"]
    occupied = (refs[c["id"]]["end_ring"] - refs[c["id"]]["start_ring"] > -10).sum()
    assert c["cfg"]["N_SCAN"] == 1024 and c["H"] % 2 == 1 and occupied == 1024 and len(refs[c["id"]]["cloud"]) > 25000
    assert len(refs["ri_cells_4096"]["cloud"]) == 4096 == cs["ri_cells_4096"]["cfg"]["N_SCAN"] * cs["ri_cells_4096"]["H"]
    assert len(refs["ri_cells_4097"]["cloud"]) == 4097 == cs["ri_cells_4097"]["cfg"]["N_SCAN"] * cs["ri_cells_4097"]["H"]
    c = cs["ri_range_gates"]
    r = np.array([D.range_f32(*p) for p in zip(c["x"], c["y"], c["z"])])
    keep = c["expect"]["keep"]
    on = np.isin(np.arange(len(r)), keep)
    print(f"ri_range_gates: ranges {r.tolist()}, kept {keep.tolist()}")
    assert set(r[on].tolist()) == {5.0, 50.0} and c["minRange"] == 5.0 and c["cfg"]["lidarMaxRange"] == 50.0
    assert set(r[~on].tolist()) == {float(D.step(5.0, -1)), float(D.step(50.0, 1))}
    assert np.array_equal(np.sort(refs[c["id"]]["range"]), np.sort(r[on]))
    c = cs["ri_dense_cell"]
    dense = c["expect"]["dense"]
    k = {D.column_of(c["x"][i], c["y"][i], c["H"])[2] for i in dense}
    assert len(k) == 1 and len(dense) == 5000 and (c["ring"][dense] == 7).all()
    col = k.pop()
    ref = refs[c["id"]]
    start = ref["start_ring"][7] - 4
    row = start + int(np.nonzero(ref["col"][start:ref["end_ring"][7] + 6] == col)[0][0])
    rivals = [i for i in np.nonzero(c["ring"] == 7)[0] if D.column_of(c["x"][i], c["y"][i], c["H"])[2] == col]
    print(f"ri_dense_cell: column {col} of ring 7 holds {len(rivals)} points, the first is input {rivals[0]}")
    assert ref["cloud"][row, 3] == c["intensity"][rivals[0]] and ref["range"][row] == D.range_f32(*(c[a][rivals[0]] for a in "xyz"))
    assert rivals[0] >= 50 and len(rivals) >= 5000


def test_nan_in_the_range_image_has_no_column(oracle):
    c, = D.cases("nan_ri")
    ref = D.reference(oracle, c)
    nans = int(np.isnan(ref["cloud"]).sum() + np.isnan(ref["range"]).sum())
    print(f"{c['id']}: {len(c['x'])} points -> {len(ref['cloud'])} cells, {nans} NaN outputs")
    # no point has column 0, the cell (int)NaN = 0 would send a NaN azimuth to; all four rings hold dropped points
    assert 0 not in {D.column_of(x, y, c["H"])[2] for x, y in zip(c["x"], c["y"])} and 0 not in ref["col"]
    assert set(c["ring"][c["expect"]["dropped"]].tolist()) == {0, 1, 2, 3}
    assert all(D.column_of(c["x"][i], c["y"][i], c["H"])[2] == -1 for i in c["expect"]["dropped"])
    assert len(ref["cloud"]) == c["expect"]["n_cells"] and nans == c["expect"]["nans"] and 0 < nans < ref["cloud"].size
    assert int(np.isnan(ref["range"]).sum()) == 7 and np.isnan(c["time"]).sum() == 7


def test_fuzz_trials_mix_the_rules(oracle):
    ns, tables, kept, cells = set(), set(), 0, 0
    for t in range(20):
        c, what = D.fuzz_trial(t)
        ns.add(len(c["x"])); tables.add(c["imu"][0] + 1)
        ref, ri = D.run_oracle(oracle, c), D.run_oracle(oracle, c, "ri")
        assert _finite(ref) and _finite(ri), what
        kept += len(ref["cloud"]); cells += len(ri["cloud"])
    print(f"fuzz: n {sorted(ns)}, tables {sorted(tables)}, {kept} survivors, {cells} cells")
    assert ns == set(D.FUZZ_N) and tables == set(D.FUZZ_TABLE) and kept > 5000 and cells > 2000


PROOF_OF = {"time": test_time_cases_take_every_branch, "first": test_first_survivor_sits_where_the_case_says,
            "compact": test_compaction_sizes_and_workgroup_patterns, "keep": test_keep_thresholds_are_strict,
            "nan": test_nan_cases_hold_the_predicted_nans, "pc2": test_layout_cases_narrow_and_convert,
            "ri": test_range_image_cases_reach_their_cells, "nan_ri": test_nan_in_the_range_image_has_no_column}


def test_every_case_family_has_its_proof():
    """Each proof above walks every case of its family (it looks each one up by id, or loops over all of them)."""
    assert set(PROOF_OF) == set(D.CASES)
    ids = [c["id"] for c in D.all_cases()]
    assert len(ids) == len(set(ids)) >= 45
    assert all(c["nan"] == c["id"].startswith("nan_") for c in D.all_cases())
    assert all(len(c["x"]) <= 70000 for c in D.all_cases())


# ---------------------------------------------------------------- the literal transcription
def _sin(x):
    return F32(math.sin(float(x)))


def _cos(x):
    return F32(math.cos(float(x)))


def _py_find_rotation(point_time, T, RX, RY, RZ, cur):
    """findRotation, IP:502-527: fp64 throughout, stored to float."""
    front = 0
    while front < cur:
        if point_time < T[front]:
            break
        front += 1
    if point_time > T[front] or front == 0:
        return F32(RX[front]), F32(RY[front]), F32(RZ[front])
    back = front - 1
    ratio_front = (point_time - T[back]) / (T[front] - T[back])
    ratio_back = (T[front] - point_time) / (T[front] - T[back])
    return (F32(RX[front] * ratio_front + RX[back] * ratio_back), F32(RY[front] * ratio_front + RY[back] * ratio_back),
            F32(RZ[front] * ratio_front + RZ[back] * ratio_back))


def _py_rotation(roll, pitch, yaw):
    """The linear part of pcl::getTransformation(0, 0, 0, roll, pitch, yaw), IP:560/565."""
    A, B, C, Dd, E, Fs = _cos(yaw), _sin(yaw), _cos(pitch), _sin(pitch), _cos(roll), _sin(roll)
    DE, DF = Dd * E, Dd * Fs
    return [A * C, A * DF - B * E, B * Fs + A * DE,
            B * C, A * E + B * DF, B * DE - A * Fs,
            -Dd, C * Fs, C * E]


def _py_inverse(m):
    """Eigen's 3 x 3 inverse by cofactors, `.inverse()` IP:560."""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1]
    c0, c1, c2 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = c0 * m[0] + c1 * m[3] + c2 * m[6]
    inv = F32(1.0) / det
    return [c0 * inv, c1 * inv, c2 * inv, cof(0, 1) * inv, cof(1, 1) * inv, cof(2, 1) * inv,
            cof(0, 2) * inv, cof(1, 2) * inv, cof(2, 2) * inv]


class _Deskew:
    """deskewPoint, IP:545-575, with its firstPointFlag / transStartInverse state."""

    def __init__(self, case):
        self.cur, self.T, self.RX, self.RY, self.RZ = (case["imu"][0],) + tuple(np.asarray(a, np.float64) for a in case["imu"][1:])
        self.t0, self.first, self.start_inv = np.float64(case["t0"]), True, None       # (numpy scalars: 0 / 0 is NaN, not an exception)
        self.on = not (case["cfg"]["deskew_flag"] == -1 or self.cur <= 0)

    def __call__(self, x, y, z, rel):
        if not self.on:
            return x, y, z
        point_time = self.t0 + np.float64(rel)
        L = _py_rotation(*_py_find_rotation(point_time, self.T, self.RX, self.RY, self.RZ, self.cur))
        if self.first:
            self.start_inv, self.first = _py_inverse(L), False
        S = self.start_inv
        Bt = [S[r * 3 + 0] * L[0 * 3 + c] + S[r * 3 + 1] * L[1 * 3 + c] + S[r * 3 + 2] * L[2 * 3 + c] for r in range(3) for c in range(3)]
        zero = F32(0.0)
        return (Bt[0] * x + Bt[1] * y + Bt[2] * z + zero, Bt[3] * x + Bt[4] * y + Bt[5] * z + zero, Bt[6] * x + Bt[7] * y + Bt[8] * z + zero)


def _py_project(case):
    """projectPointCloud, IP:577-615."""
    g = dict(D.OPEN, **case["cfg"])
    deskew = _Deskew(case)
    out, keep = [], []
    with np.errstate(all="ignore"):
        for i in range(len(case["x"])):
            x, y, z, inten = case["x"][i], case["y"][i], case["z"][i], case["intensity"][i]
            rng = np.sqrt(x * x + y * y + z * z)
            if ((y < F32(g["lidarMinFront"]) and -F32(g["lidarMinBack"]) < y and x < F32(g["lidarMinLeft"]) and -F32(g["lidarMinRight"]) < x)
                    or rng > F32(g["lidarMaxRange"]) or inten > F32(g["lidarMaxIntensity"])):
                continue
            row = int(case["ring"][i])
            if row < 0 or row >= g["N_SCAN"]:
                continue
            if row % g["downsampleRate"] != 0:
                continue
            if i % g["point_filter_num"] != 0:
                continue
            out.append(deskew(x, y, z, case["time"][i]) + (inten,))
            keep.append(i)
    return np.array(out, F32).reshape(-1, 4), np.array(keep, np.int32)


def _py_range_image(case):
    """projectPointCloud + cloudExtraction of upstream LIO-SAM on deskewPoint (the semantics oracle/lio_oracle.c states)."""
    g, H, NS = dict(D.OPEN, **case["cfg"]), case["H"], case["cfg"]["N_SCAN"]
    deskew = _Deskew(case)
    cells = {}
    with np.errstate(all="ignore"):
        for i in range(len(case["x"])):
            x, y, z = case["x"][i], case["y"][i], case["z"][i]
            rng = np.sqrt(x * x + y * y + z * z)
            if rng < F32(case["minRange"]) or rng > F32(g["lidarMaxRange"]):
                continue
            row = int(case["ring"][i])
            if row < 0 or row >= NS or row % g["downsampleRate"] != 0:
                continue
            col = D.column_of(x, y, H)[2]
            if col < 0 or (row, col) in cells:
                continue
            cells[(row, col)] = (deskew(x, y, z, case["time"][i]) + (case["intensity"][i],), rng)
    cloud, cols, ranges, start, end = [], [], [], [], []
    for row in range(NS):
        start.append(len(cloud) - 1 + 5)
        for col in sorted(c for r, c in cells if r == row):
            cloud.append(cells[(row, col)][0]); cols.append(col); ranges.append(cells[(row, col)][1])
        end.append(len(cloud) - 1 - 5)
    return {"cloud": np.array(cloud, F32).reshape(-1, 4), "col": np.array(cols, np.int32), "range": np.array(ranges, F32),
            "start_ring": np.array(start, np.int32), "end_ring": np.array(end, np.int32)}


SMALL = [c for c in D.all_cases() if len(c["x"]) <= 400]


def test_small_set_is_large_enough():
    kinds = [c["kind"] for c in SMALL]
    assert kinds.count("deskew") >= 5 and kinds.count("ri") >= 5
    assert {"time_table2", "time_t0_1.7e9", "keep_box", "nan_stamps_equal", "ri_axes", "ri_boundaries_720", "ri_wrap"} <= {c["id"] for c in SMALL}


@pytest.mark.parametrize("case", SMALL, ids=[c["id"] for c in SMALL])
def test_oracle_equals_the_literal_transcription(oracle, case):
    ref = D.reference(oracle, case)
    if case["kind"] == "ri":
        mine = _py_range_image(case)
    else:
        cloud, keep = _py_project(case)
        assert np.array_equal(keep, ref["keep"])
        mine = {"cloud": cloud}
    rep = D.diff_report(mine, ref, case["nan"])
    assert not rep, f"{case['id']}\n{rep}"
