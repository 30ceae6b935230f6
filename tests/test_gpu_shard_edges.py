"""Map sharding where the one-GPU rehearsals had never been: slab axes 1 and 2, the partition itself (who processed which
scan point, whole workgroups and single points), owners that change between Gauss-Newton iterations under the search-
bound cache, and slab plans that degenerate (eight devices, coinciding bounds, fewer cells than devices, maps of 0, 1
and 4 points, non-finite map points, a scan far outside the map).  The reference everywhere is the single-device handle
on the same inputs, which the rest of the suite pins to the oracle; one query per frame is checked against the oracle
here as well.  Builders and the frames: tests/shard_cases.py (P2 is tilted, see there).  The test box has one GPU: it is
listed several times, or holds one handle per rank."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shard_cases as S                                   # noqa: E402

pytestmark = pytest.mark.gpu

FRAME_NAMES = ["identity", "P1", "P2"]
SHIFTS = (0.0, 0.5, -0.5, 1.5, -1.5)                      # cells along the slab axis


@pytest.fixture(scope="module")
def frames(small_case):
    return {name: S.framed(small_case, name) for name in FRAME_NAMES}


def _register_equal(one, many, scan, pose, record=True):
    p1, r1, rc1 = one.scan2MapOptimization(scan, pose)
    p2, r2, rc2 = many.scan2MapOptimization(scan, pose)
    assert (rc1, r1.status, r1.iters, r1.converged, r1.is_degenerate) == (rc2, r2.status, r2.iters, r2.converged, r2.is_degenerate)
    assert list(r1.n_corr_iter) == list(r2.n_corr_iter)
    if record:
        S.assert_same_record(many.get_correspondences(0), one.get_correspondences(0))
    assert np.abs(p1[3:] - p2[3:]).max() <= S.TOL_T and np.abs(p1[:3] - p2[:3]).max() <= S.TOL_R
    return p1, r1


# ------------------------------------------------------------------ A: every axis, in the library
@pytest.mark.parametrize("n_dev", [2, 3])
@pytest.mark.parametrize("frame", FRAME_NAMES)
def test_every_slab_axis_in_the_library(pkg, oracle, frames, frame, n_dev):
    case = frames[frame]
    one = pkg.ScanToMap(record_corr_iter=0)
    one.set_map(case["map"])
    many = pkg.ScanToMap(record_corr_iter=0, n_devices=n_dev, device_ids=[0] * n_dev)
    many.set_map(case["map"])
    for k, q in enumerate(case["queries"]):
        p1, r1 = _register_equal(one, many, q["scan"], q["pose_init"])
        assert r1.converged == 1, (frame, k)              # the reference converges in this frame
        if k == 0:
            po, ro, _, _ = oracle.scan2map(oracle.default_config(knn_mode=1, n_threads=8), q["scan"], case["map"], q["pose_init"])
            assert ro.iters == r1.iters
            assert np.abs(p1[3:] - po[3:]).max() <= S.TOL_T and np.abs(p1[:3] - po[:3]).max() <= S.TOL_R
    one.close(); many.close()


@pytest.mark.parametrize("max_sq_dist", [0.49, 4.0])
def test_axis_1_with_another_gate(pkg, frames, max_sq_dist):
    """The plan's cell and the owner test's cell follow the gate together (tests/test_gpu_multidevice.py checks it on axis 0)."""
    case = frames["P1"]
    assert S.lib_plan(case["map"], 2, max_sq_dist)["axis"] == 1
    one = pkg.ScanToMap(record_corr_iter=0, max_sq_dist=max_sq_dist)
    one.set_map(case["map"])
    many = pkg.ScanToMap(record_corr_iter=0, max_sq_dist=max_sq_dist, n_devices=2, device_ids=[0, 0])
    many.set_map(case["map"])
    for q in case["queries"]:
        _, r1 = _register_equal(one, many, q["scan"], q["pose_init"])
        assert r1.converged == 1
    one.close(); many.close()


# ------------------------------------------------------------------ B: the partition, observed
def _shifted_batch(case, plan):
    scans, poses = [], []
    for q in case["queries"]:
        for d in SHIFTS:
            scans.append(q["scan"])
            poses.append(S.shift_along_axis(q["pose_init"], plan, d))
    return scans, np.stack(poses)


@pytest.fixture(scope="module")
def unsharded_pass(pkg, frames):
    """One pass of the shifted batch on the unsharded handle, per frame: (sums [scan, 32], [record of every scan])."""
    out = {}
    for name, case in frames.items():
        scans, poses = _shifted_batch(case, S.lib_plan(case["map"], 2))
        one = pkg.ScanToMap(pipeline=1, max_iters=1, record_corr_iter=0)
        one.set_map(case["map"])
        kept, _, _ = S.drive([one], scans, poses, 1)
        out[name] = (kept[0][0], [one.get_correspondences(s) for s in range(len(scans))])
        one.close()
    return out


def _assert_sums_within_reordering(parts, ref):
    """sum over the ranks == the unsharded sums: N_c exactly, the rest to the bound of another summation order."""
    tot = parts[0].copy()
    for p in parts[1:]:
        tot = tot + p
    np.testing.assert_array_equal(tot[:, S.N_C], ref[:, S.N_C])
    u = 2.0 ** -52
    for s in range(len(ref)):
        n_c = ref[s, S.N_C]
        diag = ref[s, list(S.DIAG)]
        for slot, (a, b) in enumerate(S.PAIRS):
            err = abs(tot[s, slot] - ref[s, slot])
            assert err <= n_c * u * np.sqrt(diag[a] * diag[b]), (s, slot, err)
        for a in range(6):
            err = abs(tot[s, 21 + a] - ref[s, 21 + a])
            assert err <= n_c * u * np.sqrt(diag[a] * n_c), (s, a, err)


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("halo", [1, 16])
@pytest.mark.parametrize("frame", FRAME_NAMES)
def test_every_scan_point_has_exactly_one_rank(pkg, frames, unsharded_pass, frame, halo, world):
    case = frames[frame]
    plan = S.sensor_bound_plan(case, 0) if world == 2 else S.lib_plan(case["map"], 8)
    assert plan["axis"] == S.FRAME_AXIS[frame]
    scans, poses = _shifted_batch(case, plan)
    ref_sums, ref_rec = unsharded_pass[frame]
    hs, idxs = S.rank_handles(pkg, case["map"], plan, halo, max_iters=1, record_corr_iter=0)
    kept, _, _ = S.drive(hs, scans, poses, 1)
    assert (kept[0][:, :, S.N_C].sum(1) > 0).sum() >= 2                   # a real split: two ranks at least have work
    _assert_sums_within_reordering(list(kept[0]), ref_sums)
    for s in range(len(scans)):
        S.assert_same_record(S.union_records(S.rank_records(hs, idxs, s)), ref_rec[s])
    for h in hs:
        h.close()


@pytest.mark.parametrize("halo", [1, 16])
def test_a_second_run_on_the_same_upload_records_afresh(pkg, frames, unsharded_pass, halo):
    """The record is cleared when a batch is uploaded.  A second run on the SAME upload from other guesses moves points to
    other ranks; the rank that processed them in the first run must not go on showing its old record."""
    case = frames["P1"]
    plan = S.sensor_bound_plan(case, 0)
    scans, poses = _shifted_batch(case, plan)
    ref_sums, ref_rec = unsharded_pass["P1"]
    first = poses.reshape(3, len(SHIFTS), 6)[:, ::-1].reshape(-1, 6)      # every scan starts from another of its guesses
    hs, idxs = S.rank_handles(pkg, case["map"], plan, halo, max_iters=1, record_corr_iter=0)
    S.drive(hs, scans, np.ascontiguousarray(first), 1)
    kept, _, _ = S.drive(hs, scans, poses, 1, upload=False)
    _assert_sums_within_reordering(list(kept[0]), ref_sums)
    for s in range(len(scans)):
        S.assert_same_record(S.union_records(S.rank_records(hs, idxs, s)), ref_rec[s])
    for h in hs:
        h.close()
    # the same in the library
    one, many = _pair(pkg, 2, max_iters=1)
    one.set_map(case["map"]); many.set_map(case["map"])
    for h in (one, many):
        h.batch_upload(scans); h.batch_set_poses(np.ascontiguousarray(first)); h.batch_run(); h.batch_results()
        h.batch_set_poses(poses); h.batch_run(); h.batch_results()
    for s in range(len(scans)):
        S.assert_same_record(many.get_correspondences(s), one.get_correspondences(s))
        S.assert_same_record(one.get_correspondences(s), ref_rec[s])
    one.close(); many.close()


def _one_pass(pkg, case, plan, halo, scan, pose):
    hs, idxs = S.rank_handles(pkg, case["map"], plan, halo, max_iters=1, record_corr_iter=0)
    kept, _, _ = S.drive(hs, [scan], pose[None], 1)
    recs = S.rank_records(hs, idxs, 0)
    for h in hs:
        h.close()
    return kept[0][:, 0, S.N_C], recs


def _unsharded_record(pkg, case, scan, pose):
    one = pkg.ScanToMap(pipeline=1, max_iters=1, record_corr_iter=0)
    one.set_map(case["map"])
    S.drive([one], [scan], pose[None], 1)
    rec = one.get_correspondences(0)
    one.close()
    return rec


@pytest.mark.parametrize("frame", FRAME_NAMES)
def test_whole_workgroup_ownership_is_taken(pkg, frames, frame):
    case = frames[frame]
    q = case["queries"][0]
    scan = S.one_workgroup_scan(q["scan"], 6.0)
    base = S.lib_plan(case["map"], 2)
    c_lo, c_hi = S.workgroup_cells(scan, q["pose_init"], base)
    bound = ((c_lo + c_hi) >> 1) + 2                                      # the middle cell (and its neighbours) on rank 0's side
    plan = S.with_bounds(base, [0, bound, base["dims"][base["axis"]]])
    assert c_lo < bound <= c_hi                                           # the box straddles the bound
    assert S.whole_owner(plan, 16, c_lo, c_hi) == 0 and S.whole_owner(plan, 1, c_lo, c_hi) is None
    ref = _unsharded_record(pkg, case, scan, q["pose_init"])
    n16, rec16 = _one_pass(pkg, case, plan, 16, scan, q["pose_init"])
    assert n16[0] > 0 and n16[1] == 0 and not rec16[1][0].any() and not rec16[1][3].any()
    n1, rec1 = _one_pass(pkg, case, plan, 1, scan, q["pose_init"])
    assert n1[0] > 0 and n1[1] > 0
    S.assert_same_record(S.union_records(rec16), ref)
    S.assert_same_record(S.union_records(rec1), ref)
    assert n16.sum() == n1.sum() == ref[0].sum()


@pytest.mark.parametrize("frame", FRAME_NAMES)
def test_per_point_ownership_is_taken(pkg, frames, frame):
    """A workgroup longer than any rank's slab + halos.  The eight slabs are equally wide here: the count-balanced plan ends
    in one slab of 64 cells (the thin far end of the map), which with its halos is longer than any 45 m box."""
    case = frames[frame]
    q = case["queries"][0]
    scan = S.one_workgroup_scan(q["scan"], 45.0)
    plan = S.equal_slabs_plan(case["map"], 8)
    c_lo, c_hi = S.workgroup_cells(scan, q["pose_init"], plan)
    assert c_hi - c_lo + 1 > np.diff(plan["bounds"]).max() + 2 * 16
    assert S.whole_owner(plan, 16, c_lo, c_hi) is None
    ref = _unsharded_record(pkg, case, scan, q["pose_init"])
    n16, rec16 = _one_pass(pkg, case, plan, 16, scan, q["pose_init"])
    assert (n16 > 0).sum() >= 2
    S.assert_same_record(S.union_records(rec16), ref)
    assert n16.sum() == ref[0].sum()


# ------------------------------------------------------------------ C: owners that move between iterations
def _cached_and_uncached(pkg, case, plan, halo, scan, guess):
    """The same layout with nn_cache 0 and 1 -> [(kept, poses, results, records of every rank)]."""
    outs = []
    for nn_cache in (0, 1):
        hs, idxs = S.rank_handles(pkg, case["map"], plan, halo, nn_cache=nn_cache, force_all_iters=1, max_iters=8, record_corr_iter=3)
        kept, poses, res = S.drive(hs, [scan], guess[None], 8)
        assert len(kept) == 8
        outs.append((kept, poses, res, S.rank_records(hs, idxs, 0)))
        for h in hs:
            h.close()
    return outs


def _assert_byte_identical(a, b):
    (kept_a, poses_a, res_a, rec_a), (kept_b, poses_b, res_b, rec_b) = a, b
    assert poses_a.tobytes() == poses_b.tobytes()
    for x, y in zip(res_a, res_b):
        assert bytes(x) == bytes(y)                                       # pose_iter, n_corr_iter, AtA, AtB, matP, every flag
    for x, y in zip(kept_a, kept_b):
        assert x.tobytes() == y.tobytes()                                 # every partial of every rank and iteration
    for (fa, ca, na, _), (fb, cb, nb, _) in zip(rec_a, rec_b):
        assert fa.tobytes() == fb.tobytes() and ca.tobytes() == cb.tobytes() and na.tobytes() == nb.tobytes()


@pytest.mark.parametrize("frame", ["identity", "P1"])
def test_a_workgroup_that_changes_hands_keeps_exact_neighbours(pkg, frames, frame):
    """k_shard_cull's modes 2 <-> 1: the whole workgroup is rank 1's at the guess and rank 0's from then on."""
    case = frames[frame]
    scan, guess, plan = S.moving_workgroup_case(case)
    off, on = _cached_and_uncached(pkg, case, plan, 16, scan, guess)
    n_c = np.stack([k[:, 0, S.N_C] for k in on[0]])                       # [iteration, rank]
    first = [it for it in range(8) if n_c[it, 0] == 0 < n_c[it, 1]]
    later = [it for it in range(8) if n_c[it, 0] > 0 == n_c[it, 1]]
    assert first and later and later[-1] > first[0], n_c.tolist()         # ownership really moved
    assert later[-1] >= 3 and on[3][0][0].any() and not on[3][1][0].any()   # and the record of iteration 3 is rank 0's
    _assert_byte_identical(off, on)


@pytest.mark.parametrize("frame", ["identity", "P1"])
def test_points_that_change_hands_keep_exact_neighbours(pkg, oracle, frames, frame):
    """Per-point ownership (halo 1) with the bound through the sensor while the registration walks 1.2 cells back."""
    case = frames[frame]
    scan, guess, plan = S.stable_scan_case(oracle, case)
    off, on = _cached_and_uncached(pkg, case, plan, 1, scan, guess)
    n_c = np.stack([k[:, 0, S.N_C] for k in on[0]])
    assert S.moved_per_point(n_c[:, 0], n_c[:, 1]), n_c.tolist()          # ownership really moved
    _assert_byte_identical(off, on)


@pytest.mark.parametrize("n_dev", [2, 5])
def test_search_bound_cache_is_exact_in_the_library(pkg, small_case, n_dev):
    qs = small_case["queries"]
    scans = [q["scan"] for q in qs]
    poses0 = np.stack([q["pose_init"] for q in qs])
    outs = []
    for nn_cache in (0, 1):
        m = pkg.ScanToMap(n_devices=n_dev, device_ids=[0] * n_dev, nn_cache=nn_cache)
        m.set_map(small_case["map"])
        m.batch_upload(scans); m.batch_set_poses(poses0); m.batch_run()
        p, r = m.batch_results()
        outs.append((p.tobytes(), bytes(r)))
        assert all(x.converged == 1 for x in r)
        m.close()
    assert outs[0] == outs[1]


# ------------------------------------------------------------------ D: degenerate plans, library vs single handle
def _pair(pkg, n_dev, **cfg):
    return pkg.ScanToMap(record_corr_iter=0, **cfg), pkg.ScanToMap(record_corr_iter=0, n_devices=n_dev, device_ids=[0] * n_dev, **cfg)


def test_eight_devices(pkg, small_case):
    one, many = _pair(pkg, 8)
    one.set_map(small_case["map"]); many.set_map(small_case["map"])
    qs = small_case["queries"]
    _, res = S.assert_equal_runs(one, many, [q["scan"] for q in qs], np.stack([q["pose_init"] for q in qs]))
    assert all(r.converged == 1 for r in res)
    one.close(); many.close()


def test_coinciding_bounds(pkg, small_case):
    big = S.skewed_map(small_case["map"])
    b = S.lib_plan(big, 4)["bounds"]
    assert (np.diff(b) == 0).any(), b                                     # at least one empty slab [b, b)
    one, many = _pair(pkg, 4)
    one.set_map(big); many.set_map(big)
    qs = small_case["queries"]
    _, res = S.assert_equal_runs(one, many, [q["scan"] for q in qs], np.stack([q["pose_init"] for q in qs]))
    assert all(r.converged == 1 for r in res)
    one.close(); many.close()


def test_fewer_cells_than_devices(pkg):
    cube = S.cube_case()
    plan = S.lib_plan(cube["map"], 5)
    assert plan["dims"][plan["axis"]] < 5
    one, many = _pair(pkg, 5)
    one.set_map(cube["map"]); many.set_map(cube["map"])
    _, r1 = _register_equal(one, many, cube["scan"], cube["pose_init"])
    assert r1.converged == 1 and r1.status == 0
    one.close(); many.close()


def _outcome(pkg, h, map_xyz, scan, pose):
    """What a handle does with a map: the error's name, or (rc, status, iters, n_corr_iter)."""
    try:
        h.set_map(map_xyz)
        _, res, rc = h.scan2MapOptimization(scan, pose)
    except pkg.LioError as e:
        return ("error", str(e).split(": ")[1])
    return (rc, res.status, res.iters, res.converged, list(res.n_corr_iter))


@pytest.mark.parametrize("n_map", [0, 1, 4])
def test_tiny_maps(pkg, small_case, n_map):
    q = small_case["queries"][0]
    one, many = _pair(pkg, 3)
    tiny = np.ascontiguousarray(small_case["map"][:n_map]).reshape(n_map, 3)
    assert _outcome(pkg, one, tiny, q["scan"], q["pose_init"]) == _outcome(pkg, many, tiny, q["scan"], q["pose_init"])
    one.set_map(small_case["map"]); many.set_map(small_case["map"])       # a good map afterwards registers as usual
    _, r1 = _register_equal(one, many, q["scan"], q["pose_init"])
    assert r1.converged == 1
    one.close(); many.close()


def test_nonfinite_map_rows(pkg, small_case):
    rng = np.random.default_rng(9)
    bad = small_case["map"].copy()
    rows = rng.choice(len(bad), len(bad) // 100, replace=False)
    bad[rows[0::3], 0] = np.nan
    bad[rows[1::3], 1] = np.inf
    bad[rows[2::3], 2] = -np.inf
    one, many = _pair(pkg, 3)
    one.set_map(bad); many.set_map(bad)
    for q in small_case["queries"]:
        _register_equal(one, many, q["scan"], q["pose_init"])             # (nn_idx5 in the caller's numbering, bit for bit)
        nn = many.get_correspondences(0)[2]
        assert (nn >= 0).any() and not np.isin(nn[nn >= 0], rows).any()
    one.close(); many.close()


def test_a_scan_far_outside_the_map(pkg, small_case):
    qs = small_case["queries"]
    plan = S.lib_plan(small_case["map"], 3)
    far = qs[0]["pose_init"].copy()
    far[3 + plan["axis"]] = small_case["map"][:, plan["axis"]].max() + 500.0
    scans = [q["scan"] for q in qs]
    poses0 = np.stack([q["pose_init"] for q in qs])
    one, many = _pair(pkg, 3)
    one.set_map(small_case["map"]); many.set_map(small_case["map"])
    p3, r3 = S.assert_equal_runs(one, many, scans, poses0)
    p4, r4 = S.assert_equal_runs(one, many, scans + [qs[0]["scan"]], np.concatenate([poses0, far[None]]))
    assert r4[3].status != 0 and r4[3].n_corr_last == 0                   # nothing to associate out there
    for a, b, pa, pb in zip(r4[:3], r3, p4[:3], p3):                      # the others are unaffected
        assert (a.status, a.iters, a.converged, list(a.n_corr_iter)) == (b.status, b.iters, b.converged, list(b.n_corr_iter))
        assert np.abs(pa[3:] - pb[3:]).max() <= S.TOL_T and np.abs(pa[:3] - pb[:3]).max() <= S.TOL_R
    one.close(); many.close()
