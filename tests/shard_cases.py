"""Builders shared by tests/test_gpu_shard_edges.py and tests/test_shard_plan_cpu.py: the small_case workload in world
frames whose street runs along y and along z, per-rank handles on one GPU with a host-driven Gauss-Newton loop that keeps
every rank's partial sums, scans that are exactly one association workgroup, and the maps of the degenerate slab plans.
Everything is made from small_case with numpy; nothing here casts a ray.

The frames.  P1 = (x, y, z) -> (z, x, y) puts the street along y.  P1 @ P1 = (x, y, z) -> (y, z, x) would put it along z
EXACTLY, and with it the vehicle's forward axis: the re-derived pitch is -90 deg +- the vehicle's yaw, the Euler angles
the registration iterates in are singular there, and the reference itself stops converging (2 of the 3 queries of
small_case run 30 iterations and end degenerate).  P2 is therefore P1 @ P1 followed by a 30 deg turn about the new x
axis: the street climbs at 60 deg, z is still the longest grid axis by far (slab axis 2), pitch is -60 deg, roll ~ 0 and
yaw ~ -90 deg, all far from a wrap.  P2 is no permutation, so map' is rounded to fp32 once, here; every handle and the
oracle then see that same map'."""
import importlib
import math

import numpy as np

BLOCK = 256            # LIO_BLOCK: points per association workgroup
SUMS = 32              # LIO_SUMS: 21 upper JtJ (row-major), 6 Jtr, N_c, pad
N_C = 27
DIAG = (0, 6, 11, 15, 18, 20)                                    # slots of JtJ(a, a) among the 21
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]          # slot -> (a, b)
LIB_HALO = 16          # LIO_MULTI_HALO
TOL_T, TOL_R = 1e-5, 1e-6                                        # tests/test_gpu_multidevice.py

P1 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
_C30, _S30 = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
P2 = np.array([[1.0, 0.0, 0.0], [0.0, _C30, -_S30], [0.0, _S30, _C30]]) @ P1 @ P1
FRAMES = {"identity": np.eye(3), "P1": P1, "P2": P2}
FRAME_AXIS = {"identity": 0, "P1": 1, "P2": 2}


def _mg():
    return importlib.import_module("lio-slam_amd.multigpu")


def _synth():
    return importlib.import_module("lio-slam_amd.synth")


def reframe(case, P):
    """The same workload in the world frame x' = P x: map' = map @ P.T, every pose P * pose, scans (lidar frame) as they are."""
    synth = _synth()
    P = np.asarray(P, np.float64)
    assert abs(np.linalg.det(P) - 1.0) < 1e-12 and np.allclose(P @ P.T, np.eye(3), atol=1e-12)
    Pm = np.eye(4)
    Pm[:3, :3] = P

    def move(pose):
        return synth.matrix_to_pose(Pm @ synth.pose_matrix(np.asarray(pose, np.float64))).astype(np.float32)

    queries = [{"scan": q["scan"], "pose_init": move(q["pose_init"]), "pose_true": move(q["pose_true"])} for q in case["queries"]]
    return {"map": np.ascontiguousarray((case["map"].astype(np.float64) @ P.T).astype(np.float32)), "queries": queries}


def framed(case, frame):
    """reframe() into FRAMES[frame], with the guard that the slab plan really takes the axis the frame is named for."""
    out = reframe(case, FRAMES[frame])
    assert _mg().plan_shards(out["map"], 2)["axis"] == FRAME_AXIS[frame]
    return out


def lib_plan(map_xyz, world, max_sq_dist=1.0):
    """The plan lio_multi_set_map makes for a finite map (same cell as the device-side owner test)."""
    mg = _mg()
    return mg.plan_shards(map_xyz, world, cell=mg.default_cell(max_sq_dist))


def with_bounds(plan, bounds):
    out = dict(plan)
    out["bounds"] = np.asarray(bounds, np.int64)
    assert out["bounds"][0] == 0 and out["bounds"][-1] == plan["dims"][plan["axis"]] and (np.diff(out["bounds"]) >= 0).all()
    return out


def axis_cell(plan, v):
    """Grid cell along the slab axis of coordinate(s) v, clamped to the grid as every owner test clamps it."""
    mg, a = _mg(), plan["axis"]
    return np.clip(mg.cell_coord(v, plan["origin"][a], plan["inv_cell"], plan["dims"][a]), 0, plan["dims"][a] - 1)


def shift_along_axis(pose, plan, cells):
    out = np.array(pose, np.float32).copy()
    out[3 + plan["axis"]] += np.float32(cells) * np.float32(plan["cell"])
    return out


def rank_handles(pkg, map_xyz, plan, halo, **cfg):
    """One launch-loop handle per rank of `plan` on the one GPU, each holding its slab + `halo` cells.  -> (handles, idx):
    idx[r] maps rank r's map numbering back to the caller's."""
    mg = _mg()
    hs, idxs = [], []
    for r in range(len(plan["bounds"]) - 1):
        idx = mg.shard_points(map_xyz, plan, r, halo)
        h = pkg.ScanToMap(pipeline=1, **cfg)
        h.set_map(np.ascontiguousarray(map_xyz[idx]))
        h.set_global_grid([float(v) for v in plan["origin"]], [int(v) for v in plan["dims"]])
        h.set_shard_plan(plan["axis"], r, [int(v) for v in plan["bounds"]], halo)
        hs.append(h)
        idxs.append(idx)
    return hs, idxs


def drive(hs, scans, poses0, max_iters, upload=True):
    """batch_begin, then per Gauss-Newton iteration: every handle's partial sums, added in rank order, applied on every
    handle.  -> (kept, poses, results): kept[it] is the fp64 array [rank, scan, 32] of that iteration's partials; poses
    and results are rank 0's (every rank solves the same sums)."""
    import torch
    n = len(scans)
    for h in hs:
        if upload:
            h.batch_upload(scans)
        h.batch_set_poses(poses0)
        h.batch_begin()
    part = [torch.zeros((n, SUMS), dtype=torch.float64, device="cuda") for _ in hs]
    kept, totals = [], []
    for it in range(max_iters):
        for h, s in zip(hs, part):
            h.batch_iter_partial(s.data_ptr())
        for h in hs:
            h.batch_sync()
        total = part[0].clone()
        for s in part[1:]:
            total += s
        torch.cuda.synchronize()
        totals.append(total)                                       # (alive until every apply that reads it has run)
        kept.append(np.stack([s.cpu().numpy() for s in part]))
        for h in hs:
            h.batch_iter_apply(total.data_ptr())
        if min(h.batch_n_active() for h in hs) == 0:               # (synchronises every handle's stream)
            break
    out = [h.batch_results() for h in hs]
    for p, _ in out[1:]:
        np.testing.assert_array_equal(p, out[0][0])
    return kept, out[0][0], list(out[0][1])


def rank_records(hs, idxs, scan):
    """Every rank's record of `scan` with neighbour indices in the caller's numbering: [(flag, coeff, nn, processed)]."""
    out = []
    for h, idx in zip(hs, idxs):
        flag, coeff, nn = h.get_correspondences(scan)
        if len(idx):
            nn = np.where(nn >= 0, idx[np.clip(nn, 0, len(idx) - 1)], -1).astype(np.int32)
        else:
            assert (nn < 0).all()
        out.append((flag, coeff, nn, nn[:, 0] >= 0))
    return out


def union_records(recs):
    """The union of the ranks' records as lio_multi_get_correspondences forms it, after the guard that no point was
    processed (found its five neighbours), let alone accepted, on two ranks."""
    n = len(recs[0][0])
    times = np.zeros(n, np.int64)
    accepted = np.zeros(n, np.int64)
    flag = np.zeros(n, np.uint8)
    coeff = np.zeros((n, 4), np.float32)
    nn = np.full((n, 5), -1, np.int32)
    for f, c, k, done in recs:
        times += done
        accepted += f.astype(np.int64)
        assert not (f.astype(bool) & ~done).any(), "a rank accepted a point it did not search"
        flag[done], coeff[done], nn[done] = f[done], c[done], k[done]
    assert accepted.max(initial=0) <= 1, "a scan point was accepted on two ranks"
    assert times.max(initial=0) <= 1, "a scan point was searched on two ranks"
    return flag, coeff, nn


def assert_same_record(got, ref):
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))


def one_workgroup_scan(scan, half_extent):
    """At most BLOCK points of `scan` (lidar frame) within `half_extent` of the sensor on every axis, spread over all of
    them: one association workgroup whose box the host knows."""
    near = scan[np.abs(scan).max(1) <= half_extent]
    pick = np.unique(np.round(np.linspace(0, len(near) - 1, min(BLOCK, len(near)))).astype(np.int64)) if len(near) else []
    sub = np.ascontiguousarray(near[pick])
    assert 200 <= len(sub) <= BLOCK, len(sub)
    return sub


def workgroup_cells(scan, pose, plan):
    """[c_lo, c_hi] of one workgroup's box along the slab axis as k_shard_cull forms it: the eight corners of the lidar-
    frame box under the fp32 transform of `pose`, widened by its eps, clamped to the grid."""
    synth, a = _synth(), plan["axis"]
    row = synth.pose_matrix(np.asarray(pose, np.float64)).astype(np.float32)[a]
    lo3, hi3 = scan.min(0), scan.max(0)
    q = [row[0] * (hi3[0] if c & 1 else lo3[0]) + row[1] * (hi3[1] if c & 2 else lo3[1]) + row[2] * (hi3[2] if c & 4 else lo3[2]) + row[3]
         for c in range(8)]
    lo, hi = np.float32(min(q)), np.float32(max(q))
    eps = np.float32(1.0e-4) + np.float32(1.0e-5) * max(abs(lo), abs(hi))
    return int(axis_cell(plan, lo - eps)), int(axis_cell(plan, hi + eps))


def whole_owner(plan, halo, c_lo, c_hi):
    """Rank that takes a workgroup with the cell interval [c_lo, c_hi] whole, or None where the rule falls back to
    per-point ownership (k_shard_cull)."""
    b = plan["bounds"]
    mid = (c_lo + c_hi) >> 1
    r = 0
    while r + 1 < len(b) - 1 and mid >= b[r + 1]:
        r += 1
    return r if halo > 1 and c_lo - 1 >= b[r] - halo and c_hi + 1 < b[r + 1] + halo else None


def sensor_bound_plan(case, qi=0, upper=False):
    """The two-rank plan whose bound is the lower (or the upper) edge of the cell of query qi's true position."""
    plan = lib_plan(case["map"], 2)
    a = plan["axis"]
    ct = int(axis_cell(plan, case["queries"][qi]["pose_true"][3 + a])) + (1 if upper else 0)
    assert 0 < ct < plan["dims"][a]
    return with_bounds(plan, [0, ct, plan["dims"][a]])


def equal_slabs_plan(map_xyz, world):
    plan = lib_plan(map_xyz, world)
    n = int(plan["dims"][plan["axis"]])
    return with_bounds(plan, [n * r // world for r in range(world + 1)])


def moving_workgroup_case(case, qi=2):
    """A one-workgroup scan, a guess and a two-rank plan under which the WHOLE workgroup belongs to rank 1 at the guess
    and to rank 0 at the true pose.  -> (scan, guess, plan).

    The points of one workgroup lie within 6 m of the sensor, and on a street that near field (ground, the facades'
    feet) does not observe the position along the street at all: displaced by 1.2 cells along the planner's axis the
    reference stays displaced for all 8 iterations, with the full 6 m box and with its non-ground points alone, and across
    the street 1.2 cells are beyond the 1 m gate.  So the slabs of this plan are cut ACROSS the street (the second longest
    grid axis: ownership does not care which axis a plan names) and the guess is 0.3 to 0.4 cells off, which the reference
    takes back in one iteration.  For the box's middle cell to change hands on so short a way a cell edge has to lie in
    it: the global grid is laid up to one cell lower (any origin at or below the map's, with dims that still cover it, is
    a valid global grid), and the first (origin, offset) is taken at which the middle cell is one and the same within
    6 cm of the true pose, one and the same within 3 cm of the guess, and higher at the guess."""
    base = lib_plan(case["map"], 2)
    lat = int(np.argsort(base["dims"])[1])
    q = case["queries"][qi]
    scan = one_workgroup_scan(q["scan"], 6.0)
    at_true = q["pose_init"].copy()
    at_true[3 + lat] = q["pose_true"][3 + lat]
    for s in np.arange(0.0, 1.0, 0.1):
        plan = dict(base, axis=lat, origin=base["origin"].copy(), dims=base["dims"].copy())
        plan["origin"][lat] -= np.float32(s) * base["cell"]
        plan["dims"][lat] += 1

        def mid(pose, off):
            lo, hi = workgroup_cells(scan, shift_along_axis(pose, plan, off), plan)
            return (lo + hi) >> 1

        for d in (0.3, 0.35, 0.4):
            guess = shift_along_axis(at_true, plan, d)
            m_true = {mid(at_true, e) for e in (-0.06, 0.0, 0.06)}
            m_guess = {mid(guess, e) for e in (-0.03, 0.0, 0.03)}
            if len(m_true) == 1 and len(m_guess) == 1 and min(m_guess) > max(m_true):
                plan = with_bounds(plan, [0, max(m_true) + 1, plan["dims"][lat]])
                for pose, rank in ((guess, 1), (at_true, 0)):
                    assert whole_owner(plan, LIB_HALO, *workgroup_cells(scan, pose, plan)) == rank
                return scan, guess, plan
    raise AssertionError("no grid origin / offset lets the workgroup change hands")


def stable_scan_case(oracle, case, qi=1, cells=1.2):
    """Query qi displaced by `cells` along the slab axis towards rank 1, with the bound at the upper edge of the sensor's
    true cell (at the lower edge rank 1's count goes 1708, 1665, 1670 in the y frame: no two decreases in a row), restricted to the points the reference accepts BOTH at the displaced guess and at the undisplaced one.
    -> (scan, guess, plan).

    With the whole scan the counts of both ranks grow from iteration to iteration, because obstacles snap in as the
    registration walks back (rank 1: 1855, 1959, 2307, 2423 for query 1), and that hides the ~100 points per cell that
    change hands at the bound.  The restricted scan still walks back (the reference ends 6 cm from the true position)
    and its counts change through ownership."""
    plan = sensor_bound_plan(case, qi, upper=True)
    q = case["queries"][qi]
    guess = shift_along_axis(q["pose_init"], plan, cells)
    ocfg = oracle.default_config(knn_mode=1, n_threads=8)
    keep = (oracle.surf_optimization(ocfg, guess, q["scan"], case["map"])[0] == 1) & \
           (oracle.surf_optimization(ocfg, q["pose_init"], q["scan"], case["map"])[0] == 1)
    return np.ascontiguousarray(q["scan"][keep]), guess, plan


def moved_per_point(n0, n1):
    """Rank 1's count strictly decreasing over three consecutive iterations while rank 0's grows."""
    return any(n1[k] > n1[k + 1] > n1[k + 2] and n0[k] < n0[k + 1] < n0[k + 2] for k in range(len(n0) - 2))


def skewed_map(map_xyz, n_extra=200000, seed=3):
    """map_xyz plus n_extra points packed into ONE cell along the slab axis (0 here: call it on the identity frame), 5 m
    before the map's low end and 30 m up, where no scan point reaches: a point count so skewed that slab bounds coincide."""
    mg = _mg()
    rng = np.random.default_rng(seed)
    mn = map_xyz.min(0)
    lo = np.array([mn[0] - 6.0, 0.5 * (mn[1] + map_xyz[:, 1].max()), 30.0])
    blob = (lo + rng.uniform(0.0, 0.45, (n_extra, 3))).astype(np.float32)     # (origin is min - cell/2: inside the first cell)
    out = np.ascontiguousarray(np.concatenate([map_xyz, blob]))
    plan = mg.plan_shards(out, 4)
    assert plan["axis"] == 0 and len(np.unique(axis_cell(plan, blob[:, 0]))) == 1
    return out


def cube_case(seed=4):
    """About 3000 map points on three mutually orthogonal 2.5 m square faces (4 cells along every axis: fewer cells than
    devices) and a scan of 600 of them seen from a pose about 0.05 m / 0.5 deg off the guess."""
    synth = _synth()
    rng = np.random.default_rng(seed)
    faces = []
    for a in range(3):
        f = rng.uniform(0.0, 2.5, (1000, 3))
        f[:, a] = np.abs(rng.normal(0.0, 0.003, 1000))                  # (inside the faces' 2.5 m box: 4 cells, not 5)
        faces.append(f)
    map_xyz = np.concatenate(faces).astype(np.float32)
    true = np.array([0.02, -0.015, 0.3, 1.2, 1.3, 1.1])
    T = synth.pose_matrix(true)
    pick = rng.choice(len(map_xyz), 600, replace=False)
    scan = ((map_xyz[pick].astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)      # R^T (p - t)
    init = true + np.array([0.006, -0.007, 0.0087, 0.03, -0.03, 0.03])
    return {"map": map_xyz, "scan": np.ascontiguousarray(scan), "pose_init": init.astype(np.float32), "pose_true": true.astype(np.float32)}


def assert_equal_runs(one, many, scans, poses0, record=True):
    """The issue's "equal": status fields and per-iteration counts identical, the recorded association bit for bit, poses
    within TOL_T / TOL_R.  `one` and `many` run the same batch.  -> (poses, results) of `one`."""
    outs = []
    for h in (one, many):
        h.batch_upload(scans); h.batch_set_poses(poses0); h.batch_run()
        outs.append(h.batch_results())
    (p1, r1), (p2, r2) = outs
    for s in range(len(scans)):
        a, b = r1[s], r2[s]
        assert (a.status, a.iters, a.converged, a.is_degenerate) == (b.status, b.iters, b.converged, b.is_degenerate), s
        assert list(a.n_corr_iter) == list(b.n_corr_iter), s
        if record:
            assert_same_record(many.get_correspondences(s), one.get_correspondences(s))
        assert np.abs(p1[s][3:] - p2[s][3:]).max() <= TOL_T and np.abs(p1[s][:3] - p2[s][:3]).max() <= TOL_R, s
    return p1, list(r1)
