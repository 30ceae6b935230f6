"""The planning local map on the device (lio_sor_filter, lio_kf_store_local_map) against the numpy restatement of
tests/localmap_restate.py, stage by stage.  The inputs of the filter tests are tests/test_localmap_cpu.py's, which shows
that none of their points lies inside the threshold bracket: the kept sets must be equal.  At the end: the device's crop on
its four limits, the compaction's patterns beyond 256 workgroups, and crops that leave 1, mean_k and mean_k + 1 points."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_restate as L                                                              # noqa: E402
from test_localmap_cpu import sor_cases, sor_reference, assert_bracket_empty, loop_case, xyzi   # noqa: E402

pytestmark = pytest.mark.gpu
EPS52 = 2.0 ** -52
NAMES = ["street", "corridor", "n257_k1", "n257_k10", "n257_k32", "n513_k1", "n513_k10", "n513_k32", "isolated", "duplicated",
         "planar", "k_plus_1", "k_points", "empty", "nonfinite"]
POSE = np.array([0.01, -0.02, 0.6, 10.5, 0.8, 1.8], np.float32)                          # transformTobeMapped, yaw 34 degrees
CROP = dict(front=16.0, left=12.0, back=8.0, right=12.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stat_difference(a, b):
    """Relative difference of a statistic from the restatement's; NaN must meet NaN, and 0 and inf themselves (inf otherwise)."""
    if math.isnan(b) or math.isnan(a):
        return 0.0 if math.isnan(a) and math.isnan(b) else math.inf
    if b in (0.0, math.inf):
        return 0.0 if a == b else math.inf
    return abs(a - b) / abs(b)


def check_filter(got, ref, pts, what, bracket=True):
    """mean_dist bit for bit, stats to 64 n 2^-52 (NaN = NaN and 0 = 0 exactly), the kept records = the restatement's (its
    bracket is empty; bracket=False for the inputs of tests/sor_cases.py whose note replaces that rule by a sign condition)."""
    inl, dist, stats, rc = got
    n = ref["n_finite"]
    assert rc == ref["rc"], what
    nan_d, nan_r = np.isnan(dist), np.isnan(ref["mean_dist"])
    assert np.array_equal(nan_d, nan_r), what
    n_diff = int((bits(dist)[~nan_d] != bits(ref["mean_dist"])[~nan_r]).sum())
    rel = [stat_difference(a, b) for a, b in zip(stats, ref["stats"])]
    print(f"  {what}: n {n}, kept {len(inl)} / restatement {int(ref['keep'].sum())}, mean_dist differing in {n_diff} points, "
          f"stats {stats} relative differences {rel} (bound {64 * n * EPS52:.3g})")
    assert n_diff == 0, what
    assert max(rel) <= 64 * n * EPS52, what
    if bracket:
        assert_bracket_empty(ref, what)
    assert np.array_equal(bits(inl), bits(pts[ref["keep"]])), what


@pytest.mark.parametrize("name", NAMES)
def test_sor_filter_is_the_restatement(pkg, synth, oracle, name):
    pts, k = sor_cases(synth, oracle)[name]
    check_filter(pkg.sor_filter(pts, k, 1.0), sor_reference(synth, oracle, name), pts, name)


def test_non_finite_records_change_nothing_for_the_others(pkg, synth, oracle):
    cases = sor_cases(synth, oracle)
    bad, clean = pkg.sor_filter(*cases["nonfinite"], 1.0), pkg.sor_filter(*cases["nonfinite_clean"], 1.0)
    fin = np.isfinite(cases["nonfinite"][0][:, :3]).all(1)
    assert np.array_equal(bits(bad[0]), bits(clean[0])) and np.array_equal(bits(bad[1][fin]), bits(clean[1]))
    assert np.isnan(bad[1][~fin]).all() and bad[2] == clean[2] and (bad[3], clean[3]) == (0, 0)


def test_two_runs_give_identical_bytes(pkg, synth, oracle):
    for name in ("isolated", "street"):
        pts, k = sor_cases(synth, oracle)[name]
        a, b = pkg.sor_filter(pts, k, 1.0), pkg.sor_filter(pts, k, 1.0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_refused_arguments_leave_the_filter_usable(pkg, synth, oracle):
    pts, k = sor_cases(synth, oracle)["n257_k10"]
    for bad_k, mul in ((0, 1.0), (33, 1.0), (10, float("nan"))):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            pkg.sor_filter(pts, bad_k, mul)
    check_filter(pkg.sor_filter(pts, k, 1.0), sor_reference(synth, oracle, "n257_k10"), pts, "after the refusals")
    other = pkg.sor_filter(pts, k, 0.25)                                   # another multiplier: another threshold, same distances
    ref = L.sor(pts, k, 0.25)
    assert np.array_equal(bits(other[1]), bits(ref["mean_dist"])) and len(other[0]) < int(sor_reference(synth, oracle, "n257_k10")["keep"].sum())


# ---- lio_kf_store_local_map ---------------------------------------------------------------------------------------------
def make_store(pkg, c):
    """keyframes 0..11 of the run under their poses, keyframe 12 = the revisit under its displaced pose (as tests/test_gpu_icp.py)"""
    st = pkg.KeyframeStore()
    kfs = c["case"]["keyframes"]
    rng = np.random.default_rng(8)
    clouds = [xyzi(cloud, rng) for cloud, _ in kfs] + [xyzi(c["scan"], rng)]
    for cloud in clouds:
        st.add(cloud)
    poses = np.array([p for _, p in kfs] + [c["wrong"]], np.float32)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 10.0)
    return st, poses, clouds


@pytest.fixture(scope="module")
def street(pkg, synth, oracle):
    c = dict(loop_case(synth, oracle, "street"))
    c["store"], c["poses"], c["clouds"] = make_store(pkg, c)
    c["refs"] = {}
    yield c
    c["store"].close()


def stages(pkg, c, n_keyframes, poses=None, pose=POSE, crop=CROP, mean_k=10, mul=1.0):
    """The restatement composed in numpy, once per setting: the K6 sum (lio_assemble_map_resident with a leaf that passes
    through), crop, filter."""
    key = (n_keyframes, pose.tobytes(), tuple(sorted(crop.items())), mean_k, mul, None if poses is None else poses.tobytes())
    if key not in c["refs"]:
        st = c["store"]
        poses = c["poses"] if poses is None else poses
        ids = list(range(max(0, len(st) - n_keyframes), len(st)))
        summed, n_sum, rc = st.assemble(ids, poses[ids], 1e-3)
        assert rc == 1 and n_sum == sum(len(c["clouds"][i]) for i in ids)                # passed through: the sum itself
        cropped, _ = L.crop(summed, pose, **crop)
        r = L.sor(cropped, mean_k, mul)
        assert_bracket_empty(r, key[:1])
        c["refs"][key] = dict(ids=ids, summed=summed, cropped=cropped, sor=r, inliers=cropped[r["keep"]])
    return c["refs"][key]


@pytest.mark.parametrize("n_keyframes", [5, 30])
def test_local_map_stage_by_stage(pkg, street, n_keyframes):
    st = street["store"]
    ref = stages(pkg, street, n_keyframes)
    n = len(ref["cropped"])
    # the crop alone
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=n_keyframes, remove_outliers=0, downsample=0, **CROP))
    assert rc == 0 and (info.first_keyframe, info.n_keyframes) == (ref["ids"][0], len(ref["ids"])) and info.n_keyframes == min(13, n_keyframes)
    assert info.n_summed == len(ref["summed"]) and (info.n_cropped, info.n_inliers, info.n_out) == (n, n, n) and n > 1000
    assert np.array_equal(bits(out), bits(ref["cropped"]))
    assert (info.sor_mean, info.sor_stddev, info.sor_threshold, info.voxel_passthrough) == (0.0, 0.0, 0.0, 0)
    # ... and the filter
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=n_keyframes, downsample=0, **CROP))
    got, want = (info.sor_mean, info.sor_stddev, info.sor_threshold), ref["sor"]["stats"]
    rel = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(f"  {n_keyframes} keyframes: summed {info.n_summed}, cropped {info.n_cropped}, inliers {info.n_inliers}; stats {got} "
          f"relative differences {rel} (bound {64 * n * EPS52:.3g})")
    assert rc == 0 and max(rel) <= 64 * n * EPS52
    assert info.n_inliers == info.n_out == len(ref["inliers"]) < n and np.array_equal(bits(out), bits(ref["inliers"]))
    # ... and K7 at a leaf that filters
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=n_keyframes, leaf=0.4, **CROP))
    vox, vrc = pkg.voxel_grid(ref["inliers"], 0.4)
    assert rc == 0 and vrc == 0 and info.voxel_passthrough == 0 and info.n_out == len(vox) < info.n_inliers == len(ref["inliers"])
    assert np.array_equal(bits(out), bits(vox))
    # the default leaf overflows PCL's voxel index: the inliers pass through, and that is no error
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=n_keyframes, **CROP))
    assert rc == 0 and info.voxel_passthrough == 1 and info.n_out == len(ref["inliers"]) and np.array_equal(bits(out), bits(ref["inliers"]))
    # downsampling without the filter
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=n_keyframes, remove_outliers=0, leaf=0.4, **CROP))
    assert np.array_equal(bits(out), bits(pkg.voxel_grid(ref["cropped"], 0.4)[0])) and info.n_inliers == n


def test_local_map_returns_and_errors(pkg, street):
    st, lib = street["store"], pkg.load_library()
    ref = stages(pkg, street, 5)
    # a crop that excludes everything
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=5, front=2001.0, back=-2000.0))
    assert rc == 0 and len(out) == 0 and (info.n_cropped, info.n_inliers, info.n_out) == (0, 0, 0) and info.n_summed == len(ref["summed"])
    # count only, one record too few, then room
    cfg = pkg.local_map_default_config(n_keyframes=5, **CROP)
    pose_p = POSE.ctypes.data_as(C.POINTER(C.c_float))
    n_out, need = C.c_size_t(), len(ref["inliers"])
    assert lib.lio_kf_store_local_map(st.h, C.byref(cfg), pose_p, None, 32, 0, C.byref(n_out), None) == 0 and n_out.value == need
    buf = np.zeros((need, 8), np.float32)
    assert lib.lio_kf_store_local_map(st.h, C.byref(cfg), pose_p, buf.ctypes.data, 32, need - 1, C.byref(n_out), None) == -1 and n_out.value == need
    assert not buf.any()
    assert lib.lio_kf_store_local_map(st.h, C.byref(cfg), pose_p, buf.ctypes.data, 32, need, C.byref(n_out), None) == 0 and n_out.value == need
    assert np.array_equal(bits(buf[:, :3]), bits(ref["inliers"][:, :3])) and np.array_equal(bits(buf[:, 4]), bits(ref["inliers"][:, 3]))
    # refused: configs out of range, a non-finite pose
    for kw in (dict(n_keyframes=0), dict(mean_k=0), dict(mean_k=33), dict(stddev_mul=float("nan")), dict(leaf=0.0), dict(front=float("inf")),
               dict(left=-50.0), dict(remove_outliers=2), dict(downsample=-1)):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.local_map(POSE, pkg.local_map_default_config(**kw))
    bad = POSE.copy()
    bad[2] = np.nan
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.local_map(bad)
    # an empty store; a store whose last keyframe has no pose
    empty = pkg.KeyframeStore()
    out, info, rc = empty.local_map(POSE)
    assert rc == 0 and len(out) == 0 and info.n_summed == 0
    empty.add(street["clouds"][0]); empty.add(street["clouds"][1])
    empty.set_poses(0, street["poses"][:1], times=[0.0])
    with pytest.raises(pkg.LioError, match="no pose"):
        empty.local_map(POSE)
    empty.set_poses(1, street["poses"][1:2], times=[1.0])
    out, info, rc = empty.local_map(POSE)
    assert rc == 0 and info.n_keyframes == 2 and info.n_summed == len(street["clouds"][0]) + len(street["clouds"][1])
    empty.close()
    # the store still answers
    out, info, rc = st.local_map(POSE, pkg.local_map_default_config(n_keyframes=5, **CROP))
    assert np.array_equal(bits(out), bits(ref["inliers"]))


def test_local_map_follows_the_poses_and_leaves_the_store_alone(pkg, street):
    c = dict(street, refs={})
    st, poses, _ = make_store(pkg, c)
    c["store"] = st
    for cloud in c["clouds"]:
        st.sc_add(cloud)
    cfg = pkg.local_map_default_config(n_keyframes=6, **CROP)
    sc0 = [st.sc_get(k) for k in range(len(st))]
    near0 = st.assemble_nearby(130.0, 0.4)
    kf0 = st.assemble([3, 7], poses[[3, 7]], 1e-3)[0]
    out0, _, _ = st.local_map(POSE, cfg)
    assert np.array_equal(bits(out0), bits(stages(pkg, c, 6)["inliers"]))
    near1 = st.assemble_nearby(130.0, 0.4)
    assert np.array_equal(bits(near0[0]), bits(near1[0])) and np.array_equal(near0[2], near1[2]) and near0[1] == near1[1] > 1000
    assert np.array_equal(bits(kf0), bits(st.assemble([3, 7], poses[[3, 7]], 1e-3)[0]))
    for a, b in zip(sc0, [st.sc_get(k) for k in range(len(st))]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # correctPoses: every pose rewritten, the next call uses the new ones
    moved = poses.copy()
    moved[:, 3] += np.float32(0.5); moved[:, 2] += np.float32(0.02)
    st.set_poses(0, moved)
    out1, _, _ = st.local_map(POSE, cfg)
    assert np.array_equal(bits(out1), bits(stages(pkg, c, 6, poses=moved)["inliers"])) and not np.array_equal(bits(out1), bits(out0))
    st.close()


# ---- the crop and the pass-through at their edges (one keyframe under the zero pose, the vehicle at the zero pose) ---------
ZERO = np.zeros(6, np.float32)


def one_keyframe_store(pkg, oracle, cloud):
    """A store whose only keyframe is `cloud` under the zero pose.  First, on the CPU: K6 under the zero pose returns its
    input bits (the oracle's transform; a NaN stays a NaN), so what reaches the crop is the cloud itself."""
    moved = oracle.transform_point_cloud(cloud, ZERO)
    fin = np.isfinite(cloud).all(1)
    assert np.array_equal(bits(moved[fin]), bits(cloud[fin])) and np.isnan(moved[~fin]).any(1).all()
    st = pkg.KeyframeStore()
    st.add(cloud)
    st.set_poses(0, ZERO[None], times=[0.0])
    return st


def limit_records():
    """The records of tests/test_localmap_cpu.py::test_crop_keeps_its_four_limits: each limit, one ulp outside, a NaN."""
    up, dn = lambda v: np.nextafter(np.float32(v), np.float32(np.inf)), lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    return np.array([[40, 0, 1, 7], [up(40), 0, 1, 7], [-40, 0, 1, 7], [dn(-40), 0, 1, 7],
                     [0, 70, 1, 7], [0, up(70), 1, 7], [0, -20, 1, 7], [0, dn(-20), 1, 7], [np.nan, 0, 0, 7]], np.float32)


def test_device_crop_keeps_its_four_limits(pkg, oracle):
    pts = limit_records()
    want, keep = L.crop(pts, ZERO)
    assert keep.tolist() == [True, False] * 4 + [False] and np.array_equal(bits(want), bits(pts[keep]))
    st = one_keyframe_store(pkg, oracle, pts)
    out, info, rc = st.local_map(ZERO, pkg.local_map_default_config(remove_outliers=0, downsample=0))
    st.close()
    assert rc == 0 and (info.n_summed, info.n_cropped, info.n_inliers, info.n_out) == (9, 4, 4, 4)
    assert np.array_equal(bits(out), bits(pts[keep]))


@pytest.fixture(scope="module")
def compaction_case():
    """65 793 records = 257 workgroups + 1 (tests/sor_cases.py wg_257, the size case): from there the scan over the workgroups'
    counts takes its second chunk.  Rejected records are moved out of the crop by workgroup and lane."""
    import sor_cases as S
    cloud = S.build_case("wg_257")[0].copy()
    n = len(cloud)
    wg, lane = np.arange(n) // 256, np.arange(n) % 256
    keep = np.ones(n, bool)
    keep[wg == 0] = False                                                     # a whole workgroup of rejects, the first
    keep[wg == 130] = False                                                   # ... and one in the middle
    keep[(wg == 1) & (lane != 0)] = False                                     # survivors only in lane 0
    keep[(wg == 2) & (lane != 255)] = False                                   # ... only in lane 255
    keep[(wg == 3) & (lane != 63) & (lane != 64)] = False                     # ... only across the wave boundary
    keep[(wg == 255) & (lane % 2 == 0)] = False                               # around the scan's chunk boundary
    keep[(wg == 256) & (lane < 128)] = False
    assert keep[wg == 4].all() and keep[n - 1] and wg[n - 1] == 257           # whole workgroups kept; the last, one-point workgroup kept
    cloud[~keep, 0] += np.float32(200.0)
    crop = dict(front=70.0, left=40.0, back=20.0, right=70.0)
    want, kept = L.crop(cloud, ZERO, **crop)
    assert np.array_equal(kept, keep) and np.array_equal(bits(want), bits(cloud[keep]))
    ref = L.sor(want, 1, 1.0, knn=L.knn_d2_fast)
    assert_bracket_empty(ref, "compaction")
    return dict(cloud=cloud, crop=crop, want=want, sor=ref)


def test_compaction_patterns_beyond_256_workgroups(pkg, oracle, compaction_case):
    c = compaction_case
    st = one_keyframe_store(pkg, oracle, c["cloud"])
    out, info, rc = st.local_map(ZERO, pkg.local_map_default_config(remove_outliers=0, downsample=0, **c["crop"]))
    assert rc == 0 and (info.n_summed, info.n_cropped, info.n_out) == (len(c["cloud"]), len(c["want"]), len(c["want"]))
    assert np.array_equal(bits(out), bits(c["want"]))                          # = L.crop, in order
    # the filter on that crop, alone and inside the chain
    check_filter(pkg.sor_filter(c["want"], 1, 1.0), c["sor"], c["want"], "the filter on the crop")
    out, info, rc = st.local_map(ZERO, pkg.local_map_default_config(mean_k=1, downsample=0, **c["crop"]))
    st.close()
    inl = c["want"][c["sor"]["keep"]]
    assert rc == 0 and info.n_inliers == info.n_out == len(inl) < info.n_cropped and np.array_equal(bits(out), bits(inl))
    assert max(stat_difference(a, b) for a, b in zip((info.sor_mean, info.sor_stddev, info.sor_threshold), c["sor"]["stats"])) \
        <= 64 * len(c["want"]) * EPS52


def test_a_crop_that_leaves_at_most_mean_k_points_passes_through(pkg, oracle):
    """mean_k 10.  Eleven points at x = 1 .. 11 m (uneven in y and z) and 400 beyond the crop; `right` leaves 1, 10 and 11."""
    rng = np.random.default_rng(31)
    near = np.stack([np.arange(1.0, 12.0), rng.uniform(-3, 3, 11), rng.uniform(0, 1, 11)], 1)
    far = rng.uniform(-5, 5, (400, 3)) + np.array([100.0, 0, 0])
    cloud = xyzi(np.concatenate([far[:200], near, far[200:]], 0), rng)
    st = one_keyframe_store(pkg, oracle, cloud)
    for right, n in ((1.5, 1), (10.5, 10)):
        want, _ = L.crop(cloud, ZERO, right=right)
        assert len(want) == n
        out, info, rc = st.local_map(ZERO, pkg.local_map_default_config(right=right, downsample=0))
        assert rc == 0 and info.n_cropped == info.n_inliers == info.n_out == n
        assert (info.sor_mean, info.sor_stddev, info.sor_threshold) == (0.0, 0.0, np.inf)
        assert np.array_equal(bits(out), bits(want))
        out, info, rc = st.local_map(ZERO, pkg.local_map_default_config(right=right, leaf=2.5))      # K7 behind it still runs
        vox, vrc = pkg.voxel_grid(want, 2.5)
        assert rc == 0 and vrc == 0 and info.voxel_passthrough == 0 and info.n_inliers == n and info.n_out == len(vox)
        assert np.array_equal(bits(out), bits(vox)) and (n == 1 or len(vox) < n)
    want, _ = L.crop(cloud, ZERO, right=11.5)                                  # mean_k + 1 points: the filter proper
    ref = L.sor(want, 10, 1.0)
    assert len(want) == 11 and ref["rc"] == 0 and 0 < int(ref["keep"].sum()) < 11
    assert_bracket_empty(ref, "mean_k + 1")
    out, info, rc = st.local_map(ZERO, pkg.local_map_default_config(right=11.5, downsample=0))
    st.close()
    assert rc == 0 and info.n_cropped == 11 and info.n_inliers == info.n_out == int(ref["keep"].sum())
    assert np.array_equal(bits(out), bits(want[ref["keep"]]))
    assert max(stat_difference(a, b) for a, b in zip((info.sor_mean, info.sor_stddev, info.sor_threshold), ref["stats"])) <= 64 * 11 * EPS52
