"""Loop-closure ICP on the device (lio_icp_align, lio_kf_store_loop_icp, lio_kf_store_detect_loop, lio_icp_debug_trace)
against the numpy restatement of tests/icp_restate.py, step by step: a 100-step trajectory is not judged by its end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restate as R                                    # noqa: E402
from test_icp_cpu import street_loop_case, pose_error     # noqa: E402

pytestmark = pytest.mark.gpu
LEAF = 0.4
EPS52 = 2.0 ** -52


def xyzi(xyz):
    xyz = np.asarray(xyz, np.float32)
    return np.concatenate([xyz[:, :3], np.zeros((len(xyz), 1), np.float32)], 1)


def make_store(pkg, c):
    """keyframes 0..11 of the run under their poses, keyframe 12 = the revisit under its displaced pose"""
    st = pkg.KeyframeStore()
    kfs = c["case"]["keyframes"]
    for cloud, _ in kfs:
        st.add(xyzi(cloud))
    st.add(xyzi(c["scan"]))
    poses = np.array([p for _, p in kfs] + [c["wrong"]], np.float32)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 10.0)
    return st, poses


@pytest.fixture(scope="module")
def street(pkg, synth, oracle):
    c = street_loop_case(synth, oracle)
    c["store"], c["poses"] = make_store(pkg, c)
    yield c
    c["store"].close()


@pytest.fixture(scope="module")
def corridor(pkg, synth, oracle):
    c = street_loop_case(synth, oracle, kind="corridor", seed=5)      # ground plus two walls
    c["store"], c["poses"] = make_store(pkg, c)
    yield c
    c["store"].close()


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k in R.DEFAULTS}


def ulps(a, ref):
    a, ref = np.asarray(a, np.float32), np.asarray(ref, np.float32)
    return np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref), np.abs(a))).astype(np.float64)


def stepwise(pkg, src, tgt, cfg, must_reflect_at0=False, guess=None, judge_step=None):
    """The step-wise parity of the issue; returns (result, worst step ulp, trace length).  guess: the 4x4 the alignment
    starts from.  judge_step(k, device step, restated step, paired source, paired target) replaces the 2 ulp rule where a
    caller has a rule of its own for steps whose entries an ulp does not measure (tests/test_gpu_icp_edges.py)."""
    cd = cfg_dict(cfg)
    res, steps, n_corr, mse, _ = pkg.icp_debug_trace(src, tgt, cfg, guess=guess)
    k_n = len(steps)
    assert k_n >= 1
    final = np.eye(4, dtype=np.float32) if guess is None else np.array(guess, np.float32).reshape(4, 4)
    cur = R.transform_points(final, src[:, :3])
    crit = R.Criteria(cd)
    worst = 0.0
    stop = None
    for k in range(k_n):
        res_k, steps_k, n_corr_k, mse_k, corr_dev = pkg.icp_debug_trace(src, tgt, cfg, guess=guess, rec_iter=k)
        assert np.array_equal(steps_k, steps) and np.array_equal(n_corr_k, n_corr) and np.array_equal(mse_k, mse)   # run to run
        corr, mse_r, n = R.correspondences(cur, tgt[:, :3], cd)
        assert np.array_equal(corr_dev, corr), (k, int((corr_dev != corr).sum()))
        assert n_corr[k] == n
        assert abs(mse[k] - mse_r) <= n * EPS52 * abs(mse_r), (k, mse[k], mse_r)
        if n < cd["min_corr"]:
            stop = (k, 0, R.NO_CORRESPONDENCES)
            break
        keep = corr >= 0
        step_r, refl = R.umeyama_step(cur[keep], tgt[corr[keep], :3])
        if k == 0 and must_reflect_at0:
            assert refl
        if judge_step is not None:
            judge_step(k, steps[k], step_r, cur[keep], tgt[corr[keep], :3])
        else:
            u = float(ulps(steps[k], step_r).max())
            print(f"  iteration {k}: n_corr {n} mse {mse[k]:.9g} step differs from the restatement by at most {u:.2f} ulp")
            worst = max(worst, u)
        assert abs(np.linalg.det(steps[k][:3, :3].astype(np.float64)) - 1.0) < 1e-5
        # the restatement continues from the DEVICE's step: input_transformed and final bit for bit
        cur = R.transform_points(steps[k], cur)
        final = R.compose(steps[k], final)
        conv, state = crit.has_converged(k + 1, steps[k], float(mse[k]))
        if conv:
            stop = (k, 1, state)
            break
    assert stop is not None and stop[0] == k_n - 1, (stop, k_n)
    assert (res.converged, res.state) == (stop[1], stop[2])
    assert res.iters == (k_n if stop[1] else k_n - 1) and res.n_corr_last == n_corr[-1]
    assert np.array_equal(np.array(res.T, np.float32).reshape(4, 4), final)
    assert worst <= 2.0, f"step differs by {worst:.2f} fp32 ulp"
    return res, worst, k_n


def device_submaps(c, pose_index=-1):
    res, rc, clouds = c["store"].loop_icp(12, 7, 4, LEAF, pose_index=pose_index, want_clouds=True)
    return res, rc, clouds


def test_submaps_are_the_resident_assembly_bit_for_bit(street):
    st, poses = street["store"], street["poses"]
    for pi in (-1, 5):
        res, rc, (src, tgt, closed) = device_submaps(street, pi)
        assert rc == 0 and res.status == 0
        ids = list(range(3, 12))
        ref_s, n_s, _ = st.assemble([12], poses[[12 if pi < 0 else pi]], LEAF)
        ref_t, n_t, _ = st.assemble(ids, poses[ids] if pi < 0 else np.repeat(poses[[pi]], len(ids), 0), LEAF)
        assert (res.n_source, res.n_target) == (n_s, n_t) and n_s >= 300 and n_t >= 1000
        assert np.array_equal(src.view(np.uint32), ref_s.view(np.uint32))
        assert np.array_equal(tgt.view(np.uint32), ref_t.view(np.uint32))
        # closed_cloud MO:1131 = the source under the final transformation
        ref_c = R.transform_points(np.array(res.T, np.float32).reshape(4, 4), src[:, :3])
        assert np.array_equal(closed[:, :3].view(np.uint32), ref_c.view(np.uint32)) and np.array_equal(closed[:, 3], src[:, 3])


def test_align_on_the_submaps_is_byte_identical(pkg, street):
    res, rc, (src, tgt, _) = device_submaps(street)
    res2, rc2 = pkg.icp_align(src, tgt)
    assert rc == rc2 == 0
    for f, _ in pkg.IcpResult._fields_:
        if f != "pose_corrected":
            a, b = getattr(res, f), getattr(res2, f)
            assert (bytes(a) == bytes(b)) if hasattr(a, "_length_") else (a == b), f
    assert list(res2.pose_corrected) == [0.0] * 6
    res3, _ = pkg.icp_align(src, tgt, pkg.icp_default_config(lookahead=1))      # how far the host looks ahead changes nothing
    assert bytes(res3.T) == bytes(res.T) and (res3.iters, res3.state, res3.fitness) == (res.iters, res.state, res.fitness)


def test_stepwise_parity_street(pkg, street):
    _, _, (src, tgt, _) = device_submaps(street)
    res, worst, k_n = stepwise(pkg, src, tgt, pkg.icp_default_config())
    print(f"street: {k_n} iterations, state {pkg.ICP_STATES[res.state]}, worst step difference {worst:.2f} ulp")
    assert res.state in (R.TRANSFORM, R.ABS_MSE, R.REL_MSE)


def test_stepwise_parity_corridor(pkg, corridor):
    _, _, (src, tgt, _) = device_submaps(corridor)
    res, worst, k_n = stepwise(pkg, src, tgt, pkg.icp_default_config())
    print(f"corridor: {k_n} iterations, state {pkg.ICP_STATES[res.state]}, worst step difference {worst:.2f} ulp")


def test_stepwise_parity_with_a_gate_that_bites_and_an_iteration_cap(pkg, street):
    _, _, (src, tgt, _) = device_submaps(street)
    res, _, k_n = stepwise(pkg, src, tgt, pkg.icp_default_config(max_corr_dist=0.35, max_iters=4))
    assert res.n_corr_last < len(src)                     # the gate rejected points
    assert (res.state, k_n) == (R.ITERATIONS, 4) or res.state in (R.TRANSFORM, R.ABS_MSE, R.REL_MSE)


def test_reflection_case_gives_a_proper_rotation(pkg):
    """A thin slab whose copy is mirrored in z: every point's neighbour is its own mirror image, the cross-covariance has a
    negative determinant and Umeyama's sign rule must flip the last singular direction.  One iteration: that is the step
    with the reflection.  (Later steps of this set are nearly the identity with third-axis entries around 1e-9, whose
    fp32 ulp is no measure of anything: 944 ulp of such an entry were seen at iteration 1.)"""
    rng = np.random.default_rng(7)
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 2)
    z = rng.uniform(0.01, 0.05, len(g)) * rng.choice([-1.0, 1.0], len(g))
    src = np.concatenate([g * 1.5, z[:, None]], 1).astype(np.float32)
    tgt = src * np.array([1, 1, -1], np.float32)
    res, _, k_n = stepwise(pkg, src, tgt, pkg.icp_default_config(max_iters=1), must_reflect_at0=True)
    assert (k_n, res.state) == (1, R.ITERATIONS)


def test_fitness_and_corrected_pose(pkg, street):
    res, rc, (src, tgt, _) = device_submaps(street)
    T = np.array(res.T, np.float32).reshape(4, 4)
    fit = R.fitness(T, src[:, :3], tgt[:, :3])
    assert abs(res.fitness - fit) <= len(src) * EPS52 * fit, (res.fitness, fit)
    assert res.accepted == int(res.converged and res.fitness <= 0.3) == 1
    ref = R.pose_corrected(T, street["wrong"])
    got = np.array(res.pose_corrected, np.float64)
    assert np.abs(got[3:] - ref[3:]).max() <= 1e-5 and np.abs(got[:3] - ref[:3]).max() <= 1e-6, (got, ref)


def test_end_to_end_street_pose_error(street):
    res, rc, (src, tgt, _) = device_submaps(street)
    r = R.icp(src, tgt)
    assert r["converged"] == 1 and r["state"] in (R.TRANSFORM, R.ABS_MSE, R.REL_MSE) and r["iters"] < 100
    dt_r, dr_r = pose_error(R.pose_corrected(r["T"], street["wrong"]), street["true"])
    dt_d, dr_d = pose_error(res.pose_corrected, street["true"])
    print(f"street pose error to the ground truth: device {dt_d:.4f} m / {dr_d:.5f} rad after {res.iters} iterations, "
          f"restatement {dt_r:.4f} m / {dr_r:.5f} rad after {r['iters']}; fitness {res.fitness:.5f} / {r['fitness']:.5f}")
    assert dt_d <= 2.0 * dt_r and dr_d <= 2.0 * dr_r


def test_guards_and_edge_inputs(pkg, street):
    st = street["store"]
    lib = pkg.load_library()
    # MO:1104: too few points in either submap -> soft status, nothing aligned
    for kw in (dict(min_source_points=10 ** 6), dict(min_target_points=10 ** 6)):
        res, rc, _ = st.loop_icp(12, 7, 4, LEAF, cfg=pkg.icp_default_config(**kw))
        assert rc == 1 and res.status == 1 and res.iters == 0 and res.converged == 0 and res.accepted == 0
    # key_pre +- search_num running off both ends of the store
    res, rc, clouds = st.loop_icp(12, 1, 50, LEAF, want_clouds=True)
    ref_t, n_t, _ = st.assemble(list(range(13)), street["poses"], LEAF)
    assert rc == 0 and res.n_target == n_t and np.array_equal(clouds[1].view(np.uint32), ref_t.view(np.uint32))
    # ids outside the store, a bad leaf
    cfg, r = pkg.icp_default_config(), pkg.IcpResult()
    for args in ((13, 7, 4, -1, LEAF), (12, -1, 4, -1, LEAF), (12, 7, -1, -1, LEAF), (12, 7, 4, 13, LEAF), (12, 7, 4, -1, 0.0)):
        assert lib.lio_kf_store_loop_icp(st.h, *args[:4], C.c_float(args[4]), C.byref(cfg), C.byref(r), None) == -1, args
    # an output that is too small: the needed counts, nothing aligned
    buf = np.zeros((8, 8), np.float32)
    cl = pkg.IcpClouds(buf.ctypes.data, None, None, 8, 0, 0, 0, 0, 0, 32)
    assert lib.lio_kf_store_loop_icp(st.h, 12, 7, 4, -1, LEAF, C.byref(cfg), C.byref(r), C.byref(cl)) == -1
    assert cl.n_source == res.n_source and cl.n_target > 1000
    rng = np.random.default_rng(4)
    tgt = rng.uniform(-10, 10, (3000, 3)).astype(np.float32)
    src = tgt[::3] + np.float32(0.02)
    # a source farther than max_corr_dist from every target point
    res, rc = pkg.icp_align(src + np.float32(100.0), tgt)
    assert rc == 0 and (res.converged, res.state, res.iters, res.n_corr_last, res.accepted) == (0, R.NO_CORRESPONDENCES, 0, 0, 0)
    assert np.array_equal(np.array(res.T).reshape(4, 4), np.eye(4)) and res.fitness > 100.0 ** 2       # the score has no gate
    # empty and one-point clouds
    for s, t in ((src[:0], tgt), (src, tgt[:0]), (src[:0], tgt[:0])):
        res, rc = pkg.icp_align(s, t)
        assert rc == 0 and (res.converged, res.state, res.iters) == (0, R.NO_CORRESPONDENCES, 0) and res.fitness == R.DBL_MAX
    res, rc = pkg.icp_align(src[:1], tgt)
    assert rc == 0 and (res.converged, res.state, res.n_corr_last) == (0, R.NO_CORRESPONDENCES, 1)
    wide = pkg.icp_default_config(max_corr_dist=100.0)
    res, rc = pkg.icp_align(src, tgt[:1], wide)
    assert rc == 0 and res.n_corr_last == len(src) and np.isfinite(res.fitness)
    assert abs(np.linalg.det(np.array(res.T, np.float64).reshape(4, 4)[:3, :3]) - 1.0) < 1e-4
    # a target that is one point repeated
    res, rc = pkg.icp_align(src, np.repeat(tgt[:1], 500, 0), wide)
    assert rc == 0 and res.n_corr_last == len(src) and np.isfinite(res.fitness)
    # NaN / inf coordinates are skipped on both sides: the same answer as without them
    clean, _ = pkg.icp_align(src, tgt)
    s_bad = np.concatenate([src, [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]], 0).astype(np.float32)
    t_bad = np.concatenate([tgt, [[np.inf, 0, 0], [np.nan, np.nan, np.nan]]], 0).astype(np.float32)
    res, rc = pkg.icp_align(s_bad, t_bad)
    assert rc == 0 and bytes(res.T) == bytes(clean.T) and (res.iters, res.state, res.fitness) == (clean.iters, clean.state, clean.fitness)
    assert clean.converged == 1
    res, rc = pkg.icp_align(src, np.full((10, 3), np.nan, np.float32))
    assert rc == 0 and res.state == R.NO_CORRESPONDENCES
    # the store works afterwards
    res, rc, _ = st.loop_icp(12, 7, 4, LEAF)
    assert rc == 0 and res.converged == 1 and res.accepted == 1


def test_detect_loop_against_the_literal_loop(pkg, synth):
    rng = np.random.default_rng(9)
    cloud = np.zeros((4, 4), np.float32)

    def run(xyz, times, radius, time_diff, time_cur):
        st = pkg.KeyframeStore()
        for _ in xyz:
            st.add(cloud)
        poses = np.zeros((len(xyz), 6), np.float32)
        poses[:, 3:] = xyz
        st.set_poses(0, poses, times=times)
        got = st.detect_loop(radius, time_diff, time_cur)
        st.close()
        assert got == R.detect_loop_literal(poses[:, 3:], times, radius, time_diff, time_cur), (got, radius, time_diff)
        return got

    # straight run: nothing old enough within the radius
    straight = synth.keyframe_poses(120, seed=1)[:, 3:]
    t = np.arange(120) * 1.0
    assert run(straight, t, 15.0, 30.0, 119.0) is None
    assert run(straight, t, 15.0, 5.0, 119.0) == (119, 113)
    # lawn-mower: the neighbouring row is close in space and old
    lawn = synth.keyframe_poses(300, seed=2, lawnmower=True)[:, 3:]
    t = np.arange(300) * 1.0
    got = run(lawn, t, 15.0, 30.0, 299.0)
    assert got is not None and got[0] == 299 and t[got[1]] < 299.0 - 30.0
    # the nearest pose is too young, the second nearest is taken
    xyz = np.array([[0.5, 0, 0], [5, 0, 0], [0.2, 0, 0], [0, 0, 0]], np.float32)
    assert run(xyz, np.array([0.0, 1.0, 99.0, 100.0]), 15.0, 30.0, 100.0) == (3, 0)
    # equal distances: the lower index; only the last key itself: none
    xyz = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 0]], np.float32)
    assert run(xyz, np.array([0.0, 0.0, 100.0]), 15.0, 30.0, 100.0) == (2, 0)
    assert run(xyz[2:], np.array([0.0]), 15.0, -1.0, 100.0) is None
    for _ in range(5):
        n = int(rng.integers(2, 200))
        run(rng.uniform(-20, 20, (n, 3)).astype(np.float32), rng.uniform(0, 100, n), 15.0, 30.0, 100.0)
