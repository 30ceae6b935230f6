"""Loop-closure ICP, the part that needs no GPU: the numpy restatement (tests/icp_restate.py) against closed forms, the ABI
structs and defaults, refused configs, and the no-device answer of the device entry points.  lio_kf_store_detect_loop is
host code but lives on a store, which only a device can create: its test is in tests/test_gpu_icp.py."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restate as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def street_loop_case(synth, oracle, kind="street", seed=3):
    """A 12-keyframe run and one more visit of its end whose pose is off by 0.3 m / 1 degree: keyframes (cloud, pose), the
    displaced pose, the true one, and the two submaps as loopFindNearKeyframes builds them (leaf 0.4)."""
    case = synth.make_case("vlp16", n_keyframes=12, seed=seed, kind=kind, device="cpu")
    q = case["queries"][0]
    wrong = q["pose_true"].astype(np.float64).copy()
    wrong[3] += 0.25; wrong[4] -= 0.15; wrong[5] += 0.05; wrong[2] += np.radians(1.0)      # |dt| = 0.296 m
    wrong = wrong.astype(np.float32)

    def world(xyz, pose):
        return oracle.transform_point_cloud(np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1), pose)

    def vox(c):
        out = oracle.voxel_grid(c, 0.4)
        return out[0] if isinstance(out, tuple) else out

    src = vox(world(q["scan"], wrong))
    tgt = vox(np.concatenate([world(*case["keyframes"][i]) for i in range(3, 12)], 0))
    return dict(case=case, scan=q["scan"], wrong=wrong, true=q["pose_true"], src=src, tgt=tgt)


def pose_error(pose, true):
    d = np.asarray(pose, np.float64) - np.asarray(true, np.float64)
    return float(np.linalg.norm(d[3:])), float(np.abs(d[:3]).max())


def test_umeyama_step_is_the_closed_form_on_exact_pairs():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(1)
    for _ in range(20):
        s = rng.uniform(-20, 20, (200, 3))
        rot = Rotation.from_rotvec(rng.normal(0, 0.3, 3))
        t = rot.apply(s) + rng.uniform(-3, 3, 3)
        s32, t32 = s.astype(np.float32), t.astype(np.float32)
        step, refl = R.umeyama_step(s32, t32)
        assert not refl
        s64, t64 = s32.astype(np.float64), t32.astype(np.float64)
        ref, _ = Rotation.align_vectors(t64 - t64.mean(0), s64 - s64.mean(0))
        np.testing.assert_allclose(step[:3, :3], ref.as_matrix(), atol=2e-6)
        np.testing.assert_allclose(step[:3, 3], t64.mean(0) - ref.as_matrix() @ s64.mean(0), atol=2e-5)
        assert np.array_equal(step[3], [0, 0, 0, 1])


def test_mirrored_pairs_yield_a_proper_rotation():
    rng = np.random.default_rng(2)
    s = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    t = s * np.array([1, 1, -1], np.float32)                      # a reflection: no rotation maps s onto t
    step, refl = R.umeyama_step(s, t)
    assert refl
    Rm = step[:3, :3].astype(np.float64)
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-6
    np.testing.assert_allclose(Rm @ Rm.T, np.eye(3), atol=1e-6)


def test_brute_force_nn_is_the_kdtree_nn_and_ties_go_down():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-30, 30, (4000, 3)).astype(np.float32)
    src = rng.uniform(-35, 35, (1500, 3)).astype(np.float32)
    idx, d2 = R.nn_brute(src, tgt)
    dk, ik = cKDTree(tgt.astype(np.float64)).query(src.astype(np.float64))
    same = idx == ik
    # where the fp64 tree disagrees the two candidates are equally far in fp32
    d2k = ((src - tgt[ik]) ** 2).astype(np.float32)
    assert same.mean() > 0.999
    assert np.all(np.abs(d2[~same] - (d2k[~same, 0] + d2k[~same, 1] + d2k[~same, 2])) <= 1e-5 * d2[~same])
    np.testing.assert_allclose(np.sqrt(d2.astype(np.float64)), dk, rtol=1e-5, atol=1e-6)
    # tied points: every target point twice, and a query midway between two of them
    tied = np.concatenate([tgt[:50], tgt[:50]], 0)
    idx_t, _ = R.nn_brute(tgt[:50], tied)
    assert np.array_equal(idx_t, np.arange(50))
    pair = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 0]], np.float32)
    assert R.nn_brute(np.array([[1, 0, 0]], np.float32), pair)[0][0] == 0


def test_known_answer_alignment_on_the_street(synth, oracle):
    c = street_loop_case(synth, oracle)
    assert len(c["src"]) >= 300 and len(c["tgt"]) >= 1000          # the size guards of MO:1104
    r = R.icp(c["src"], c["tgt"])
    assert r["converged"] == 1 and r["state"] in (R.TRANSFORM, R.ABS_MSE, R.REL_MSE) and r["iters"] < 100
    dt0, dr0 = pose_error(c["wrong"], c["true"])
    dt, dr = pose_error(R.pose_corrected(r["T"], c["wrong"]), c["true"])
    print(f"street: {r['iters']} iterations, state {r['state']}, fitness {r['fitness']:.4f}, |dt| {dt0:.3f} -> {dt:.3f} m, "
          f"max |dr| {dr0:.4f} -> {dr:.4f} rad")
    assert dt0 > 0.29 and dr0 > 0.017
    assert dt < 0.1 and dr < 0.005                                  # centimetres of sampling noise, not the 0.3 m / 1 degree
    assert r["fitness"] <= 0.3


def test_struct_layouts_match_c(pkg):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "liogpu.h"
    int main(void) {
        printf("%zu %zu %zu\n", sizeof(lio_icp_config), sizeof(lio_icp_result), sizeof(lio_icp_clouds));
        printf("%zu %zu %zu %zu\n", offsetof(lio_icp_config, fitness_max), offsetof(lio_icp_config, max_iters),
               offsetof(lio_icp_config, min_target_points), offsetof(lio_icp_config, lookahead));
        printf("%zu %zu %zu %zu %zu\n", offsetof(lio_icp_result, n_corr_last), offsetof(lio_icp_result, n_launches),
               offsetof(lio_icp_result, fitness), offsetof(lio_icp_result, T), offsetof(lio_icp_result, pose_corrected));
        printf("%zu %zu %zu\n", offsetof(lio_icp_clouds, cap_source), offsetof(lio_icp_clouds, n_closed), offsetof(lio_icp_clouds, stride));
        printf("%d %d\n", LIO_ICP_MAX_ITERS, LIO_ICP_NO_CORRESPONDENCES);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        v = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    cfg, res, cl = pkg.IcpConfig, pkg.IcpResult, pkg.IcpClouds
    assert v[:3] == [C.sizeof(cfg), C.sizeof(res), C.sizeof(cl)]
    assert v[3:7] == [cfg.fitness_max.offset, cfg.max_iters.offset, cfg.min_target_points.offset, cfg.lookahead.offset]
    assert v[7:12] == [res.n_corr_last.offset, res.n_launches.offset, res.fitness.offset, res.T.offset, res.pose_corrected.offset]
    assert v[12:15] == [cl.cap_source.offset, cl.n_closed.offset, cl.stride.offset]
    assert v[15:] == [1000, 5] and pkg.ICP_STATES[5] == "NO_CORRESPONDENCES"


def test_defaults_are_the_cited_literals(pkg):
    c = pkg.icp_default_config()
    assert (c.max_corr_dist, c.max_iters, c.transform_eps, c.fitness_eps) == (30.0, 100, 1e-6, 1e-6)       # MO:1112-1115
    assert (c.rel_mse_eps, c.rotation_threshold, c.min_corr, c.max_similar) == (1e-5, 0.99999, 3, 0)       # PCL 1.10
    assert (c.min_source_points, c.min_target_points, c.fitness_max) == (300, 1000, 0.3)                   # MO:1104, UT:324
    assert c.lookahead == 0
    d = {k: getattr(c, k) for k in R.DEFAULTS}
    assert d == R.DEFAULTS                                          # the checker restates the same numbers


BAD = [("max_corr_dist", 0.0), ("max_corr_dist", float("nan")), ("max_corr_dist", float("inf")), ("max_iters", 0),
       ("max_iters", 1001), ("transform_eps", -1e-9), ("fitness_eps", float("nan")), ("rel_mse_eps", -1.0),
       ("rotation_threshold", 1.5), ("fitness_max", -0.1), ("min_corr", 0), ("max_similar", -1), ("min_source_points", -1),
       ("min_target_points", -5), ("lookahead", 65)]


@pytest.mark.parametrize("field,bad", BAD)
def test_out_of_range_icp_config_is_refused_not_clamped(pkg, field, bad):
    lib = pkg.load_library()
    pts = np.zeros((8, 3), np.float32)
    cfg = pkg.icp_default_config(**{field: bad})
    res = pkg.IcpResult()
    args = (0, pts.ctypes.data, 8, 12, pts.ctypes.data, 8, 12, C.byref(cfg), None)
    assert lib.lio_icp_align(*args, C.byref(res)) == -1, (field, bad)                                   # LIO_ERR_ARG, no device touched
    assert lib.lio_icp_debug_trace(*args, -1, C.byref(res), None, None, None, None, None) == -1
    assert lib.lio_kf_store_loop_icp(None, 0, 0, 0, -1, 0.4, C.byref(cfg), C.byref(res), None) == -1
    assert lib.lio_icp_align(0, pts.ctypes.data, 8, 10, pts.ctypes.data, 8, 12, C.byref(pkg.icp_default_config()), None, C.byref(res)) == -1


def test_no_device_no_fallback(pkg):
    """Without a GPU the device entry points answer LIO_ERR_NO_DEVICE.  lio_kf_store_loop_icp works on a store, and no store
    exists without a device: it is lio_kf_store_create that answers for that path."""
    import torch
    lib = pkg.load_library()
    rng = np.random.default_rng(0)
    tgt = rng.uniform(-5, 5, (2000, 3)).astype(np.float32)
    src = (tgt[::4] + np.float32(0.05)).astype(np.float32)
    if torch.cuda.is_available():
        res, rc = pkg.icp_align(src, tgt)
        assert rc == 0 and res.converged == 1
        return
    with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
        pkg.icp_align(src, tgt)
    with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
        pkg.icp_debug_trace(src, tgt, rec_iter=0)
    h = C.c_void_p()
    assert lib.lio_kf_store_create(0, C.byref(h)) == -5 and not h.value
    with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
        pkg.KeyframeStore()
