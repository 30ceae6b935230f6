"""The plain instantiation of k_s2m_iterate (lio-slam_amd/csrc/lio_kernels.hip): the batch path of one device with map
sharding, the association record and the phase clock folded away at compile time.  It executes the same arithmetic as the
general instantiation, so everything observable must be the same BYTES: poses and every field of every lio_s2m_result, on
a ragged batch (a refused scan, the smallest accepted one, exactly one workgroup, a one-point workgroup, a partial last
workgroup, a scan that finds no plane), on a degenerate corridor, eagerly and from a captured graph, on a first and on a
second run of a handle.  LIO_PLAIN_KERNEL=0 in the environment when a handle is created keeps the general instantiation;
handles that record associations, stamp the phase clock, hold a shard plan or run a corner batch never get the plain one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_TOL_T = 1e-5   # metres   (tests/test_gpu_parity.py)
POSE_TOL_R = 1e-6   # radians


def _handle(pkg, plain=True, **cfg):
    """A launch-loop handle (pipeline=1: the one-launch loop of small batches is another kernel); plain=False: created
    under LIO_PLAIN_KERNEL=0."""
    old = os.environ.get("LIO_PLAIN_KERNEL")
    try:
        if plain:
            os.environ.pop("LIO_PLAIN_KERNEL", None)
        else:
            os.environ["LIO_PLAIN_KERNEL"] = "0"
        return pkg.ScanToMap(pipeline=1, **cfg)
    finally:
        if old is None:
            os.environ.pop("LIO_PLAIN_KERNEL", None)
        else:
            os.environ["LIO_PLAIN_KERNEL"] = old


def _spread(scan, n):
    """n points spread over the whole scan (a prefix would be one ring)."""
    sub = np.ascontiguousarray(scan[:: len(scan) // n][:n])
    assert len(sub) == n
    return sub


def _run(s2m, scans, poses0):
    s2m.batch_upload(scans); s2m.batch_set_poses(poses0); s2m.batch_run()
    poses, res = s2m.batch_results()
    return poses.tobytes(), bytes(res), poses, list(res)


@pytest.fixture(scope="module")
def ragged(small_case):
    qs = small_case["queries"]
    far = qs[0]["scan"] + np.float32(500.0)                      # nowhere near the map: no point finds a plane, MO:1721-1724
    scans = [_spread(qs[0]["scan"], 20), _spread(qs[1]["scan"], 31), _spread(qs[2]["scan"], 256), _spread(qs[1]["scan"], 257),
             _spread(qs[0]["scan"], 700), np.ascontiguousarray(far[:900]), qs[2]["scan"], qs[1]["scan"]]
    poses0 = np.stack([qs[k]["pose_init"] for k in (0, 1, 2, 1, 0, 0, 2, 1)])
    return scans, poses0


@pytest.fixture(scope="module")
def plain_eager(pkg, small_case, ragged):
    """The ragged batch through a plain handle, launch by launch: (pose bytes, result bytes, poses, results)."""
    s2m = _handle(pkg, True, use_graph=0, max_iters=30)
    s2m.set_map(small_case["map"])
    out = _run(s2m, *ragged)
    assert s2m.kernel_variant()[0] is True
    s2m.close()
    return out


def _plain_equals_general(pkg, map_xyz, scans, poses0):
    outs = []
    for cfg in (dict(use_graph=0), dict(use_graph=1, graph_iters=4)):
        both = []
        for plain in (True, False):
            s2m = _handle(pkg, plain, max_iters=30, **cfg)
            s2m.set_map(map_xyz)
            first = _run(s2m, scans, poses0)
            is_plain, waves = s2m.kernel_variant()
            assert is_plain is plain and waves in (5, 6)
            second = _run(s2m, scans, poses0)                   # (the state of the first run, matP included, is still in place)
            assert s2m.kernel_variant()[0] is plain
            s2m.close()
            both.append((first, second))
        for run in (0, 1):
            assert both[0][run][0] == both[1][run][0], f"poses differ ({cfg}, run {run})"
            assert both[0][run][1] == both[1][run][1], f"results differ ({cfg}, run {run})"
        assert both[0][0][:2] == both[0][1][:2]                  # and a run is reproducible
        outs.append(both[0][0])
    assert outs[0][:2] == outs[1][:2]                            # eager launches == graph replays
    return outs[0]


def test_plain_equals_general_on_a_ragged_batch(pkg, small_case, ragged, plain_eager):
    out = _plain_equals_general(pkg, small_case["map"], *ragged)
    assert out[:2] == plain_eager[:2]
    res = out[3]
    assert res[0].status == 1 and res[0].iters == 0                          # 20 points: refused (N_s <= 30, MO:1844)
    assert res[1].status != 1 and res[1].iters > 0                           # 31 points: the smallest accepted scan
    assert res[5].status == 2 and res[5].n_corr_last < 50                    # starved
    assert all(r.status == 0 for r in res[6:])
    assert len({r.iters for r in res}) >= 3                                  # the scans stop at different iterations


def test_plain_equals_general_on_a_degenerate_corridor(pkg, synth):
    case = synth.make_case("vlp16", n_keyframes=5, seed=3, kind="corridor", device="cpu")
    q = case["queries"][0]
    out = _plain_equals_general(pkg, case["map"], [q["scan"], _spread(q["scan"], 700)], np.stack([q["pose_init"]] * 2))
    assert out[3][0].is_degenerate == 1


def test_plain_poses_match_the_oracle(oracle, small_case, ragged, plain_eager):
    scans, poses0 = ragged
    _, _, poses, res = plain_eager
    ocfg = oracle.default_config(knn_mode=1, n_threads=8)
    for i, (scan, p0) in enumerate(zip(scans, poses0)):
        pose_o, res_o, _, _ = oracle.scan2map(ocfg, scan, small_case["map"], p0)
        assert res[i].status == res_o.status and res[i].iters == res_o.iters, i
        assert np.abs(poses[i][3:] - pose_o[3:]).max() <= POSE_TOL_T, i
        assert np.abs(poses[i][:3] - pose_o[:3]).max() <= POSE_TOL_R, i


@pytest.mark.parametrize("cfg", [dict(record_corr_iter=0), dict(record_corr_iter=2), dict(profile=2)])
def test_recording_and_stamping_handles_keep_the_general_kernel(pkg, oracle, small_case, ragged, plain_eager, cfg):
    scans, poses0 = ragged
    s2m = _handle(pkg, True, max_iters=30, **cfg)
    s2m.set_map(small_case["map"])
    out = _run(s2m, scans, poses0)
    assert s2m.kernel_variant() == (False, 5)
    assert out[:2] == plain_eager[:2]                            # neither changes a result
    if "record_corr_iter" in cfg:
        # the association recorded at that iteration is the exact one at the pose the plain handle had there
        it = cfg["record_corr_iter"]
        ocfg = oracle.default_config(knn_mode=1, n_threads=8)
        for i in (4, 6):
            assert plain_eager[3][i].iters > it
            pose_at = poses0[i] if it == 0 else np.array(plain_eager[3][i].pose_iter[it - 1], np.float32)
            flag, coeff, nn = s2m.get_correspondences(i)
            fo, co, no = oracle.surf_optimization(ocfg, pose_at, scans[i], small_case["map"])
            assert np.array_equal(flag, fo) and np.array_equal(nn, no)
            assert np.array_equal(coeff[flag == 1].view(np.uint32), co[fo == 1].view(np.uint32))
    s2m.close()


def test_a_shard_plan_keeps_the_general_kernel(pkg, small_case, ragged, plain_eager):
    """Two slabs of the map on two handles of the one GPU; the sums are added as the all-reduce would."""
    import importlib
    import torch
    mg = importlib.import_module("lio-slam_amd.multigpu")
    scans, poses0 = ragged
    map_xyz = small_case["map"]
    plan = mg.plan_shards(map_xyz, 2, cell=mg.default_cell())
    hs, sums = [], []
    for r in range(2):
        h = _handle(pkg, True, max_iters=30)
        h.set_map(np.ascontiguousarray(map_xyz[mg.shard_points(map_xyz, plan, r, 16)]))
        h.set_global_grid([float(v) for v in plan["origin"]], [int(v) for v in plan["dims"]])
        h.set_shard_plan(plan["axis"], r, [int(v) for v in plan["bounds"]], 16)
        h.batch_upload(scans); h.batch_set_poses(poses0)
        h.batch_begin()
        hs.append(h)
        sums.append(torch.zeros((len(scans), 32), dtype=torch.float64, device="cuda"))
    for it in range(30):
        for h, s in zip(hs, sums):
            h.batch_iter_partial(s.data_ptr())
        for h in hs:
            h.batch_sync()
        total = sums[0] + sums[1]
        torch.cuda.synchronize()
        for h in hs:
            h.batch_iter_apply(total.data_ptr())
        if hs[0].batch_n_active() == 0:
            break
    _, _, ref_poses, ref_res = plain_eager
    for h in hs:
        assert h.kernel_variant() == (False, 5)
        p, r = h.batch_results()
        assert [x.iters for x in r] == [x.iters for x in ref_res]
        assert [x.status for x in r] == [x.status for x in ref_res]
        np.testing.assert_allclose(p[:, 3:], ref_poses[:, 3:], atol=POSE_TOL_T)      # (tests/test_gpu_sharded.py)
        np.testing.assert_allclose(p[:, :3], ref_poses[:, :3], atol=POSE_TOL_R)
        h.close()


def test_a_corner_batch_keeps_the_general_kernel(pkg, oracle, synth, small_case):
    case = synth.add_corners(dict(small_case, queries=[dict(q) for q in small_case["queries"]]), "vlp16", seed=11)
    qs = case["queries"][:2]
    poses0 = np.stack([q["pose_init"] for q in qs])
    ocfg = oracle.default_config(knn_mode=1, n_threads=8)
    s2m = _handle(pkg, True, max_iters=30)
    s2m.set_map(case["map"])
    s2m.set_corner_map(case["corner_map"])
    s2m.batch_upload([q["scan"] for q in qs])
    s2m.batch_upload_corners([q["corners"] for q in qs])
    s2m.batch_set_poses(poses0)
    s2m.batch_run()
    poses, res = s2m.batch_results()
    assert s2m.kernel_variant() == (False, 5)
    for i, q in enumerate(qs):
        po, ro, _, _ = oracle.scan2map_cs(ocfg, q["corners"], case["corner_map"], q["scan"], case["map"], q["pose_init"])
        assert res[i].iters == ro.iters and list(res[i].n_corr_iter)[:ro.iters] == list(ro.n_corr_iter)[:ro.iters]
        assert np.abs(poses[i][3:] - po[3:]).max() <= 1e-5 and np.abs(poses[i][:3] - po[:3]).max() <= 1e-6   # (tests/test_gpu_corner.py)
    # a surf-only batch uploaded afterwards is the plain path again
    s2m.batch_upload([q["scan"] for q in qs]); s2m.batch_set_poses(poses0); s2m.batch_run()
    poses, res = s2m.batch_results()
    assert s2m.kernel_variant()[0] is True
    for i, q in enumerate(qs):
        po, ro = oracle.scan2map(ocfg, q["scan"], case["map"], q["pose_init"])[:2]
        assert res[i].iters == ro.iters
        assert np.abs(poses[i][3:] - po[3:]).max() <= POSE_TOL_T and np.abs(poses[i][:3] - po[:3]).max() <= POSE_TOL_R
    s2m.close()
