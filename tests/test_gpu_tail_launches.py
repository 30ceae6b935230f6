"""The looped form of the plain k_s2m_iterate (k_s2m_iterate_tail, lio-slam_amd/csrc/lio_tail.hip): from launch LIO_TAIL_FROM of
a run on, a fixed grid of LIO_TAIL_WGS workgroups loops over the live entries of the block list instead of one workgroup per
entry.  It runs the same body on the same entries, so everything observable must be the same BYTES as with LIO_TAIL_FROM=-1
(never looped): poses and every field of every lio_s2m_result, whatever the grid, the first looped launch, the list length
(not a multiple of 8, shorter than 8, shorter than the grid), eagerly and from a captured graph, on a first and on a second
run of a handle.  Handles that record associations, stamp the phase clock or run a corner batch never take it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_TOL_T = 1e-5   # metres   (tests/test_gpu_parity.py)
POSE_TOL_R = 1e-6   # radians
SWITCHES = ("LIO_TAIL_FROM", "LIO_TAIL_WGS")


def _handle(pkg, tail_from, tail_wgs=None, **cfg):
    """A launch-loop handle (pipeline=1) created under LIO_TAIL_FROM / LIO_TAIL_WGS (None: not set, the library's default)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k, v in zip(SWITCHES, (tail_from, tail_wgs)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        return pkg.ScanToMap(pipeline=1, **cfg)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _spread(scan, n):
    """n points spread over the whole scan (a prefix would be one ring)."""
    sub = np.ascontiguousarray(scan[:: len(scan) // n][:n])
    assert len(sub) == n
    return sub


def _n_blocks(scans):
    return sum((len(s) + 255) // 256 for s in scans)


def _run(s2m, scans, poses0):
    s2m.batch_upload(scans); s2m.batch_set_poses(poses0); s2m.batch_run()
    poses, res = s2m.batch_results()
    return poses.tobytes(), bytes(res), poses, list(res)


def _two_runs(pkg, map_xyz, scans, poses0, tail_from, tail_wgs=None, **cfg):
    """First and second run of one handle, and the launch forms of the second: ((first, second), (full, looped))."""
    s2m = _handle(pkg, tail_from, tail_wgs, **cfg)
    s2m.set_map(map_xyz)
    first = _run(s2m, scans, poses0)
    second = _run(s2m, scans, poses0)                           # (the state of the first run, matP included, is still in place)
    forms = s2m.launch_forms()
    assert s2m.kernel_variant()[0] is True
    s2m.close()
    return (first, second), forms


def _assert_equal(got, ref, what):
    for run in (0, 1):
        assert got[run][0] == ref[run][0], f"poses differ ({what}, run {run})"
        assert got[run][1] == ref[run][1], f"results differ ({what}, run {run})"


@pytest.fixture(scope="module")
def ragged(small_case):
    """The ragged batch of test_gpu_plain_kernel.py, then copies under other initial poses: more than 8 scans, so that
    batch_set_poses re-orders the block list, and a block count that is no multiple of 8."""
    qs = small_case["queries"]
    far = qs[0]["scan"] + np.float32(500.0)                      # nowhere near the map: no point finds a plane, MO:1721-1724
    scans = [_spread(qs[0]["scan"], 20), _spread(qs[1]["scan"], 31), _spread(qs[2]["scan"], 256), _spread(qs[1]["scan"], 257),
             _spread(qs[0]["scan"], 700), np.ascontiguousarray(far[:900]), qs[2]["scan"], qs[1]["scan"]]
    poses0 = [qs[k]["pose_init"] for k in (0, 1, 2, 1, 0, 0, 2, 1)]
    rng = np.random.default_rng(5)
    for k in (2, 0, 1):                                          # copies that start elsewhere: other iteration counts, other places in the list
        d = np.concatenate([rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.15, 0.15, 3)]).astype(np.float32)
        scans.append(qs[k]["scan"]); poses0.append(qs[k]["pose_init"] + d)
        scans.append(_spread(qs[k]["scan"], 700)); poses0.append(qs[k]["pose_true"])
    while _n_blocks(scans) % 8 == 0:
        scans.append(_spread(qs[0]["scan"], 31)); poses0.append(qs[0]["pose_init"])
    assert len(scans) > 8 and _n_blocks(scans) % 8 != 0
    return scans, np.stack(poses0).astype(np.float32)


GRAPH_CFGS = {0: dict(use_graph=0), 1: dict(use_graph=1, graph_iters=4)}


@pytest.fixture(scope="module")
def reference(pkg, small_case, ragged):
    """The ragged batch with LIO_TAIL_FROM=-1, launch by launch and from a graph: {use_graph: (first, second)}."""
    out = {}
    for ug, cfg in GRAPH_CFGS.items():
        out[ug], forms = _two_runs(pkg, small_case["map"], *ragged, -1, None, max_iters=30, **cfg)
        assert forms[1] == 0 and forms[0] > 0                    # the reference never loops
    assert out[0][0][:2] == out[1][0][:2]
    res = out[0][0][3]
    assert res[0].status == 1 and res[0].iters == 0 and res[5].status == 2
    assert len({r.iters for r in res}) >= 3                      # the scans stop at different iterations
    return out


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("tail_wgs", [8, 16, None])
@pytest.mark.parametrize("tail_from", [0, 1, 3])
def test_looped_equals_full_grid_on_a_ragged_batch(pkg, small_case, ragged, reference, tail_from, tail_wgs, use_graph):
    got, (full, looped) = _two_runs(pkg, small_case["map"], *ragged, tail_from, tail_wgs, max_iters=30, **GRAPH_CFGS[use_graph])
    _assert_equal(got, reference[use_graph], f"from {tail_from}, {tail_wgs} workgroups, graph {use_graph}")
    assert looped > 0                                            # (with 8 workgroups every one of them loops over several entries)
    if use_graph:
        assert full == tail_from * ((full + looped) // 4)        # by position in the chunk of 4, in every unit
    else:
        assert full == tail_from


def test_lists_shorter_than_8_and_shorter_than_the_grid(pkg, small_case):
    qs = small_case["queries"]
    tiny = [_spread(qs[1]["scan"], 31), _spread(qs[2]["scan"], 257)]                       # 3 blocks
    short = [_spread(qs[0]["scan"], 700), _spread(qs[1]["scan"], 1100), _spread(qs[2]["scan"], 300)]   # 10 blocks
    for scans, ks, wgs in ((tiny, (1, 2), (8, None)), (short, (0, 1, 2), (16, None))):
        assert _n_blocks(scans) < (wgs[0] if scans is short else 8)
        poses0 = np.stack([qs[k]["pose_init"] for k in ks])
        ref, forms = _two_runs(pkg, small_case["map"], scans, poses0, -1, None, max_iters=30, use_graph=0)
        assert forms[1] == 0
        for w in wgs:
            got, forms = _two_runs(pkg, small_case["map"], scans, poses0, 0, w, max_iters=30, use_graph=0)
            _assert_equal(got, ref, f"{_n_blocks(scans)} blocks, {w} workgroups")
            assert forms[0] == 0 and forms[1] > 0
            assert all(r.iters > 0 for r in got[0][3])


def test_looped_launches_after_every_scan_has_finished_change_nothing(pkg, small_case, ragged, reference):
    """One graph of 30 launches, looped from launch 12 on, started at the poses the reference converged to: every scan has
    finished long before, the 18 looped launches find *n_active == 0."""
    scans, _ = ragged
    poses0 = np.ascontiguousarray(reference[0][0][2])
    cfg = dict(max_iters=30, use_graph=1, graph_iters=30)
    ref, forms = _two_runs(pkg, small_case["map"], scans, poses0, -1, None, **cfg)
    assert forms == (30, 0)
    assert max(r.iters for r in ref[0][3] if r.status == 0) < 12
    got, forms = _two_runs(pkg, small_case["map"], scans, poses0, 12, None, **cfg)
    assert forms == (12, 18)
    _assert_equal(got, ref, "all finished before the first looped launch")


def test_a_scan_that_iterates_to_the_last_launch_over_several_units(pkg, small_case, ragged):
    """Convergence thresholds nothing meets: every accepted scan with enough correspondences runs all 30 iterations, 8 units
    of a 4-launch graph; the refused and the starved scan are dead entries in every looped launch."""
    cfg = dict(max_iters=30, use_graph=1, graph_iters=4, conv_deg=0.0, conv_cm=0.0)
    ref, _ = _two_runs(pkg, small_case["map"], *ragged, -1, None, **cfg)
    assert max(r.iters for r in ref[0][3]) == 30 and ref[0][3][0].iters == 0
    for tail_from, tail_wgs in ((1, 8), (3, None)):
        got, (full, looped) = _two_runs(pkg, small_case["map"], *ragged, tail_from, tail_wgs, **cfg)
        assert (full, looped) == (8 * tail_from, 8 * (4 - tail_from))
        _assert_equal(got, ref, f"30 iterations, from {tail_from}")


def test_looped_equals_full_grid_on_a_degenerate_corridor(pkg, synth):
    case = synth.make_case("vlp16", n_keyframes=5, seed=3, kind="corridor", device="cpu")
    q = case["queries"][0]
    scans, poses0 = [q["scan"], _spread(q["scan"], 700)], np.stack([q["pose_init"]] * 2)
    for cfg in GRAPH_CFGS.values():
        ref, _ = _two_runs(pkg, case["map"], scans, poses0, -1, None, max_iters=30, **cfg)
        assert ref[0][3][0].is_degenerate == 1
        got, forms = _two_runs(pkg, case["map"], scans, poses0, 0, 8, max_iters=30, **cfg)
        assert forms[0] == 0 and forms[1] > 0
        _assert_equal(got, ref, f"corridor {cfg}")
        assert got[0][3][0].is_degenerate == 1


@pytest.mark.parametrize("cfg", [dict(record_corr_iter=0), dict(profile=2)])
def test_recording_and_stamping_handles_never_loop(pkg, small_case, ragged, reference, cfg):
    s2m = _handle(pkg, 0, 8, max_iters=30, **cfg)
    s2m.set_map(small_case["map"])
    out = _run(s2m, *ragged)
    assert s2m.kernel_variant() == (False, 5)
    full, looped = s2m.launch_forms()
    assert looped == 0 and full > 0
    assert out[:2] == reference[0][0][:2]
    s2m.close()


def test_a_corner_batch_never_loops(pkg, synth, small_case):
    case = synth.add_corners(dict(small_case, queries=[dict(q) for q in small_case["queries"]]), "vlp16", seed=11)
    qs = case["queries"][:2]
    poses0 = np.stack([q["pose_init"] for q in qs])
    outs = []
    for tail_from in (-1, 0):
        s2m = _handle(pkg, tail_from, 8, max_iters=30)
        s2m.set_map(case["map"])
        s2m.set_corner_map(case["corner_map"])
        s2m.batch_upload([q["scan"] for q in qs])
        s2m.batch_upload_corners([q["corners"] for q in qs])
        s2m.batch_set_poses(poses0)
        s2m.batch_run()
        poses, res = s2m.batch_results()
        assert s2m.kernel_variant() == (False, 5)
        full, looped = s2m.launch_forms()
        assert looped == 0 and full > 0
        outs.append((poses.tobytes(), bytes(res)))
        s2m.close()
    assert outs[0] == outs[1]


def test_looped_poses_match_the_oracle(pkg, oracle, small_case, ragged):
    scans, poses0 = ragged[0][:8], ragged[1][:8]
    s2m = _handle(pkg, 0, 8, max_iters=30, use_graph=0)
    s2m.set_map(small_case["map"])
    _, _, poses, res = _run(s2m, scans, poses0)
    full, looped = s2m.launch_forms()
    assert full == 0 and looped > 0
    s2m.close()
    ocfg = oracle.default_config(knn_mode=1, n_threads=8)
    for i, (scan, p0) in enumerate(zip(scans, poses0)):
        pose_o, res_o, _, _ = oracle.scan2map(ocfg, scan, small_case["map"], p0)
        assert res[i].status == res_o.status and res[i].iters == res_o.iters, i
        assert np.abs(poses[i][3:] - pose_o[3:]).max() <= POSE_TOL_T, i
        assert np.abs(poses[i][:3] - pose_o[:3]).max() <= POSE_TOL_R, i
