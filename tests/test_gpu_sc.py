"""Scan Context loop detection on the device (lio_sc.hip) against the numpy restatement (tests/sc_restate.py).

Where the bands come from.  Host and device share every operation of the descriptor bit for bit (IEEE +, *, /, sqrt, fp64
ceil) but one: the fp32 atan, which differs between libms by a few ulp, about 2e-7 rad.  Rounding an angle of up to 360
degrees to float adds 3e-5 degrees; together below 1e-5 sector units.  A point whose sector coordinate u_s lies within 1e-4
of an integer (tenfold margin) may therefore fall on either side; the ring coordinate is exact and gets the same band for
simplicity, as does 1e-3 m around max_radius.  Such points are `boundary-near`: the exact tests remove them (about 4e-4 of
a sweep, asserted below 1 %), the whole-cloud test brackets what they may do.

The synth sensors fire their columns at exact multiples of 360 / 1800 (or 360 / 1024) degrees, so in the sensor frame every
30th column of a 1800-column sweep sits exactly on a sector boundary: 3.3 % of the points.  A node hands Scan Context the
deskewed cloud in the base frame, behind the lidar-to-base extrinsic rotation; the sweeps here are turned by a mounting yaw
of 1.3 degrees (6.5 columns) for the same reason, which leaves the share expected of points in general position.  One
sweep is also bracketed as it leaves the sensor, boundaries included.

Distances: fp64 sums of at most 60 terms of magnitude <= 1 round to ~1e-14; the bound is 1e-12.  An argmin is only pinned
when its runner-up is further than that rounding: pairs / shifts closer than 1e-9 are left out, and at least 90 % stay."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sc_restate as R   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [("vlp16", "street"), ("vlp16", "corridor"), ("hdl64", "street"), ("hdl64", "corridor")]
MOUNT_YAW = np.radians(1.3)
_SWEEPS = {}


def sweep(synth, sensor, kind, k=3, seed=500, yaw=0.0, mount=MOUNT_YAW):
    """One sweep from keyframe pose k (the sensor turned by `yaw` more), in the base frame: the sensor frame turned by `mount`."""
    key = (sensor, kind, k, seed, yaw, mount)
    if key not in _SWEEPS:
        boxes = synth.make_scene(21, length=120.0, kind=kind)
        pose = synth.keyframe_poses(60, spacing=2.0, seed=21)[k].copy()
        pose[2] += yaw
        xyz = synth.cast_scan(boxes, pose, sensor, seed=seed, device="cpu")["xyz"].astype(np.float64)
        c, s = np.cos(mount), np.sin(mount)
        _SWEEPS[key] = (xyz @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])).astype(np.float32)
    return _SWEEPS[key]


def pinned_part(xyz, **cfg):
    """The cloud without its boundary-near points, and the share that was removed."""
    g = {**R.DEFAULTS, **cfg}
    c = R.coords(xyz, **g)
    nb = R.boundary_near(c, **g)
    return np.ascontiguousarray(xyz[~nb]), float(nb.sum()) / len(xyz)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def check_triplet(got, desc):
    same_bits(got[0], desc)
    same_bits(got[1], R.ring_key(desc))
    same_bits(got[2], R.sector_key(desc))


def random_cloud(seed, n=3000, reach=70.0):
    rng = np.random.default_rng(seed)
    r, a = rng.uniform(0.5, reach, n), rng.uniform(0, 2 * np.pi, n)
    xyz = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.8, 8.0, n)], 1).astype(np.float32)
    return pinned_part(xyz)[0]


def xyzi_records(xyz):
    rec = np.zeros((len(xyz), 8), np.float32)
    rec[:, :3], rec[:, 3] = xyz, 1.0
    return rec


# ---------------------------------------------------------------------------------------------------------- descriptor
@pytest.mark.parametrize("sensor,kind", CASES)
def test_descriptor_and_keys_equal_the_restatement_bit_for_bit_by_every_route(pkg, synth, small_case, sensor, kind):
    xyz, share = pinned_part(sweep(synth, sensor, kind))
    print(f"{sensor} {kind}: {len(xyz)} points, boundary-near share {share:.2e}")
    assert share < 0.01
    desc = R.make_desc(xyz)
    assert np.count_nonzero(desc) > 60
    check_triplet(pkg.sc_make(xyz), desc)                                         # lio_sc_make, stride 12
    st = pkg.KeyframeStore()
    a = st.sc_add(xyzi_records(xyz))                                              # host records, stride 32
    dev = pkg.DeviceBuffer(np.concatenate([xyz, np.ones((len(xyz), 1), np.float32)], 1))
    b = st.sc_add_device(dev.ptr, len(xyz), 16)
    dev.close()
    h = pkg.ScanToMap()
    h.set_map(small_case["map"])
    lay = pkg.PC2Layout(point_step=32, off_x=0, off_intensity=16, off_ring=-1, off_time=-1)
    with pytest.raises(pkg.LioError, match="staged"):
        st.sc_add_from_handle(h)                                                  # nothing staged yet
    h.downsampleAndScan2MapOptimization(xyzi_records(xyz), len(xyz), lay, 0.4, small_case["queries"][0]["pose_init"])
    c = st.sc_add_from_handle(h)                                                  # the staged blob, no copy
    assert (a, b, c) == (0, 1, 2) and st.sc_count() == 3 and len(st) == 0
    for k in (a, b, c):
        check_triplet(st.sc_get(k), desc)
    h.close(); st.close()


def boundary_cloud():
    """Points that sit on cell boundaries: the axes, ranges of exactly 4 k metres, 80 m, sector boundaries; with points the
    build skips (non-finite, on the z axis) and a few ordinary ones."""
    rng = np.random.default_rng(77)
    pts = []
    for r in (0.5, 4.0, 8.0, 13.0, 40.0, 76.0, 80.0):
        for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            pts.append([r * dx, r * dy, rng.uniform(-1, 5)])
    for k in range(1, 21):                                                        # range 4 k at assorted angles
        for a in rng.uniform(0, 2 * np.pi, 6):
            pts.append([4.0 * k * np.cos(a), 4.0 * k * np.sin(a), rng.uniform(-1, 5)])
    for j in range(60):                                                           # the sector boundaries, some at 80 m
        a = np.radians(6.0 * j)
        for r in (3.0, 22.0, 80.0, 80.0005, 79.9995):
            pts.append([r * np.cos(a), r * np.sin(a), rng.uniform(-1, 5)])
    pts += [[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [0, 0, 50.0], [-0.0, 0.0, 60.0], [30, 30, -1.9], [-20, 5, -2.5]]
    more = rng.uniform(-60, 60, (500, 3)); more[:, 2] = rng.uniform(-1.8, 6, 500)
    return np.concatenate([np.array(pts, np.float64), more]).astype(np.float32)


@pytest.mark.parametrize("which", ["vlp16-street", "vlp16-corridor", "hdl64-street", "hdl64-corridor", "sensor-frame", "boundaries"])
def test_whole_cloud_descriptor_lies_between_the_bounds(pkg, synth, which):
    if which == "boundaries":
        xyz = boundary_cloud()
    elif which == "sensor-frame":
        xyz = sweep(synth, "vlp16", "street", mount=0.0)                          # every 30th column on a sector boundary
    else:
        xyz = sweep(synth, *which.split("-"))
    lo, hi, share = R.desc_bounds(xyz)
    dev = pkg.sc_make(xyz)[0]
    loose = int(np.count_nonzero(lo != hi))
    print(f"{which}: boundary-near share {share:.2e}, cells with lo != hi: {loose}, device == lo in {int((dev == lo).sum())} of {lo.size}")
    if which in ("boundaries", "sensor-frame"):
        assert share > (0.3 if which == "boundaries" else 0.03) and loose > 20    # the cloud does sit on boundaries
    bad = np.argwhere(~((lo <= dev) & (dev <= hi)))
    assert len(bad) == 0, [(tuple(i), lo[tuple(i)], dev[tuple(i)], hi[tuple(i)]) for i in bad[:5]]


def test_empty_and_skipped_only_clouds_give_zero(pkg):
    for cloud in (np.zeros((0, 3), np.float32), np.array([[np.nan, 0, 0], [0, 0, 3], [200, 0, 1]], np.float32)):
        d, rk, sk = pkg.sc_make(cloud)
        assert not d.any() and not rk.any() and not sk.any()
    st = pkg.KeyframeStore()
    assert st.sc_add(np.zeros((0, 3), np.float32)) == 0 and not st.sc_get(0)[0].any()
    st.close()


# ------------------------------------------------------------------------------------------------------- distance hook
def test_distance_hook_equals_the_restatement(pkg, synth):
    descs = [R.make_desc(sweep(synth, "vlp16", "street", k=k, seed=600 + k)) for k in (2, 9, 20, 33)]
    descs.append(R.make_desc(sweep(synth, "hdl64", "corridor")))
    descs += [R.make_desc(random_cloud(s)) for s in (1, 2)]
    pairs = [(a, np.roll(a, k, axis=1)) for a in descs for k in (0, 1, 17, 30, 59)]
    pairs += [(descs[i], descs[j]) for i in range(len(descs)) for j in range(len(descs)) if i != j]
    kept = 0
    worst = 0.0
    for a, b in pairs:
        d_ref, al_ref, info = R.distance(a, b)
        if not R.runner_up_gap(info) > 1e-9:
            continue
        kept += 1
        d, al = pkg.sc_distance(a, b)
        assert al == al_ref
        worst = max(worst, abs(d - d_ref))
        assert abs(d - d_ref) <= 1e-12, (d, d_ref)
    print(f"distance hook: kept {kept} of {len(pairs)} pairs, worst |dist - restatement| = {worst:.2e}")
    assert kept >= 0.9 * len(pairs)
    # an empty descriptor shares no column with anything: every shift is NaN, the initial 1e7 and align 0 stay
    empty = np.zeros((20, 60), np.float32)
    for a, b in ((descs[0], empty), (empty, descs[0]), (empty, empty)):
        assert pkg.sc_distance(a, b) == (10000000.0, 0) and R.distance(a, b)[:2] == (10000000.0, 0)
    # a wider search and another geometry
    cfg = pkg.sc_default_config(search_ratio=1.0)
    d_ref, al_ref, info = R.distance(descs[0], np.roll(descs[1], 11, axis=1), search_ratio=1.0)
    assert len(info["shifts"]) == 60
    d, al = pkg.sc_distance(descs[0], np.roll(descs[1], 11, axis=1), cfg)
    assert al == al_ref and abs(d - d_ref) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ detection
def compare_detection(res, out):
    n = res.n_candidates
    assert res.n_searched == out["n_searched"] and n == len(out["cand_idx"])
    assert list(res.cand_idx[:n]) == out["cand_idx"]
    same_bits(np.array(res.cand_ring_d2[:n], np.float32), np.array(out["cand_d2"], np.float32))
    assert list(res.cand_align[:n]) == out["cand_align"]
    for a, b in zip(res.cand_dist[:n], out["cand_dist"]):
        assert abs(a - b) <= 1e-12, (a, b)
    assert (res.nn_idx, res.loop_id, res.align) == (out["nn_idx"], out["loop_id"], out["align"])
    assert abs(res.min_dist - out["min_dist"]) <= 1e-12
    same_bits(np.float32(res.yaw_diff_rad).reshape(1), np.float32(out["yaw"]).reshape(1))


def test_detection_finds_the_revisited_keyframe_and_its_yaw(pkg, synth):
    n_kf, revisit, turn = 40, 5, 7
    clouds = [pinned_part(sweep(synth, "vlp16", "street", k=k, seed=700 + k))[0] for k in range(n_kf)]
    # one more sweep from keyframe 5's place with the sensor turned by 7 sectors (210 of the 1800 columns: the same rays)
    clouds.append(pinned_part(sweep(synth, "vlp16", "street", k=revisit, seed=999, yaw=np.radians(turn * 6.0)))[0])
    st, m = pkg.KeyframeStore(), R.Manager()
    for c in clouds:
        st.sc_add(c)
        m.add(R.make_desc(c))
    for k in (0, revisit, n_kf):
        check_triplet(st.sc_get(k), m.descs[k])
    out = m.detect()
    res = st.sc_detect()
    print(f"detection: searched {res.n_searched}, candidates {list(res.cand_idx[:res.n_candidates])}, ring d2 "
          f"{[float(v) for v in out['d2_sorted'][:5]]}, dists {list(res.cand_dist[:res.n_candidates])}, gaps {out['gaps']}")
    assert out["n_searched"] == n_kf + 1 - 30 and out["d2_sorted"][2] != out["d2_sorted"][3]   # the third candidate is pinned
    assert min(out["gaps"]) > 1e-9                                                             # and so is every argmin
    compare_detection(res, out)
    assert res.loop_id == revisit
    # the sensor turned by +7 sectors sees the scene turned by -7: the old descriptor matches after a shift of 60 - 7
    assert res.align == 60 - turn and abs(float(res.yaw_diff_rad) - np.radians((60 - turn) * 6.0)) < 1e-6
    # a threshold that rejects: the same best candidate, no loop
    res2 = st.sc_detect(pkg.sc_default_config(dist_thres=res.min_dist))                        # strict <
    assert res2.loop_id == -1 and res2.nn_idx == revisit and res2.min_dist == res.min_dist
    st.close()


def test_prefix_goes_stale_within_the_period_and_is_refreshed_past_it(pkg):
    over = dict(num_exclude_recent=3, tree_period=3, num_candidates=2)
    cfg = pkg.sc_default_config(**over)
    st, m = pkg.KeyframeStore(), R.Manager(**over)
    seen = []
    for k in range(11):
        c = random_cloud(40 + k, n=800)
        st.sc_add(c); m.add(R.make_desc(c))
        res, out = st.sc_detect(cfg), m.detect()
        if k < 3:                                                                 # fewer than num_exclude_recent + 1
            assert (res.loop_id, res.yaw_diff_rad, res.n_searched, res.n_candidates, res.min_dist) == (-1, 0.0, 0, 0, 10000000.0)
            assert out["loop_id"] == -1 and m.counter == 0
            continue
        compare_detection(res, out)
        seen.append(res.n_searched)
    assert seen == [1, 1, 1, 4, 4, 4, 7, 7]                                      # rebuilt on calls 0, 3, 6 of those that got that far
    # more candidates asked for than the prefix holds: only those are evaluated
    over2 = dict(num_exclude_recent=9, tree_period=1, num_candidates=16)
    res = st.sc_detect(pkg.sc_default_config(**over2))
    m.counter = 0
    out = m.detect(**over2)
    assert res.n_searched == 2 and res.n_candidates == 2
    compare_detection(res, out)
    st.close()


def test_another_geometry_and_what_is_refused(pkg, synth):
    import torch
    over = dict(num_rings=10, num_sectors=30, max_radius=50.0, lidar_height=1.5, num_exclude_recent=2, num_candidates=3, search_ratio=0.2)
    cfg = pkg.sc_default_config(**over)
    st, m = pkg.KeyframeStore(), R.Manager(**over)
    assert st.sc_geometry() == (0, 0)
    for k in range(8):
        c = pinned_part(random_cloud(60 + k if k < 7 else 61, n=1500), **over)[0]    # the last one repeats keyframe 1
        st.sc_add(c, cfg); m.add(R.make_desc(c, **over))
        check_triplet(st.sc_get(k), m.descs[k])                                   # (sized by the store's geometry, not the default)
    assert st.sc_geometry() == (10, 30)
    check_triplet(pkg.sc_make(c, cfg), m.descs[-1])
    res, out = st.sc_detect(cfg), m.detect()
    compare_detection(res, out)
    assert res.loop_id == 1 and res.align == 0 and res.min_dist < 1e-12
    # the geometry of the first descriptor holds for the store; NULL means that geometry
    with pytest.raises(pkg.LioError, match="geometry"):
        st.sc_add(c, pkg.sc_default_config())
    assert st.sc_add(c) == 8 and st.sc_count() == 9
    check_triplet(st.sc_get(8), m.descs[-1])
    with pytest.raises(pkg.LioError, match="num_rings"):
        st.sc_detect(pkg.sc_default_config())
    for field, v in (("num_candidates", 17), ("num_candidates", 0), ("tree_period", 0), ("search_ratio", 2.0), ("num_exclude_recent", -1)):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.sc_detect(pkg.sc_default_config(**{**over, field: v}))
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        st.sc_add(c, pkg.sc_default_config(num_rings=100, num_sectors=100))
    with pytest.raises(pkg.LioError, match="no such descriptor"):
        st.sc_get(9)
    dev = pkg.DeviceBuffer(np.concatenate([c, np.ones((len(c), 1), np.float32)], 1))
    with pytest.raises(pkg.LioError, match="aligned to 4 bytes"):
        st.sc_add_device(dev.ptr + 2, len(c) - 1, 16)                             # read as floats on the device: refused, not launched
    with pytest.raises(pkg.LioError, match="multiple of 4"):
        st.sc_add_device(dev.ptr, len(c) - 1, 18)
    dev.close()
    assert st.sc_count() == 9
    assert st.sc_detect(cfg).loop_id == 1                                         # the refusals left the store usable
    # a handle that has staged nothing, and a store on another device than the handle's (refused before anything else is looked at)
    h = pkg.ScanToMap()
    with pytest.raises(pkg.LioError, match="no cloud staged"):
        st.sc_add_from_handle(h)
    h.close()
    if torch.cuda.device_count() > 1:
        h = pkg.ScanToMap(device_id=1)
        with pytest.raises(pkg.LioError, match="different devices"):
            st.sc_add_from_handle(h)
        h.close()
    st.close()


# ---------------------------------------------------------------------------------------------------------------- chain
def test_one_callback_feeds_the_keyframe_the_descriptor_the_detection_and_the_icp(pkg, synth):
    """saveKeyFramesAndFactor MO:2136-2156 + performSCLoopClosure MO:1163-1269 from one lio_s2m_register_raw per keyframe:
    nothing but poses and the result structs visit the host."""
    n_kf, revisit = 7, 1
    boxes = synth.make_scene(21, length=120.0, kind="street")
    poses = synth.keyframe_poses(60, spacing=2.0, seed=21)
    order = list(range(n_kf)) + [revisit]
    case = synth.make_case("vlp16", n_keyframes=6, seed=21, device="cpu")
    h = pkg.ScanToMap()
    h.set_map(case["map"])
    lay = pkg.PC2Layout(point_step=32, off_x=0, off_intensity=16, off_ring=-1, off_time=-1)
    sc_cfg = pkg.sc_default_config(num_exclude_recent=4)
    st, m = pkg.KeyframeStore(), R.Manager(num_exclude_recent=4)
    for j, k in enumerate(order):
        xyz = pinned_part(sweep(synth, "vlp16", "street", k=k, seed=800 + j))[0]
        _, _, _, n_ds = h.downsampleAndScan2MapOptimization(xyzi_records(xyz), len(xyz), lay, 0.4, poses[k].astype(np.float32))
        kid = st.add_from_handle(h)                                               # laserCloudSurfLastDS -> surfCloudKeyFrames
        assert st.sc_add_from_handle(h, sc_cfg) == kid == j                       # cloud_deskewed -> polarcontexts_
        assert int(pkg.load_library().lio_kf_store_points(st.h, kid)) == n_ds
        st.set_poses(j, poses[k].astype(np.float32)[None], [0.1 * j])
        m.add(R.make_desc(xyz))
        check_triplet(st.sc_get(j), m.descs[j])
    res, out = st.sc_detect(sc_cfg), m.detect()
    compare_detection(res, out)
    assert res.loop_id == revisit
    key_cur, search_num = len(st) - 1, 2
    icp_cfg = pkg.icp_default_config(min_source_points=100, min_target_points=300)
    r, rc, _ = st.loop_icp(key_cur, res.loop_id, search_num, 0.4, cfg=icp_cfg, pose_index=0)
    assert rc == 0 and r.status == 0
    base = poses[order[0]].astype(np.float32)
    near = [i for i in range(res.loop_id - search_num, res.loop_id + search_num + 1) if 0 <= i < len(st)]
    _, n_src, _ = st.assemble([key_cur], base[None], 0.4, want_output=False)
    _, n_tgt, _ = st.assemble(near, np.repeat(base[None], len(near), 0), 0.4, want_output=False)
    assert (r.n_source, r.n_target) == (n_src, n_tgt) and n_src > 100 and n_tgt > n_src
    h.close(); st.close()


# ------------------------------------------------------------------------------------------------------------ lifecycle
def test_many_adds_growing_storage_two_stores_and_destroy_with_work_in_flight(pkg, small_case):
    over = dict(num_exclude_recent=5, num_candidates=4, tree_period=1)
    cfg_a, cfg_b = pkg.sc_default_config(**over), pkg.sc_default_config(num_rings=8, num_sectors=24, **over)
    a, b = pkg.KeyframeStore(), pkg.KeyframeStore()
    ma, mb = R.Manager(**over), R.Manager(num_rings=8, num_sectors=24, **over)
    clouds = [random_cloud(900 + k, n=300) for k in range(16)]
    n = 600                                                                       # past two doublings of the descriptor storage
    for k in range(n):
        c = clouds[(k * 7) % 16][k % 3::3]
        a.sc_add(c, cfg_a)
        if k % 2 == 0:
            cb = pinned_part(c, num_rings=8, num_sectors=24)[0]
            b.sc_add(cb, cfg_b); mb.add(R.make_desc(cb, num_rings=8, num_sectors=24))
        ma.add(R.make_desc(c))
    assert a.sc_count() == n and b.sc_count() == n // 2
    for k in (0, 1, 255, 256, 257, 511, 512, n - 1):                              # across the blocks that were moved
        check_triplet(a.sc_get(k), ma.descs[k])
    for k in (0, 128, 255, 256, n // 2 - 1):
        check_triplet(b.sc_get(k), mb.descs[k])
    res_a, res_b = a.sc_detect(cfg_a), b.sc_detect(cfg_b)
    assert res_a.n_searched == n - 5 and res_b.n_searched == n // 2 - 5
    assert list(res_a.cand_idx[:4]) == ma.detect()["cand_idx"] and list(res_b.cand_idx[:4]) == mb.detect()["cand_idx"]
    # destroy a store while another handle's launch loop is still in flight on its own stream, then keep using the other
    q = small_case["queries"][0]
    s = pkg.ScanToMap(max_batch=16)
    s.set_map(small_case["map"])
    s.batch_upload([q["scan"]] * 16); s.batch_set_poses(np.repeat(q["pose_init"][None], 16, 0)); s.batch_run()
    a.sc_add(clouds[0], cfg_a)
    a.close()
    s.batch_sync()
    s.close()
    assert b.sc_add(pinned_part(clouds[1], num_rings=8, num_sectors=24)[0]) == n // 2
    assert b.sc_detect(cfg_b).n_searched == n // 2 + 1 - 5
    b.close()
