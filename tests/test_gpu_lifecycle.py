"""Handle lifecycle: a SLAM node runs for hours and re-creates nothing, but a service that registers batches creates
and destroys handles all day.  Every flavour of handle must give its device memory back on destroy, survive
destroy in any state (mid-run, after an error), and leave later handles unaffected.  The reference's analogue is the
node's constructor/destructor pair (allocateMemory MO:229-262 and the pcl::PointCloud::Ptr members it resets)."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _one_round(pkg, case, flavour):
    qs = case["queries"]
    scans = [q["scan"] for q in qs]
    poses0 = np.stack([q["pose_init"] for q in qs])
    if flavour == "plain":
        s = pkg.ScanToMap(sort_scan=2, use_graph=1, graph_iters=4)
        s.set_map(case["map"])
        s.batch_upload(scans); s.batch_set_poses(poses0); s.batch_run()
        p, _ = s.batch_results()
        s.close()
    elif flavour == "sharer":
        a = pkg.ScanToMap(sort_scan=2)
        b = pkg.ScanToMap(sort_scan=2)
        a.set_map(case["map"]); b.share_map(a)
        b.batch_upload(scans); b.batch_set_poses(poses0); b.batch_run()
        p, _ = b.batch_results()
        a.close(); b.close()                      # the owner goes first: the sharer must not touch freed memory
    elif flavour == "cert":
        s = pkg.ScanToMap(sort_scan=2, pipeline=1)
        s.set_map(case["map"])
        s.batch_upload(scans); s.batch_set_poses(poses0); s.batch_run()
        p, _ = s.batch_results()
        s.close()
    elif flavour == "multi":
        s = pkg.ScanToMap(sort_scan=2, n_devices=2, device_ids=[0, 0])
        s.set_map(case["map"])
        s.batch_upload(scans); s.batch_set_poses(poses0); s.batch_run()
        p, _ = s.batch_results()
        s.close()
    elif flavour == "abandoned":
        s = pkg.ScanToMap(sort_scan=2, use_graph=1, graph_iters=4)
        s.set_map(case["map"])
        s.batch_upload(scans); s.batch_set_poses(poses0); s.batch_run()
        s.close()                                 # destroyed with the launch loop still in flight
        p = None
    elif flavour == "store":
        st = pkg.KeyframeStore()
        rec = np.zeros((len(case["map"]), 4), np.float32)
        rec[:, :3] = case["map"]
        for k in range(4):
            st.add(rec[k::4])
        s = pkg.ScanToMap(sort_scan=2)
        ident = np.zeros((4, 6), np.float32)
        st.assemble(list(range(4)), ident, 0.4, s2m=s, want_output=False)
        p, _, _ = s.scan2MapOptimization(scans[0], poses0[0])
        s.close(); st.close()
    elif flavour == "raw":                        # the raw-sweep workspace of the handle, and a keyframe taken from it
        lay = pkg.PC2Layout(point_step=32, off_x=0, off_intensity=16, off_ring=-1, off_time=-1, pin_host=0)
        raw = np.zeros((len(scans[0]), 8), np.float32)
        raw[:, :3] = scans[0]; raw[:, 4] = 1.0
        s = pkg.ScanToMap()
        s.set_map(case["map"])
        p, _, _, _ = s.downsampleAndScan2MapOptimization(raw, len(raw), lay, 0.4, poses0[0])
        st = pkg.KeyframeStore()
        st.add_from_handle(s)
        s.close(); st.close()
    elif flavour == "nearby":                     # the store's key-pose table and selection workspace
        st = pkg.KeyframeStore()
        rec = np.zeros((len(case["map"]), 4), np.float32)
        rec[:, :3] = case["map"]
        for k in range(4):
            st.add(rec[k::4])
        st.set_poses(0, np.zeros((4, 6), np.float32), np.arange(4, dtype=np.float64))
        s = pkg.ScanToMap(sort_scan=2)
        st.assemble_nearby(3.5, 0.4, s2m=s, want_ids=False, want_output=False)
        p, _, _ = s.scan2MapOptimization(scans[0], poses0[0])
        s.close(); st.close()
    elif flavour == "corner":                     # the corner child handle
        s = pkg.ScanToMap()
        s.set_map(case["map"])
        s.set_corner_map(case["map"][::3])
        p, _, _ = s.scan2MapOptimizationCS(scans[0][::4], scans[0], poses0[0])
        s.close()
    elif flavour == "persist":                    # the one-launch loop's generation numbers and speculation sums
        s = pkg.ScanToMap(sort_scan=2, pipeline=4)
        s.set_map(case["map"])
        s.batch_upload(scans); s.batch_set_poses(poses0); s.batch_run()
        p, _ = s.batch_results()
        s.close()
    return p


@pytest.mark.parametrize("flavour", ["plain", "sharer", "cert", "multi", "abandoned", "store", "raw", "nearby", "corner", "persist"])
def test_destroy_returns_device_memory(pkg, small_case, flavour):
    first = _one_round(pkg, small_case, flavour)   # warm-up: code objects, HIP's own pools, pinned staging
    _one_round(pkg, small_case, flavour)
    gc.collect()
    before = _free_bytes()
    for _ in range(12):
        again = _one_round(pkg, small_case, flavour)
        if first is not None:
            np.testing.assert_array_equal(again, first)
    gc.collect()
    after = _free_bytes()
    # a leak of one handle's buffers is tens of MiB per round; allow allocator granularity only
    assert before - after < 8 << 20, (flavour, before - after)


def test_error_then_reuse(pkg, small_case):
    """A refused call leaves the handle usable (the node keeps its handle across a bad message)."""
    qs = small_case["queries"]
    s = pkg.ScanToMap(sort_scan=2)
    with pytest.raises(pkg.LioError):
        s.scan2MapOptimization(qs[0]["scan"], qs[0]["pose_init"])     # LIO_ERR_NO_MAP
    s.set_map(small_case["map"])
    with pytest.raises(pkg.LioError):
        s.batch_upload([qs[0]["scan"]]); s.batch_run()                # poses not set: LIO_ERR_ARG
    p, r, _ = s.scan2MapOptimization(qs[0]["scan"], qs[0]["pose_init"])
    ref = pkg.ScanToMap(sort_scan=2)
    ref.set_map(small_case["map"])
    pw, rw, _ = ref.scan2MapOptimization(qs[0]["scan"], qs[0]["pose_init"])
    np.testing.assert_array_equal(p, pw)
    assert r.iters == rw.iters
    s.close(); ref.close()


def test_upload_options_do_not_outlive_their_call(pkg, small_case):
    """What one entry asks of its upload -- a record layout (register_pc2), a pose carried inside the state and no wait
    (register), a wait for the copy only (batch_upload_async), the launch loop in place of the one-launch loop (the
    fall-back inside batch_results) -- holds for that call alone: six different calls in a row on ONE handle give, each,
    the bits the same call gives on a fresh handle."""
    qs = small_case["queries"]
    scan, pose0 = qs[0]["scan"], qs[0]["pose_init"]
    blob = np.zeros((len(scan), 4), np.float32)            # records of 16 bytes: intensity, x, y, z
    blob[:, 0] = 7.0; blob[:, 1:] = scan
    lay = pkg.PC2Layout(point_step=16, off_x=4, off_intensity=0, off_ring=-1, off_time=-1, pin_host=0)
    two = [qs[1]["scan"], qs[2]["scan"]]
    two_poses = np.stack([qs[1]["pose_init"], qs[2]["pose_init"]])
    rec = np.ascontiguousarray(np.concatenate(two), np.float32)
    pin = pkg.PinnedBuffer(rec.nbytes)
    pin.array[:] = rec.view(np.uint8).reshape(-1)

    def lone(out):
        p, r, rc = out
        assert rc == r.status
        return p[None], [r]

    def pc2(h):
        return lone(h.scan2MapOptimizationPC2(blob, len(blob), lay, pose0))

    def plain(h):
        return lone(h.scan2MapOptimization(scan, pose0))

    def async_batch(h):
        h.batch_upload_raw(pin.ptr, [len(s) for s in two], 12, asynchronous=True)
        h.batch_set_poses(two_poses); h.batch_run()
        return h.batch_results()

    def corners(h):
        h.set_corner_map(small_case["map"][::3])
        return lone(h.scan2MapOptimizationCS(scan[::4], scan, pose0))

    def timed_out(h):
        h.debug_persist_spin(spin_max=1, withhold_wg=0)    # the one-launch loop gives up: batch_results re-runs the launch loop
        out = lone(h.scan2MapOptimization(scan, pose0))
        assert h.profile().persist_fallbacks == 1 and h.profile().pipeline == 1
        h.debug_persist_spin(spin_max=0, withhold_wg=-1)
        return out

    def healthy(h):
        out = lone(h.scan2MapOptimization(scan, pose0))
        assert h.profile().pipeline == 4                   # the launch loop of the re-run did not stick
        return out

    steps = [pc2, plain, async_batch, corners, timed_out, healthy]
    shared = pkg.ScanToMap(pipeline=4)
    shared.set_map(small_case["map"])
    got = [step(shared) for step in steps]
    assert shared.profile().persist_fallbacks == 1
    shared.close()
    for step, (p, r) in zip(steps, got):
        fresh = pkg.ScanToMap(pipeline=4)
        fresh.set_map(small_case["map"])
        pw, rw = step(fresh)
        fresh.close()
        np.testing.assert_array_equal(p.view(np.uint32), pw.view(np.uint32), err_msg=step.__name__)
        for a, b in zip(r, rw):
            np.testing.assert_array_equal([a.iters, a.status], [b.iters, b.status], err_msg=step.__name__)
            for f in ("AtA", "AtB"):
                np.testing.assert_array_equal(np.array(getattr(a, f), np.float32).view(np.uint32),
                                              np.array(getattr(b, f), np.float32).view(np.uint32), err_msg=step.__name__)
    pin.close()


def test_sharer_follows_an_asynchronously_installed_map(pkg, small_case):
    """lio_assemble_map_resident returns with the owner's grid build still in flight on the owner's stream; a handle
    sharing that map runs on its own stream and must wait for the build (event), not read a half-built grid."""
    qs = small_case["queries"]
    m = small_case["map"]
    rec = np.zeros((len(m), 4), np.float32)
    rec[:, :3] = m
    st = pkg.KeyframeStore()
    ids = [st.add(rec[k::5]) for k in range(5)]
    ident = np.zeros((5, 6), np.float32)
    owner = pkg.ScanToMap()
    sharer = pkg.ScanToMap()
    sharer.share_map(owner)
    ref = pkg.ScanToMap()
    for rep in range(6):
        leaf = 0.4 + 0.05 * (rep % 3)                       # a different map every time
        out, n_out, _ = st.assemble(ids, ident, leaf, s2m=None, want_output=True, max_out=len(m))
        st.assemble(ids, ident, leaf, s2m=owner, want_output=False)          # asynchronous installation
        p_sh, r_sh, _ = sharer.scan2MapOptimization(qs[rep % len(qs)]["scan"], qs[rep % len(qs)]["pose_init"])
        ref.set_map(np.ascontiguousarray(out[:n_out, :3]))
        p_ref, r_ref, _ = ref.scan2MapOptimization(qs[rep % len(qs)]["scan"], qs[rep % len(qs)]["pose_init"])
        np.testing.assert_array_equal(p_sh, p_ref)
        assert r_sh.iters == r_ref.iters and list(r_sh.n_corr_iter) == list(r_ref.n_corr_iter)
    for h in (sharer, owner, ref):
        h.close()
    st.close()
