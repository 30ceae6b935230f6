"""The global map (publishGlobalMap MO:992-1041), the map export (saveMapService MO:935-962), the keyframe read-back and
the registered clouds (publishFrames MO:2330-2345) on the device, against the restatement of tests/globalmap_restate.py
(pinned by tests/test_globalmap_cpu.py).  Every comparison is on uint32 views: the kernels are K6's and K7's arithmetic,
so no tolerance is needed.

Key-pose times: lio_kf_store_set_poses refuses a first pose without a time, so "times never set" is exercised as far as
the interface allows -- every time left at 0.0, and a second store with times in disorder: the global map reads none."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import globalmap_restate as G                                  # noqa: E402
from test_globalmap_cpu import PASS_DENSITY                    # noqa: E402

pytestmark = pytest.mark.gpu


def _eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def _store(pkg, clouds, poses, times=None):
    st = pkg.KeyframeStore()
    for c in clouds:
        st.add(c)
    if len(clouds):
        st.set_poses(0, poses, np.zeros(len(clouds)) if times is None else times)
    return st


@pytest.fixture(scope="module")
def curved(oracle):
    poses, clouds = G.curved_path(seed=G.CURVED_SEED)
    ref = {}
    for name, (dens, leaf) in {"plain": (G.CURVED_DENSITY, G.CURVED_LEAF), "pose_pass": (PASS_DENSITY, G.CURVED_LEAF),
                               "leaf_pass": (G.CURVED_DENSITY, 1e-4)}.items():
        ref[name] = G.global_map(oracle, clouds, poses, G.CURVED_R, dens, leaf)
    return poses, clouds, ref


@pytest.fixture(scope="module")
def curved_store(pkg, curved):
    st = _store(pkg, curved[1], curved[0])
    yield st
    st.close()


def _gm(pkg, st, dens, leaf, R=G.CURVED_R):
    return st.global_map(pkg.global_map_default_config(search_radius=R, pose_density=dens, leaf=leaf))


# ------------------------------------------------------------------ global map
def test_global_map_ids_and_cloud_equal_the_restatement(pkg, curved, curved_store):
    m_ref, ids_ref, info_ref = curved[2]["plain"]
    m, ids, info = _gm(pkg, curved_store, G.CURVED_DENSITY, G.CURVED_LEAF)
    assert ids.tolist() == ids_ref.tolist() and len(ids) > len(set(ids.tolist()))          # duplicates included
    _eq(m, m_ref)
    assert (info.n_keyframes, info.n_summed, info.n_out, info.voxel_passthrough) == (len(ids_ref), info_ref["n_summed"], len(m_ref), 0)
    # a second call from the kept workspace, then without the outputs: the same counts
    m2, ids2, _ = _gm(pkg, curved_store, G.CURVED_DENSITY, G.CURVED_LEAF)
    _eq(m2, m)
    assert ids2.tolist() == ids.tolist()
    _, _, info3 = curved_store.global_map(pkg.global_map_default_config(search_radius=G.CURVED_R, pose_density=G.CURVED_DENSITY,
                                                                        leaf=G.CURVED_LEAF), want_ids=False, want_output=False)
    assert (info3.n_keyframes, info3.n_out) == (info.n_keyframes, info.n_out)


def test_global_map_when_the_pose_filter_passes_through(pkg, curved, curved_store):
    m_ref, ids_ref, info_ref = curved[2]["pose_pass"]
    assert info_ref["pose_passthrough"] == 1 and len(ids_ref) == info_ref["n_hits"]
    m, ids, info = _gm(pkg, curved_store, PASS_DENSITY, G.CURVED_LEAF)
    assert ids.tolist() == ids_ref.tolist()
    _eq(m, m_ref)


def test_global_map_when_the_cloud_filter_overflows(pkg, oracle, curved, curved_store):
    m_ref, ids_ref, info_ref = curved[2]["leaf_pass"]
    assert info_ref["voxel_passthrough"] == 1
    m, ids, info = _gm(pkg, curved_store, G.CURVED_DENSITY, 1e-4)
    assert info.voxel_passthrough == 1 and info.n_out == info.n_summed
    _eq(m, G.summed(oracle, curved[1], curved[0], ids_ref))                                 # the output is the sum itself
    _eq(m, m_ref)


def test_global_map_reads_no_key_pose_time(pkg, curved, curved_store):
    poses, clouds, ref = curved
    rng = np.random.default_rng(1)
    st = _store(pkg, clouds, poses, rng.permutation(len(clouds)) * 1e6)                     # (curved_store: every time 0.0)
    try:
        m, ids, _ = _gm(pkg, st, G.CURVED_DENSITY, G.CURVED_LEAF)
    finally:
        st.close()
    assert ids.tolist() == ref["plain"][1].tolist()
    _eq(m, ref["plain"][0])


def test_global_map_single_keyframe_and_empty_store(pkg, oracle, curved):
    poses, clouds, _ = curved
    k = next(i for i, c in enumerate(clouds) if len(c) > 10)
    st = _store(pkg, [clouds[k]], poses[k:k + 1])
    try:
        m, ids, info = st.global_map()
        m_ref, ids_ref, _ = G.global_map(oracle, [clouds[k]], poses[k:k + 1])
        assert ids.tolist() == ids_ref.tolist() == [0]
        _eq(m, m_ref)
    finally:
        st.close()
    st = pkg.KeyframeStore()
    try:
        m, ids, info = st.global_map()
        assert len(m) == 0 and len(ids) == 0 and (info.n_keyframes, info.n_summed, info.n_out) == (0, 0, 0)
    finally:
        st.close()


# ------------------------------------------------------------------ export
@pytest.fixture(scope="module")
def export(pkg, oracle):
    poses, clouds = G.export_case()
    full, ds, vpt = G.export_map(oracle, clouds, poses, 0.5)
    st = _store(pkg, clouds, poses)
    yield poses, clouds, full, ds, st
    st.close()


@pytest.mark.parametrize("stride", [32, 20])
def test_export_is_the_concatenation_for_every_chunk_size(pkg, oracle, export, stride):
    poses, clouds, full_ref, ds_ref, st = export
    for chunk in (256, 768, 0):
        full, ds, (n_full, n_ds, vpt) = st.export_map(0.5, chunk_points=chunk, stride=stride)
        assert n_full == len(full_ref) == sum(len(c) for c in clouds) and vpt == 0
        _eq(full, full_ref)
        _eq(ds, oracle.voxel_grid(full, np.float32(0.5))[0])
        _eq(ds, ds_ref)
        assert st.export_map(0.5, chunk_points=chunk, stride=stride, want_full=False, want_ds=False)[2] == (n_full, n_ds, 0)


def test_export_records_are_pcl_records(pkg, export):
    """The whole 32-byte record, not only its four fields: data[3] = 1, the padding zero, nothing behind the last record."""
    _, _, full_ref, _, st = export
    n = len(full_ref)
    buf = np.full((n + 3, 8), 7.0, np.float32)
    cfg = pkg.ExportConfig(0.0, 768)
    n_full, n_ds, vpt = C.c_size_t(), C.c_size_t(), C.c_int32(5)
    sentinel = np.full((4, 8), 9.0, np.float32)
    rc = st.lib.lio_kf_store_export_map(st.h, C.byref(cfg), buf.ctypes.data, 32, n, C.byref(n_full), sentinel.ctypes.data, 32, 4,
                                        C.byref(n_ds), C.byref(vpt))
    assert rc == 0 and n_full.value == n and n_ds.value == 0 and vpt.value == 0
    assert (sentinel == 9.0).all()                                   # resolution 0: out_ds untouched
    assert (buf[n:] == 7.0).all()
    _eq(buf[:n, [0, 1, 2, 4]], full_ref)
    assert (buf[:n, 3] == 1.0).all() and (buf[:n, 5:].view(np.uint32) == 0).all()


def test_export_records_wider_than_the_lds_tile(pkg, export):
    """A stride of 80 bytes: records above 64 bytes take the kernel's field-by-field stores.  The whole record is checked,
    with and without a filtered copy (the chunks are then cut from the world-frame cloud), over ragged chunks."""
    _, _, full_ref, ds_ref, st = export
    n, W = len(full_ref), 20
    for res in (0.0, 0.5):
        buf = np.full((n + 3, W), 7.0, np.float32)
        ds = np.full((len(ds_ref) + 2, W), 9.0, np.float32)
        cfg = pkg.ExportConfig(res, 768)
        n_full, n_ds, vpt = C.c_size_t(), C.c_size_t(), C.c_int32()
        rc = st.lib.lio_kf_store_export_map(st.h, C.byref(cfg), buf.ctypes.data, 4 * W, n, C.byref(n_full), ds.ctypes.data, 4 * W, len(ds_ref),
                                            C.byref(n_ds), C.byref(vpt))
        assert rc == 0 and n_full.value == n and n_ds.value == (len(ds_ref) if res else 0)
        assert (buf[n:] == 7.0).all()                                # nothing behind the last record
        _eq(buf[:n, [0, 1, 2, 4]], full_ref)
        assert (buf[:n, 3] == 1.0).all() and (buf[:n, 5:].view(np.uint32) == 0).all()
        if res:
            m = len(ds_ref)
            _eq(ds[:m, [0, 1, 2, 4]], ds_ref)
            assert (ds[:m, 3] == 1.0).all() and (ds[:m, 5:].view(np.uint32) == 0).all() and (ds[m:] == 9.0).all()
        else:
            assert (ds == 9.0).all()


def test_export_when_the_filter_overflows(pkg, export):
    _, _, full_ref, _, st = export
    full, ds, (n_full, n_ds, vpt) = st.export_map(1e-3, chunk_points=768)
    assert vpt == 1 and n_ds == n_full
    _eq(ds, full_ref)
    _eq(full, full_ref)


# ------------------------------------------------------------------ read-back and registered clouds
def _pcl(xyz, intensity):
    rec = np.zeros((len(xyz), 8), np.float32)
    rec[:, :3], rec[:, 3], rec[:, 4] = xyz, 1.0, intensity
    return rec


@pytest.fixture(scope="module")
def sweep(synth):
    boxes = synth.make_scene(11, length=60.0)
    pose = synth.keyframe_poses(6, seed=11)[1]
    sc = synth.cast_scan(boxes, pose, "vlp16", seed=301, device="cpu")
    xyzi = np.concatenate([sc["xyz"], sc["intensity"][:, None]], 1).astype(np.float32)
    return xyzi, pose.astype(np.float32)


LAYOUT = dict(point_step=32, off_x=0, off_intensity=16, off_ring=-1, off_time=-1)


def test_registered_clouds_and_keyframe_read_back(pkg, oracle, small_case, sweep, export):
    xyzi, pose = sweep
    h = pkg.ScanToMap()
    h.set_map(small_case["map"])
    n = C.c_size_t()
    p6 = pose.ctypes.data_as(C.POINTER(C.c_float))
    # nothing staged yet
    assert h.lib.lio_s2m_registered_cloud(h.h, pkg.STAGED_RAW, p6, None, 32, 0, C.byref(n)) == -1
    assert h.lib.lio_s2m_registered_cloud(h.h, pkg.STAGED_DS, p6, None, 32, 0, C.byref(n)) == -1
    # a plain registration stages the scan but no raw cloud
    scan = xyzi[::7]
    h.scan2MapOptimization(_pcl(scan[:, :3], scan[:, 3]), pose)
    _eq(h.registered_cloud(pkg.STAGED_DS, pose), oracle.transform_point_cloud(scan, pose))
    assert h.lib.lio_s2m_registered_cloud(h.h, pkg.STAGED_RAW, p6, None, 32, 0, C.byref(n)) == -1
    # the callback chain stages both
    final, res, rc, ds = h.downsampleAndScan2MapOptimization(_pcl(xyzi[:, :3], xyzi[:, 3]), len(xyzi), pkg.PC2Layout(**LAYOUT), 0.4, pose,
                                                             want_ds=True)
    _eq(h.registered_cloud(pkg.STAGED_DS, final), oracle.transform_point_cloud(ds, final))
    _eq(h.registered_cloud(pkg.STAGED_RAW, final), oracle.transform_point_cloud(xyzi, final))
    # a cap that is too small: the needed count, nothing written
    small = np.full((4, 8), 3.0, np.float32)
    fp = np.ascontiguousarray(final, np.float32)
    assert h.lib.lio_s2m_registered_cloud(h.h, pkg.STAGED_RAW, fp.ctypes.data_as(C.POINTER(C.c_float)), small.ctypes.data, 32, 4,
                                          C.byref(n)) == -1
    assert n.value == len(xyzi) and (small == 3.0).all()
    bad = fp.copy(); bad[1] = np.inf
    assert h.lib.lio_s2m_registered_cloud(h.h, pkg.STAGED_DS, bad.ctypes.data_as(C.POINTER(C.c_float)), None, 32, 0, C.byref(n)) == -1
    assert h.lib.lio_s2m_registered_cloud(h.h, 2, p6, None, 32, 0, C.byref(n)) == -1
    # a multi-device handle is refused for both kinds, *n_out and the buffer untouched -- also once it has registered a scan
    many = pkg.ScanToMap(n_devices=2, device_ids=[0, 0])
    try:
        many.set_map(small_case["map"])
        for registered in (False, True):
            if registered:
                many.scan2MapOptimization(_pcl(scan[:, :3], scan[:, 3]), pose)
            for which in (pkg.STAGED_DS, pkg.STAGED_RAW):
                buf = np.full((len(xyzi), 8), 3.0, np.float32)
                cnt = C.c_size_t(12345)
                assert many.lib.lio_s2m_registered_cloud(many.h, which, p6, buf.ctypes.data, 32, len(buf), C.byref(cnt)) == -1
                assert cnt.value == 12345 and (buf == 3.0).all()
                assert b"single-device" in many.lib.lio_last_error()
    finally:
        many.close()
    # ---- read-back: the keyframes of the export case and one that add_from_handle made
    poses, clouds, _, _, st = export
    for k, c in enumerate(clouds):
        _eq(st.get_keyframe(k), c)
    rng = np.random.default_rng(2)
    for k in (int(i) for i in np.argsort([-len(c) for c in clouds])[:3]):
        p = (rng.uniform(-1, 1, 6) * np.array([0.3, 0.3, 3.0, 40.0, 40.0, 3.0])).astype(np.float32)
        _eq(st.get_keyframe(k, p), oracle.transform_point_cloud(clouds[k], p))
    st2 = pkg.KeyframeStore()
    try:
        kid = st2.add_from_handle(h)
        _eq(st2.get_keyframe(kid), ds)
        _eq(st2.get_keyframe(kid, final), oracle.transform_point_cloud(ds, final))
    finally:
        st2.close()
    h.close()


# ------------------------------------------------------------------ isolation
def test_global_map_and_export_leave_the_store_and_the_handle_alone(pkg, synth, curved):
    poses, clouds, _ = curved
    times = 100.0 + 0.5 * np.arange(len(clouds))
    st = _store(pkg, clouds, poses, times)
    h = pkg.ScanToMap()
    try:
        m0, n0, ids0, _ = st.assemble_nearby(times[-1] + 0.1, 0.5, s2m=h, search_radius=40.0)
        # a scan that lies on the map: every third map point, seen from the last key pose
        T = np.linalg.inv(synth.pose_matrix(poses[-1].astype(np.float64)))
        scan = np.ascontiguousarray((m0[::3, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
        assert len(scan) > 100
        p0, r0, rc0 = h.scan2MapOptimization(scan, poses[-1])
        gm = _gm(pkg, st, G.CURVED_DENSITY, G.CURVED_LEAF)
        ex = st.export_map(0.5, chunk_points=768)
        # the map installed before the two calls still registers the same scan to the same bits
        p1, r1, rc1 = h.scan2MapOptimization(scan, poses[-1])
        assert rc0 == rc1 and r0.iters == r1.iters >= 1
        np.testing.assert_array_equal(p0.view(np.uint32), p1.view(np.uint32))
        assert bytes(r0) == bytes(r1)                                 # the whole lio_s2m_result
        m2, n2, ids2, _ = st.assemble_nearby(times[-1] + 0.1, 0.5, s2m=h, search_radius=40.0)
        assert ids2.tolist() == ids0.tolist() and n2 == n0
        _eq(m2, m0)
        _eq(_gm(pkg, st, G.CURVED_DENSITY, G.CURVED_LEAF)[0], gm[0])
        _eq(st.export_map(0.5, chunk_points=0)[0], ex[0])
    finally:
        h.close(); st.close()


# ------------------------------------------------------------------ errors
def test_errors_return_err_arg_and_the_needed_counts(pkg, curved, curved_store, export):
    L = curved_store.lib
    i32p = C.POINTER(C.c_int32)
    n_ids, n_out, info = C.c_int32(), C.c_size_t(), pkg.GlobalMapInfo()
    good = dict(search_radius=G.CURVED_R, pose_density=G.CURVED_DENSITY, leaf=G.CURVED_LEAF)

    def gm(cfg, ids=None, ids_cap=0, out=None, cap=0):
        return L.lio_kf_store_global_map(curved_store.h, C.byref(cfg), ids.ctypes.data_as(i32p) if ids is not None else None, ids_cap,
                                         C.byref(n_ids), out.ctypes.data if out is not None else None, 32, cap, C.byref(n_out), C.byref(info))
    for field in good:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert gm(pkg.global_map_default_config(**{**good, field: bad})) == -1, (field, bad)
    ref_ids, ref_n = len(curved[2]["plain"][1]), len(curved[2]["plain"][0])
    small = np.full(2, -5, np.int32)
    assert gm(pkg.global_map_default_config(**good), ids=small, ids_cap=2) == -1 and n_ids.value == ref_ids > 2
    assert small.tolist() == [-5, -5]
    out = np.full((4, 8), 3.0, np.float32)
    assert gm(pkg.global_map_default_config(**good), out=out, cap=4) == -1 and n_out.value == ref_n > 4 and (out == 3.0).all()
    assert gm(pkg.global_map_default_config(**good)) == 0 and (n_ids.value, n_out.value) == (ref_ids, ref_n)
    # a keyframe without a pose: all three store calls refuse
    poses, clouds, full_ref, ds_ref, est = export
    st = _store(pkg, clouds[:6], poses[:6])
    st.add(clouds[7])
    try:
        with pytest.raises(pkg.LioError, match="no pose"):
            st.global_map()
        with pytest.raises(pkg.LioError, match="no pose"):
            st.export_map()
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.get_keyframe(7)
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            st.get_keyframe(-1)
        with pytest.raises(pkg.LioError, match="non-finite"):
            st.get_keyframe(1, [0, 0, np.nan, 0, 0, 0])
        n = C.c_size_t()
        k = next(i for i in range(6) if len(clouds[i]) > 4)
        buf = np.full((4, 8), 3.0, np.float32)
        assert L.lio_kf_store_get_keyframe(st.h, k, None, buf.ctypes.data, 32, 4, C.byref(n)) == -1
        assert n.value == len(clouds[k]) and (buf == 3.0).all()
        _eq(st.get_keyframe(6), clouds[7])                            # (a keyframe needs no pose to be read back as stored)
    finally:
        st.close()
    # export: resolution, chunk_points, caps
    n_full, n_ds, vpt = C.c_size_t(), C.c_size_t(), C.c_int32()

    def ex(res, chunk, full=None, full_cap=0, ds=None, ds_cap=0):
        cfg = pkg.ExportConfig(res, chunk)
        return L.lio_kf_store_export_map(est.h, C.byref(cfg), full.ctypes.data if full is not None else None, 32, full_cap, C.byref(n_full),
                                         ds.ctypes.data if ds is not None else None, 32, ds_cap, C.byref(n_ds), C.byref(vpt))
    for res in (-0.5, float("nan"), float("inf")):
        assert ex(res, 0) == -1
    for chunk in (-1, 1, 255, (1 << 26) + 1):
        assert ex(0.5, chunk) == -1
    assert ex(0.5, 256) == 0 and ex(0.5, 1 << 26) == 0 and (n_full.value, n_ds.value) == (len(full_ref), len(ds_ref))
    a, b = np.full((8, 8), 3.0, np.float32), np.full((len(full_ref), 8), 3.0, np.float32)
    assert ex(0.5, 0, full=a, full_cap=8, ds=b, ds_cap=len(b)) == -1
    assert (n_full.value, n_ds.value) == (len(full_ref), len(ds_ref)) and (a == 3.0).all() and (b == 3.0).all()
    assert ex(0.5, 0, full=b, full_cap=len(b), ds=a, ds_cap=8) == -1
    assert (n_full.value, n_ds.value) == (len(full_ref), len(ds_ref)) and (a == 3.0).all() and (b == 3.0).all()
    assert ex(0.0, 0, full=b, full_cap=len(b), ds=a, ds_cap=0) == 0 and (a == 3.0).all()      # resolution 0: ds_cap does not matter
    assert L.lio_kf_store_export_map(est.h, C.byref(pkg.ExportConfig(0.0, 0)), b.ctypes.data, 16, len(b), C.byref(n_full), None, 32, 0,
                                     C.byref(n_ds), C.byref(vpt)) == -1                          # a stride below 20
