"""The two places where the shared cloud upload (lio_upload_xyzi) and the shared keyframe sum (lio_kf_sum_*) could change
bits without any other test noticing: which byte of a host record becomes the intensity, and how the sum treats an empty
keyframe, an exact 256-point chunk, a single point and a chunk plus one when the id range is clipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restate as R                                    # noqa: E402
import localmap_restate as L                               # noqa: E402

pytestmark = pytest.mark.gpu
COUNTS = (300, 0, 256, 1, 257)         # a chunk and a tail, empty, an exact chunk, one point, a chunk plus one
LEAF = 0.05


def rows(a):
    """The rows of a float32 array as a sorted list of bit patterns: equality as a set, bit for bit."""
    return sorted(map(bytes, np.ascontiguousarray(a, np.float32)))


# ---- the intensity offset of host records
@pytest.fixture(scope="module")
def records():
    """257 records of 32 bytes (two workgroups and a one-record tail): x, y, z, then distinct non-zero floats at bytes 12,
    20, 24 and 28 around the intensity at byte 16.  One point per voxel at leaf 0.25, ascending voxel key = input order."""
    n = 257
    rec = np.zeros((n, 8), np.float32)
    i = np.arange(n, dtype=np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = i, 0.5, -0.25
    rec[:, 3] = 1000.0 + i          # byte 12
    rec[:, 4] = 0.5 + i             # byte 16: the intensity
    rec[:, 5] = 2000.0 + i          # byte 20
    rec[:, 6] = 3000.0 + i          # byte 24
    rec[:, 7] = 4000.0 + i          # byte 28
    return rec


def test_voxel_grid_reads_the_intensity_at_byte_16(pkg, records):
    lib, n = pkg.load_library(), len(records)
    out = np.zeros((n, 8), np.float32)
    n_out = C.c_size_t()
    assert lib.lio_voxel_grid(0, records.ctypes.data, n, 32, C.c_float(0.25), out.ctypes.data, 32, C.byref(n_out)) == 0
    assert n_out.value == n                                                       # every point is its own voxel
    assert np.array_equal(out[:, :3].view(np.uint32), records[:, :3].view(np.uint32))
    assert np.array_equal(out[:, 4].view(np.uint32), records[:, 4].view(np.uint32))


def test_kf_store_add_reads_the_intensity_at_byte_16(pkg, records):
    st = pkg.KeyframeStore()
    try:
        kid = C.c_int32(-1)
        assert st.lib.lio_kf_store_add(st.h, records.ctypes.data, len(records), 32, C.byref(kid)) == 0 and kid.value == 0
        got = st.get_keyframe(0)
        assert np.array_equal(got.view(np.uint32), records[:, [0, 1, 2, 4]].view(np.uint32))
    finally:
        st.close()


# ---- the keyframe sum
@pytest.fixture(scope="module")
def sums(pkg, oracle):
    rng = np.random.default_rng(257)
    clouds = []
    for n in COUNTS:
        c = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32) * np.array([10.0, 10.0, 2.0, 50.0], np.float32)
        clouds.append(c)
    poses = np.array([[0.01 * k, -0.02 * k, 0.3 * k - 0.5, 2.0 * k, -1.5 * k, 0.1 * k] for k in range(len(COUNTS))], np.float32)
    st = pkg.KeyframeStore()
    for c in clouds:
        st.add(c)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 10.0)
    assert [int(st.lib.lio_kf_store_points(st.h, k)) for k in range(len(COUNTS))] == list(COUNTS)

    def world(ids, pose_ids):
        """K6 as the tests restate it: keyframe ids[k] under the stored pose of pose_ids[k], concatenated."""
        parts = []
        for i, p in zip(ids, pose_ids):
            roll, pitch, yaw, x, y, z = (float(v) for v in poses[p])
            M = oracle.get_transformation(x, y, z, roll, pitch, yaw)
            parts.append(np.concatenate([R.transform_points(M, clouds[i][:, :3]), clouds[i][:, 3:4]], 1))
        return np.concatenate(parts)

    yield dict(store=st, world=world)
    st.close()


@pytest.mark.parametrize("pose_index", [-1, 2])
@pytest.mark.parametrize("key,ids", [(0, [0, 1, 2]), (4, [2, 3, 4])])
def test_loop_submap_with_a_clipped_range(sums, key, ids, pose_index):
    """search_num = 2 around the first and the last keyframe: the range is clipped below and above.  The leaf leaves every
    point a voxel of its own, so the filtered submap is the sum as a set."""
    st = sums["store"]
    res, rc, (src, tgt, _) = st.loop_icp(2, key, 2, LEAF, pose_index=pose_index, want_clouds=True)
    assert rc > 0                                                                 # MO:1104: too few points, nothing is aligned
    ref_t = sums["world"](ids, ids if pose_index < 0 else [pose_index] * len(ids))
    ref_s = sums["world"]([2], [2])
    assert (res.n_source, res.n_target) == (len(ref_s), len(ref_t)) == (256, sum(COUNTS[i] for i in ids))
    assert rows(tgt) == rows(ref_t)
    assert rows(src) == rows(ref_s)


def test_local_map_sums_every_keyframe_in_order(pkg, sums):
    st = sums["store"]
    pose = np.array([0.0, 0.0, 0.7, 3.0, -2.0, 0.5], np.float32)
    box = dict(front=1e4, left=1e4, back=1e4, right=1e4)
    out, info, rc = st.local_map(pose, pkg.local_map_default_config(n_keyframes=5, remove_outliers=0, downsample=0, **box))
    ids = list(range(len(COUNTS)))
    ref, keep = L.crop(sums["world"](ids, ids), pose, **box)
    assert rc == 0 and keep.all() and (info.first_keyframe, info.n_keyframes, info.n_summed, info.n_out) == (0, 5, sum(COUNTS), sum(COUNTS))
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
