"""The permutation of the upload-time tile sort, pinned directly: both forms of the sort (the one-launch k_scan_sort_radix and
the multi-kernel counting sort + rank sort / big-tile sort) against the plain restatement of the contract in
tests/scan_order_restate.py, on the designed inputs of tests/scan_order_cases.py (tests/test_scan_order_cases_cpu.py proves
that each input reaches the edge it is named after).  Read back through lio_s2m_debug_scan_order: perm[base + j] = base + i and
the SoA the Gauss-Newton loop reads.  Everything is exact: no tolerance, no share of points left out."""
import ctypes as C
import functools

import numpy as np
import pytest

import scan_order_cases as sc
import scan_order_restate as so

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(perm int32 [total], SoA bits uint32 [total, 3]) by the restatement; computed once per case."""
    scans, cfg, _ = sc.build_case(name)
    perm = so.batch_perm(scans, sc.tile0_of(cfg), cfg.get("shard_axis", -1))
    rec = np.concatenate(scans) if scans else np.zeros((0, 3), np.float32)
    soa = np.ascontiguousarray(rec[perm]).view(np.uint32)
    perm.flags.writeable = False
    soa.flags.writeable = False
    return perm, soa


def _handle(pkg, cfg, form):
    h = pkg.ScanToMap(sort_scan=form, **sc.handle_cfg(cfg))
    if "shard_axis" in cfg:                                 # one device holding the whole map, as tests/test_gpu_sharded.py does
        h.set_global_grid([0.0, 0.0, 0.0], [64, 64, 64])
        h.set_shard(cfg["shard_axis"], 0, 64)
    return h


def _check_segments(perm, scans):
    """Every scan's segment of perm is a permutation of its own index range."""
    base = 0
    for s in scans:
        seg = np.sort(perm[base:base + len(s)])
        assert np.array_equal(seg, np.arange(base, base + len(s))), f"segment of the scan at {base} is no permutation of its range"
        base += len(s)


def _compare(name, got, scans):
    srt, perm, xyz = got
    want_perm, want_soa = _expected(name)
    assert srt is True
    assert perm.shape == want_perm.shape and xyz.shape == want_soa.shape
    _check_segments(perm, scans)
    bad = np.nonzero(perm != want_perm)[0]
    assert len(bad) == 0, f"{name}: {len(bad)} of {len(perm)} positions differ, first at {bad[0]}: {perm[bad[0]]} for {want_perm[bad[0]]}"
    assert np.array_equal(xyz.view(np.uint32), want_soa), f"{name}: the SoA is not the records gathered by the permutation"


def _upload(pkg, h, scans, stride):
    """stride 12: the caller's host arrays; stride 32: records already in device memory, sorted in place (returns their owner)."""
    if stride == 12:
        h.batch_upload(scans)
        return None
    n = sum(len(s) for s in scans)
    rec = np.full((max(n, 1), stride // 4), np.nan, np.float32)         # (whatever lies beside x, y, z is never read as a coordinate)
    rec[:n, :3] = np.concatenate(scans)
    rec[:, 4] = 7.0
    dev = pkg.DeviceBuffer(rec)
    h.batch_upload_raw(dev.ptr, [len(s) for s in scans], stride, asynchronous=False)
    return dev


def _run_case(pkg, name, stride=12):
    scans, cfg, _ = sc.build_case(name)
    perms = {}
    for form in cfg["forms"]:
        h = _handle(pkg, cfg, form)
        keep = [_upload(pkg, h, scans, stride)]
        first = h.debug_scan_order()
        _compare(name, first, scans)
        keep.append(_upload(pkg, h, scans, stride))         # a second upload on the same handle: the same arrays
        again = h.debug_scan_order()
        assert again[0] is True and np.array_equal(again[1], first[1])
        assert np.array_equal(again[2].view(np.uint32), first[2].view(np.uint32))
        perms[form] = first[1]
        h.close()
        for d in keep:
            if d is not None:
                d.close()
    if len(perms) == 2:
        assert np.array_equal(perms[2], perms[3]), f"{name}: the two forms of the sort disagree"


@pytest.mark.parametrize("name", sc.NAMES)
def test_permutation_equals_the_restatement(pkg, name):
    _run_case(pkg, name)


@pytest.mark.parametrize("name", ["size_ragged", "nonfinite_single", "shard_1"])
def test_records_sorted_in_place_in_device_memory(pkg, name):
    """Stride 32 with the batch already in this device's memory: the sort reads the caller's records where they are."""
    _run_case(pkg, name, stride=32)


def test_unsorted_batch_reports_no_permutation(pkg):
    (scan,), _, _ = sc.build_case("pass2")
    h = pkg.ScanToMap(sort_scan=0)
    h.batch_upload([scan])
    srt, perm, _ = h.debug_scan_order()
    assert srt is False and perm is None
    lib = pkg.load_library()
    raw = np.full(len(scan), -7, np.int32)
    flag = C.c_int32(5)
    assert lib.lio_s2m_debug_scan_order(h.h, raw.ctypes.data, None, len(scan), C.byref(flag)) == len(scan)
    assert flag.value == 0 and np.all(raw == -7)            # nothing copied
    # the size query, and what the hook refuses
    assert lib.lio_s2m_debug_scan_order(h.h, None, None, 0, None) == len(scan)
    assert lib.lio_s2m_debug_scan_order(h.h, raw.ctypes.data, None, len(scan) - 1, None) == -1          # LIO_ERR_ARG
    assert lib.lio_s2m_debug_scan_order(None, None, None, 0, None) == -1
    h.close()


def test_the_loop_consumes_the_pinned_order(pkg, small_case):
    """Ties the hook to what the Gauss-Newton loop reads, as test_oversized_tiles_are_ordered_deterministically does: with one
    tile per scan the pinned permutation is the identity and the registration reproduces the unsorted one bit for bit, under both
    forms; with 4 m tiles the permutation is the restatement's, both forms and a second run give the same bits, and against the
    unsorted run only the order of the fp64 sums differs: the same iteration counts, poses within 1e-5 (a few fp32 spacings of
    a pose component; the sums themselves agree to ~1e-16 relative)."""
    qs = small_case["queries"]
    scans = [np.ascontiguousarray(q["scan"][:, :3], np.float32) for q in qs]
    poses0 = np.stack([q["pose_init"] for q in qs])
    total = sum(len(s) for s in scans)
    outs = {}
    for key, cfg in (("unsorted", dict(sort_scan=0)), ("one_tile_2", dict(sort_scan=2, tile_size=1.0e4)),
                     ("one_tile_3", dict(sort_scan=3, tile_size=1.0e4)), ("tiles_2", dict(sort_scan=2)),
                     ("tiles_2_again", dict(sort_scan=2)), ("tiles_3", dict(sort_scan=3))):
        s = pkg.ScanToMap(**cfg)
        s.set_map(small_case["map"])
        s.batch_upload(scans)
        srt, perm, xyz = s.debug_scan_order()
        s.batch_set_poses(poses0); s.batch_run()
        p, r = s.batch_results()
        outs[key] = (srt, perm, p, [np.array(x.AtA, np.float32).view(np.uint32) for x in r], [x.iters for x in r])
        s.close()
    assert outs["unsorted"][0] is False
    for key in ("one_tile_2", "one_tile_3"):
        assert outs[key][0] is True and np.array_equal(outs[key][1], np.arange(total))
        assert np.array_equal(outs[key][1], so.batch_perm(scans, 1.0e4))
        np.testing.assert_array_equal(outs[key][2], outs["unsorted"][2])
        for a, b in zip(outs[key][3], outs["unsorted"][3]):
            np.testing.assert_array_equal(a, b)
    want = so.batch_perm(scans, 4.0)
    assert not np.array_equal(want, np.arange(total))
    for key in ("tiles_2", "tiles_2_again", "tiles_3"):
        assert np.array_equal(outs[key][1], want)
        np.testing.assert_array_equal(outs[key][2], outs["tiles_2"][2])
        for a, b in zip(outs[key][3], outs["tiles_2"][3]):
            np.testing.assert_array_equal(a, b)
    assert outs["tiles_2"][4] == outs["unsorted"][4]
    np.testing.assert_allclose(outs["tiles_2"][2], outs["unsorted"][2], atol=1e-5)
