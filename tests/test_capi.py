"""C-ABI surface checks that need no GPU: the library loads, exports every
symbol include/liogpu.h declares, the ctypes structs match the C layout, and
the product fails loudly (no CPU fallback) when no device is present."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "liogpu.h")).read()
    declared = set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"lio_s2m_handle"}
    assert len(declared) >= 28
    api = __import__("importlib").import_module("lio-slam_amd.api")
    assert declared == set(api.EXPORTS), declared ^ set(api.EXPORTS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} is declared in include/liogpu.h but not exported"
    assert lib.lio_version() == 102


def test_struct_layouts_match_c(pkg):
    """sizeof/offsetof of the ABI structs as seen by gcc == the ctypes mirrors."""
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "liogpu.h"
    int main(void) {
        printf("%zu %zu %zu %zu\n", sizeof(lio_s2m_config), sizeof(lio_s2m_result), sizeof(lio_s2m_profile), sizeof(lio_deskew_config));
        printf("%zu %zu %zu %zu\n", offsetof(lio_s2m_config, plane_tol), offsetof(lio_s2m_config, cell_div),
               offsetof(lio_s2m_result, pose_iter), offsetof(lio_s2m_profile, point_iters));
        printf("%zu %zu %zu %zu\n", sizeof(lio_feature_config), sizeof(lio_range_image_config),
               offsetof(lio_s2m_config, nn_cache), offsetof(lio_range_image_config, lidarMaxRange));
        printf("%zu %zu\n", offsetof(lio_s2m_profile, persist_fallbacks), offsetof(lio_s2m_profile, multi_stream_syncs));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe], text=True).split()
    sizes = [int(v) for v in out]
    assert sizes[:4] == [C.sizeof(pkg.S2MConfig), C.sizeof(pkg.S2MResult), C.sizeof(pkg.S2MProfile), C.sizeof(pkg.DeskewConfig)]
    assert sizes[4:8] == [pkg.S2MConfig.plane_tol.offset, pkg.S2MConfig.cell_div.offset,
                          pkg.S2MResult.pose_iter.offset, pkg.S2MProfile.point_iters.offset]
    assert sizes[8:12] == [C.sizeof(pkg.FeatureConfig), C.sizeof(pkg.RangeImageConfig),
                           pkg.S2MConfig.nn_cache.offset, pkg.RangeImageConfig.lidarMaxRange.offset]
    assert sizes[12:] == [pkg.S2MProfile.persist_fallbacks.offset, pkg.S2MProfile.multi_stream_syncs.offset]


def test_defaults_are_the_reference_literals(pkg):
    cfg = pkg.S2MConfig()
    pkg.load_library().lio_s2m_default_config(C.byref(cfg))
    assert (cfg.k, cfg.max_sq_dist, cfg.plane_tol, cfg.weight, cfg.min_s) == (5, 1.0, 0.2, 0.9, 0.1)   # MO:1631-1679
    assert (cfg.min_corr, cfg.max_iters, cfg.eig_thresh, cfg.conv_deg, cfg.conv_cm) == (50, 30, 100.0, 0.05, 0.05)
    assert cfg.min_scan_pts == 30 and cfg.jacobian_mode == 0 and cfg.force_all_iters == 0
    d = pkg.deskew_default_config()
    assert (d.N_SCAN, d.downsampleRate, d.point_filter_num) == (16, 1, 3)                               # UT:275-278
    assert (d.lidarMinFront, d.lidarMinBack, d.lidarMinLeft, d.lidarMinRight) == (1.0, 5.0, 2.0, 2.0)   # UT:280-283


def test_no_cpu_fallback(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
        pkg.ScanToMap()
    rec = pkg.pack_xyzirt(np.ones((4, 3), np.float32), np.ones(4), np.zeros(4), np.zeros(4))
    none = (0, np.zeros(2000), np.zeros(2000), np.zeros(2000), np.zeros(2000))
    with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
        pkg.deskew(pkg.deskew_default_config(), rec, 0.0, none)
    with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
        pkg.curvature(np.ones(100, np.float32))


def test_host_side_scalar_code_matches_oracle(pkg, oracle):
    """transformUpdate (MO:1867-1907) and imuDeskewInfo (IP:359-418) run on the
    host inside the product library; they must agree with the oracle bit for bit."""
    rng = np.random.default_rng(0)
    for _ in range(200):
        pose = rng.uniform(-1, 1, 6).astype(np.float32) * np.array([0.5, 0.5, 3, 50, 50, 5], np.float32)
        kw = dict(imu_available=int(rng.integers(0, 2)), imu_type=int(rng.integers(0, 2)),
                  imu_roll_init=float(rng.uniform(-0.5, 0.5)), imu_pitch_init=float(rng.uniform(-1.6, 1.6)),
                  imu_rpy_weight=float(rng.uniform(0, 1)), rotation_tollerance=float(rng.choice([0.1, 1000.0])),
                  z_tollerance=float(rng.choice([1.0, 1000.0])))
        np.testing.assert_array_equal(pkg.transform_update(pose, **kw), oracle.transform_update(pose, **kw))
    stamp = 5.0 + np.cumsum(rng.uniform(0.001, 0.003, 300))
    gyro = rng.normal(0, 1, (300, 3))
    a = pkg.imu_deskew_info(stamp, gyro, 5.2, 5.3)
    b = oracle.imu_deskew_info(stamp, gyro, 5.2, 5.3)
    assert a[0] == b[0] > 10
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


def test_out_of_range_config_is_refused_not_clamped(pkg, oracle):
    """k != 5 (MO:1631 hard-codes 5) and max_iters beyond the 32-entry iteration trace return LIO_ERR_ARG from
    lio_s2m_create -- before any device is touched -- and the oracle refuses the same configuration."""
    lib = pkg.load_library()
    for field, bad in (("k", 4), ("k", 6), ("max_iters", 0), ("max_iters", 33), ("max_sq_dist", 0.0)):
        cfg = pkg.S2MConfig()
        lib.lio_s2m_default_config(C.byref(cfg))
        setattr(cfg, field, bad)
        h = C.c_void_p()
        assert lib.lio_s2m_create(C.byref(cfg), C.byref(h)) == -1, (field, bad)      # LIO_ERR_ARG
        assert not h.value
    ocfg = oracle.default_config(max_iters=33)
    scan = np.zeros((100, 3), np.float32)
    _, res, _, _ = oracle.scan2map(ocfg, scan, scan, np.zeros(6, np.float32))
    assert res.status == -1


def test_bench_starts_its_own_ranks_from_the_plain_command():
    """`python bench.py --gpus 2` with no launcher -- the form the driver records -- must start its ranks itself (a child
    `python -m torch.distributed.run`), relay their exit code and never touch the GPU in the parent.  Without a GPU the ranks
    refuse to run ("no CPU fallback"), which is exactly what shows here: the parent spawned them, they said why, rc != 0."""
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("on a GPU box the same command is exercised by the gloo rehearsal (profiles/r03_bench_gloo2_selfspawn_1gpu.json)")
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "4", "--no-cpu"],
                       capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode != 0
    assert "starting 2 ranks" in p.stderr and "torch.distributed.run" in p.stderr
    assert "bench.py needs a GPU" in p.stderr
    assert p.stdout.strip() == ""                              # no JSON line without a measurement


# Entry points that return a count or a constant and allocate nothing on the C++ side: no exception can leave them.
_UNGUARDED_INT_ENTRY_POINTS = {"lio_version", "lio_kf_store_count", "lio_imu_deskew_info", "lio_s2m_debug_stamps"}


def _matching(src, i, open_ch, close_ch):
    """Index of the bracket that closes the one at src[i] (brackets inside comments and literals are skipped)."""
    depth = 0
    while True:
        if src.startswith("//", i):
            i = src.index("\n", i)
        elif src.startswith("/*", i):
            i = src.index("*/", i) + 2
        elif src[i] in "\"'":
            q, i = src[i], i + 1
            while src[i] != q:
                i += 2 if src[i] == "\\" else 1
            i += 1
        else:
            depth += (src[i] == open_ch) - (src[i] == close_ch)
            if depth == 0:
                return i
            i += 1


def test_status_entry_points_stop_exceptions():
    """include/liogpu.h promises that nothing throws: every extern "C" definition returning a status is a
    function-try-block ending in LIO_CATCH, which turns an exception into LIO_ERR_CAPACITY."""
    csrc = os.path.join(ROOT, "lio-slam_amd", "csrc")
    guarded, unguarded = set(), set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".hip"):
            continue
        src = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r'extern "C" int (lio_\w+)\s*\(', src):
            after = src[_matching(src, m.end() - 1, "(", ")") + 1:].lstrip()
            if after.startswith(";"):
                continue                                                  # a declaration
            if after.startswith("try"):
                body = src.index("{", len(src) - len(after))
                tail = src[_matching(src, body, "{", "}") + 1:].lstrip()
                if tail.startswith("LIO_CATCH"):
                    guarded.add(m.group(1))
                    continue
            unguarded.add(m.group(1))
    assert len(guarded) >= 40, sorted(guarded)
    assert unguarded == _UNGUARDED_INT_ENTRY_POINTS, unguarded ^ _UNGUARDED_INT_ENTRY_POINTS
