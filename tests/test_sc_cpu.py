"""Scan Context loop detection, the part that needs no GPU: the ABI (symbols, struct layouts, defaults, refused configs, the
no-device answer) and the numpy restatement (tests/sc_restate.py) against closed forms."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sc_restate as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SC_SYMBOLS = ["lio_sc_default_config", "lio_sc_make", "lio_sc_distance", "lio_kf_store_sc_add", "lio_kf_store_sc_add_device",
              "lio_kf_store_sc_add_from_handle", "lio_kf_store_sc_count", "lio_kf_store_sc_geometry", "lio_kf_store_sc_get", "lio_kf_store_sc_detect"]


def polar_cloud(cells, R_=20, S=60, max_radius=80.0, turn=0):
    """One point per (ring, sector, z) at the centre of the cell, the whole cloud turned by `turn` sectors about z."""
    pts = []
    for r, s, z in cells:
        rad = (r + 0.5) * max_radius / R_
        ang = np.radians((s + 0.5 + turn) * 360.0 / S)
        pts.append([rad * np.cos(ang), rad * np.sin(ang), z])
    return np.array(pts, np.float32).reshape(-1, 3)


def random_cells(seed, n=400):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, 20)), int(rng.integers(0, 60)), float(rng.uniform(-1.5, 6.0))) for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_the_library_exports_the_scan_context_symbols(pkg):
    lib = pkg.load_library()
    api = __import__("importlib").import_module("lio-slam_amd.api")
    hdr = open(os.path.join(ROOT, "include", "liogpu.h")).read()
    for name in SC_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS and name + "(" in hdr.replace(" (", "(")


def test_sc_struct_layouts_match_c(pkg):
    fields_c = ["max_radius", "lidar_height", "search_ratio", "dist_thres", "num_rings", "num_sectors", "num_exclude_recent",
                "num_candidates", "tree_period"]
    fields_r = ["status", "loop_id", "align", "nn_idx", "n_searched", "n_candidates", "yaw_diff_rad", "min_dist", "cand_idx",
                "cand_ring_d2", "cand_dist", "cand_align"]
    lines = ['printf("%zu %zu %d\\n", sizeof(lio_sc_config), sizeof(lio_sc_result), LIO_SC_MAX_CANDIDATES);']
    lines += [f'printf("%zu\\n", offsetof(lio_sc_config, {f}));' for f in fields_c]
    lines += [f'printf("%zu\\n", offsetof(lio_sc_result, {f}));' for f in fields_r]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    api = __import__("importlib").import_module("lio-slam_amd.api")
    assert out[:3] == [C.sizeof(pkg.ScConfig), C.sizeof(pkg.ScResult), api.SC_MAX_CANDIDATES]
    assert out[3:3 + len(fields_c)] == [getattr(pkg.ScConfig, f).offset for f in fields_c]
    assert out[3 + len(fields_c):] == [getattr(pkg.ScResult, f).offset for f in fields_r]


def test_sc_defaults_are_the_reference_constants(pkg):
    c = pkg.sc_default_config()
    assert (c.num_rings, c.num_sectors, c.max_radius, c.lidar_height) == (20, 60, 80.0, 2.0)            # Scancontext.h:80-84
    assert (c.num_exclude_recent, c.num_candidates, c.search_ratio, c.dist_thres, c.tree_period) == (30, 3, 0.1, 0.3, 10)
    for k, v in R.DEFAULTS.items():
        assert getattr(c, k) == v


def test_out_of_range_sc_configs_are_refused_before_any_device(pkg):
    import torch
    lib = pkg.load_library()
    cloud = np.ones((8, 3), np.float32)
    desc = np.zeros(4096, np.float32)
    bad = [("num_rings", 0), ("num_rings", 257), ("num_sectors", 0), ("num_sectors", 257), ("max_radius", 0.0), ("max_radius", float("inf")),
           ("lidar_height", float("nan")), ("search_ratio", -0.1), ("search_ratio", 1.5), ("dist_thres", float("nan")),
           ("num_exclude_recent", -1), ("num_candidates", 0), ("num_candidates", 17), ("tree_period", 0)]
    for field, v in bad:
        cfg = pkg.sc_default_config(**{field: v})
        assert lib.lio_sc_make(0, cloud.ctypes.data, 8, 12, C.byref(cfg), desc.ctypes.data, None, None) == -1, (field, v)
    cfg = pkg.sc_default_config(num_rings=100, num_sectors=100)                   # 10 000 cells: beyond the LDS layout
    assert lib.lio_sc_make(0, cloud.ctypes.data, 8, 12, C.byref(cfg), desc.ctypes.data, None, None) == -1
    assert b"LIO_SC_MAX_CELLS" in lib.lio_last_error()
    cfg = pkg.sc_default_config()
    assert lib.lio_sc_make(0, cloud.ctypes.data, 8, 10, C.byref(cfg), desc.ctypes.data, None, None) == -1   # the stride
    assert lib.lio_sc_make(0, cloud.ctypes.data, 8, 12, None, desc.ctypes.data, None, None) == -1
    if not torch.cuda.is_available():                                             # no CPU fallback
        with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
            pkg.sc_make(cloud)
        with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
            pkg.sc_distance(np.zeros((20, 60)), np.zeros((20, 60)))


# ------------------------------------------------------------------------------------------------- the restatement
def test_hand_placed_points_land_in_the_cells_worked_out_by_hand():
    pts = np.array([
        [10.0, 0.0, 1.0],        # range 10 -> ceil(2.5) = ring 3; angle 0 -> ceil(0) = 0 -> clamped to sector 1
        [0.0, 10.0, -0.5],       # angle 90 -> ceil(15) = sector 15; z + 2 = 1.5
        [-3.0, 0.0, 0.25],       # range 3 -> ring 1; angle 180 - 0 -> ceil(30) = sector 30
        [0.0, -4.0, 3.0],        # range 4 -> ceil(1.0) = ring 1; angle 360 - 90 = 270 -> sector 45
        [1e-3, 1e-3, 0.0],       # range 1.4e-3 -> ceil(3.5e-4) = ring 1; angle 45 -> ceil(7.5) = sector 8
        [80.0, 0.0, 5.0],        # range exactly 80: kept (only > 80 is dropped) -> ring 20, sector 1
        [80.001, 0.0, 9.0],      # dropped
        [56.0, -56.0, 2.0],      # range 79.196 -> ceil(19.8) = ring 20; angle 315 -> ceil(52.5) = sector 53
        [10.0, 0.0, 0.5],        # the same cell as the first, lower: the maximum stays
        [20.0, 20.0, -1002.5],   # z + 2 = -1000.5 < -1000: never taken, the cell stays empty
        [np.nan, 1.0, 1.0], [0.0, 0.0, 7.0], [np.inf, 0.0, 1.0],                  # skipped
    ], np.float32)
    d = R.make_desc(pts)
    want = np.zeros((20, 60), np.float32)
    want[2, 0] = 3.0; want[2, 14] = 1.5; want[0, 29] = 2.25; want[0, 44] = 5.0; want[0, 7] = 2.0; want[19, 0] = 7.0; want[19, 52] = 4.0
    np.testing.assert_array_equal(d, want)
    np.testing.assert_array_equal(R.ring_key(d)[[0, 2, 19]], np.array([9.25 / 60, 4.5 / 60, 11.0 / 60], np.float32))
    assert R.sector_key(d)[0] == 10.0 / 20 and R.sector_key(d)[52] == 4.0 / 20
    assert R.make_desc(np.zeros((0, 3), np.float32)).sum() == 0


def test_a_turn_by_k_sectors_is_found_as_align_k():
    cells = random_cells(5)
    base = R.make_desc(polar_cloud(cells))
    for k in (0, 1, 7, 29, 30, 59):
        turned = R.make_desc(polar_cloud(cells, turn=k))
        np.testing.assert_array_equal(turned, np.roll(base, k, axis=1))
        dist, align, _ = R.distance(turned, base)
        assert align == k and abs(dist) < 1e-6, (k, align, dist)


def test_a_descriptor_against_itself():
    d = R.make_desc(polar_cloud(random_cells(6)))
    dist, align, info = R.distance(d, d)
    assert align == 0 and abs(dist) < 1e-15
    assert info["shifts"] == [0, 1, 2, 3, 57, 58, 59]                             # +- round(0.5 * 0.1 * 60) around 0, sorted


def test_all_zero_columns_are_skipped_and_no_common_column_never_wins():
    a = np.zeros((20, 60)); b = np.zeros((20, 60))
    a[:, :10] = 1.0; b[:, :10] = 1.0
    b[:, 30:40] = 5.0                                        # columns a does not have: skipped, not counted as dissimilar
    assert abs(R.dist_direct(a, b)) < 1e-15
    b2 = np.zeros((20, 60)); b2[:, 30:40] = 1.0
    assert np.isnan(R.dist_direct(a, b2))                    # no common non-zero column at shift 0: 0 / 0
    m = R.Manager(num_exclude_recent=1, num_candidates=2)
    good = R.make_desc(polar_cloud(random_cells(7)))
    empty = np.zeros((20, 60), np.float32)
    m.add(empty); m.add(good); m.add(good.copy()); m.add(good.copy())
    out = m.detect()
    assert out["n_searched"] == 3 and R.distance(good, empty)[0] == 10000000.0    # every shift NaN: the initial value stays
    assert out["loop_id"] in (1, 2) and out["min_dist"] < 1e-12
    # a query with nothing in common with any candidate: every distance is NaN, nothing wins, no loop
    m2 = R.Manager(num_exclude_recent=1, num_candidates=2)
    m2.add(empty); m2.add(empty); m2.add(good)
    out2 = m2.detect()
    assert out2["loop_id"] == -1 and out2["min_dist"] == 10000000.0 and out2["nn_idx"] == 0 and out2["yaw"] == 0
    assert out2["cand_dist"] == [10000000.0, 10000000.0]


def test_the_prefix_goes_stale_between_rebuilds_and_too_few_descriptors_report_none():
    m = R.Manager(num_exclude_recent=3, tree_period=3, num_candidates=2)
    rng = np.random.default_rng(8)
    for _ in range(3):
        m.add(rng.uniform(0, 5, (20, 60)).astype(np.float32))
    assert m.detect()["loop_id"] == -1 and m.counter == 0    # 3 < 3 + 1: returns before the counter
    seen = []
    for _ in range(5):
        m.add(rng.uniform(0, 5, (20, 60)).astype(np.float32))
        seen.append(m.detect()["n_searched"])
    assert seen == [1, 1, 1, 4, 4]                           # rebuilt at calls 0 and 3


def test_candidates_are_ordered_by_distance_then_index():
    m = R.Manager(num_exclude_recent=1, num_candidates=3)
    a = np.zeros((20, 60), np.float32); a[0, :] = 1.0
    b = np.zeros((20, 60), np.float32); b[0, :] = 3.0
    for d in (b, a, b, a, a * 1.5):                          # ring keys (ring 0): 3, 1, 3, 1 and the query 1.5
        m.add(d)
    out = m.detect()
    assert out["cand_idx"] == [1, 3, 0]                      # the tie at 0.25 goes to the lower index, then 2.25 twice likewise
    assert out["cand_d2"] == [np.float32(0.25), np.float32(0.25), np.float32(2.25)]
    assert R.c_round(0.5 * 0.1 * 60) == 3 and R.c_round(2.5) == 3 and R.c_round(2.4999) == 2
