"""The median fill without a GPU: the numpy restatement of grid_map_filters' MedianFillFilter (tests/median_fill_restate.py)
pinned on the reference's own test case and on the properties the kernels rely on (box form = iterated form, the truncated
radii, which holes a closing of N iterations fills), the host program that runs the kernels' text against it, and the C ABI
(symbols, struct layouts against gcc, defaults, every refusal that comes before a device is touched)."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import median_fill_restate as R                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


def reference_case():
    """grid_map_filters/test/median_fill_filter_test.cpp: 20 x 20 at 0.02 m, ones, the bottom right 5 x 5 NaN"""
    g = np.ones((20, 20), f32)
    g[15:, 15:] = np.nan
    return g


REFERENCE_HOLES = ((0, 0), (10, 5), (2, 4), (6, 3), (11, 8), (3, 15), (10, 10))
REFERENCE_CFG = dict(fill_hole_radius=0.02, existing_value_radius=0.02, filter_existing_values=1, num_erode_dilation_iterations=4)


def test_the_reference_test_case():
    g = reference_case()
    before = R.median_fill(g, 0.02, **REFERENCE_CFG)
    corner = np.zeros((20, 20), bool)
    corner[15:, 15:] = True
    assert np.array_equal(before["fill_mask"] == 0, corner)                        # "the fill mask is all ones" outside the block
    holes = g.copy()
    for r, c in REFERENCE_HOLES:
        holes[r, c] = np.nan
    res = R.median_fill(holes, 0.02, **REFERENCE_CFG)
    assert np.array_equal(np.isnan(res["filled"]), corner)                         # NaN exactly on the 5 x 5 block
    assert np.array_equal(res["filled"][~corner], np.ones(400 - 25, f32))          # the map without the seven holes
    assert (res["fill_radius_cells"], res["existing_radius_cells"]) == (1, 1)
    assert (res["n_nan_in"], res["n_filled"], res["n_nan_out"]) == (32, 7, 25)


@pytest.mark.parametrize("n", range(6))
def test_box_form_equals_iterated_form(n):
    rng = np.random.default_rng(100 + n)
    for rows, cols in ((1, 1), (1, 7), (6, 1), (2, 2), (5, 9), (13, 11), (24, 17)):
        for density in (0.3, 0.7, 0.95):
            valid = (rng.uniform(size=(rows, cols)) < density).astype(np.uint8)
            cleaned = R.cleaned_mask(valid)
            fill = R.fill_holes(cleaned, n)
            cleaned_b, fill_b = R.masks_box_form(valid, n)
            assert np.array_equal(cleaned, cleaned_b) and np.array_equal(fill, fill_b), (rows, cols, density)


def test_n_zero_dilates_once_and_never_erodes():
    valid = np.zeros((9, 9), np.uint8)
    valid[3:6, 3:6] = 1
    assert np.array_equal(R.cleaned_mask(valid), valid)
    want = np.zeros((9, 9), np.uint8)
    want[2:7, 2:7] = 1
    assert np.array_equal(R.fill_holes(valid, 0), want)
    assert np.array_equal(R.fill_holes(valid, 1), valid)


def test_hole_widths():
    """40 x 40 at 0.2 m, N = 4, radius 1.0: square holes up to 8 wide are filled completely, a 9 x 9 hole stays NaN"""
    for w in range(1, 10):
        g = np.arange(1600, dtype=f32).reshape(40, 40)
        g[15:15 + w, 14:14 + w] = np.nan
        res = R.median_fill(g, 0.2, fill_hole_radius=1.0, num_erode_dilation_iterations=4)
        assert res["fill_radius_cells"] == 5
        assert res["n_nan_out"] == (81 if w == 9 else 0), w
        assert res["n_filled"] == (0 if w == 9 else w * w), w


def test_radii_truncate():
    assert R.radius_cells(0.6, 0.2) == 2 and R.radius_cells(0.3, 0.1) == 2
    assert R.radius_cells(0.05, 0.02) == 2 and R.radius_cells(1.0, 0.2) == 5 and R.radius_cells(0.0, 0.2) == 0


def test_median_conventions():
    g = np.array([[np.nan, 3.0, 1.0], [2.0, 4.0, np.inf]], f32)
    assert R.median_bits(g, 0, 0, 2) == int(f32(3.0).view(u32))                    # four finite values: the upper median
    assert R.median_bits(g, 0, 0, 0) == R.QNAN_BITS                                # an empty window
    z = np.array([[np.nan, -0.0, 0.0]], f32)
    assert R.median_bits(z, 0, 0, 2) == 0x00000000                                 # -0 sorts below +0: position 1 of 2 is +0
    z = np.array([[np.nan, 0.0, -0.0, -0.0]], f32)
    assert R.median_bits(z, 0, 0, 3) == 0x80000000
    g = np.array([[np.nan, 1.0]], f32)
    g.view(u32)[0, 0] = 0x7fc12345
    res = R.median_fill(g, 1.0, fill_hole_radius=1.0, mask_in=np.zeros((1, 2), f32))
    assert res["filled"].view(u32)[0, 0] == 0x7fc12345                             # an unmasked cell: the bits copied


HOST_CASES = [(1, 1, 1, 4, 0), (1, 40, 2, 4, 0), (40, 1, 2, 1, 1), (2, 2, 1, 0, 0), (32, 8, 2, 4, 1), (33, 9, 5, 1, 0), (69, 19, 2, 4, 1),
              (69, 19, 5, 15, 0), (80, 70, 32, 4, 0)]


def test_host_program_runs_the_same_bits():
    """tools/median_fill_host_check.cpp runs csrc/lio_medianfill.h -- the text the kernels run -- on the host: its own cases
    against its plain second implementation with no read outside a window, and its `case` mode against the restatement"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "median_fill_host_check")
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                               os.path.join(ROOT, "tools", "median_fill_host_check.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip().endswith("out-of-range accesses: 0, mismatches: 0"), out.stdout[-400:]
        for rows, cols, radius, n, filt in HOST_CASES:
            g = R.make_grid(rows, cols, seed=rows * 100 + cols)
            g.T.tofile(os.path.join(d, "in.f32"))                                  # column-major
            res = 0.2
            want = R.median_fill(g, res, fill_hole_radius=(radius + 0.5) * res, existing_value_radius=2.5 * res, filter_existing_values=filt,
                                 num_erode_dilation_iterations=n)
            assert want["fill_radius_cells"] == radius
            got = subprocess.check_output([exe, "case", str(rows), str(cols), repr(res), repr((radius + 0.5) * res), repr(2.5 * res), str(filt),
                                           str(n), os.path.join(d, "in.f32")], text=True).split()
            assert (int(got[1], 16), int(got[3])) == (R.checksum(want), 0), (rows, cols, radius, n, filt)
        g = R.make_grid(33, 9, seed=5)
        m = (np.random.default_rng(6).uniform(size=g.shape) < 0.5).astype(f32)
        g.T.tofile(os.path.join(d, "in.f32"))
        m.T.tofile(os.path.join(d, "mask.f32"))
        want = R.median_fill(g, 0.2, fill_hole_radius=0.5, existing_value_radius=0.3, filter_existing_values=1, mask_in=m)
        got = subprocess.check_output([exe, "case", "33", "9", "0.2", "0.5", "0.3", "1", "4", os.path.join(d, "in.f32"),
                                       os.path.join(d, "mask.f32")], text=True).split()
        assert (int(got[1], 16), int(got[3])) == (R.checksum(want), 0)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in ("lio_median_fill_default_config", "lio_median_fill", "lio_kf_store_planning_map"):
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    structs = (("lio_median_fill_config", pkg.MedianFillConfig), ("lio_median_fill_info", pkg.MedianFillInfo),
               ("lio_planning_map_buffers", pkg.PlanningMapBuffers))
    lines, want = [], []
    for cname, cls in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(cls))
        for n, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {n}));')
            want.append(getattr(cls, n).offset)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert out == want


def test_defaults_are_the_constructor_s(pkg):
    cfg = pkg.median_fill_default_config()
    assert (cfg.fill_hole_radius, cfg.existing_value_radius, cfg.filter_existing_values, cfg.num_erode_dilation_iterations) == (0.05, 0.0, 0, 4)


def test_refused_before_any_device(pkg):
    """the configuration is checked first: LIO_ERR_ARG, not LIO_ERR_NO_DEVICE, on a machine without a GPU too; an empty grid
    is LIO_OK without one"""
    lib = pkg.load_library()
    grid = np.zeros((4, 5), f32, order="F")
    out = np.zeros((4, 5), f32, order="F")
    info = pkg.MedianFillInfo()
    call = lambda cfg, res=0.2, g=grid.ctypes.data, o=out.ctypes.data, i=C.byref(info), rows=4, cols=5: lib.lio_median_fill(
        0, g, rows, cols, res, None if cfg is None else C.byref(cfg), None, o, None, None, i)
    nan, inf = float("nan"), float("inf")
    for kw, why in ((dict(fill_hole_radius=-0.1), b"radii"), (dict(fill_hole_radius=nan), b"radii"), (dict(existing_value_radius=-1.0), b"radii"),
                    (dict(existing_value_radius=inf), b"radii"), (dict(filter_existing_values=2), b"filter_existing_values"),
                    (dict(filter_existing_values=-1), b"filter_existing_values"), (dict(num_erode_dilation_iterations=-1), b"iterations"),
                    (dict(num_erode_dilation_iterations=16), b"iterations"), (dict(fill_hole_radius=0.2 * 33.0), b"32 cells"),
                    (dict(existing_value_radius=0.2 * 33.5), b"32 cells")):
        assert call(pkg.median_fill_default_config(**kw)) == -1, kw
        assert why in lib.lio_last_error(), (kw, lib.lio_last_error())
    cfg = pkg.median_fill_default_config()
    for res in (5e-5, nan, inf, -0.2):
        assert call(cfg, res=res) == -1 and b"resolution" in lib.lio_last_error(), res
    for kw in (dict(cfg=None), dict(cfg=cfg, g=None), dict(cfg=cfg, o=None), dict(cfg=cfg, i=None)):
        assert call(**kw) == -1 and b"null" in lib.lio_last_error(), kw
    assert call(cfg, rows=-1) == -1
    assert call(cfg, rows=1 << 16, cols=1 << 15) == -3 and b"2^31" in lib.lio_last_error()                   # LIO_ERR_CAPACITY
    # the widest settings that are not refused get as far as the device check (or run, where there is one)
    assert call(pkg.median_fill_default_config(fill_hole_radius=0.2 * 32.9, num_erode_dilation_iterations=15)) != -1
    info = pkg.MedianFillInfo()
    cfg = pkg.median_fill_default_config(fill_hole_radius=0.6, existing_value_radius=0.3)
    assert lib.lio_median_fill(0, None, 0, 5, 0.2, C.byref(cfg), None, None, None, None, C.byref(info)) == 0
    assert (info.rows, info.cols, info.fill_radius_cells, info.existing_radius_cells) == (0, 5, 2, 1)
    assert lib.lio_median_fill(0, None, 0, 5, 0.1, C.byref(cfg), None, None, None, None, C.byref(info)) == 0
    assert (info.fill_radius_cells, info.existing_radius_cells) == (5, 2)          # 0.6 / 0.1 = 5.999.., 0.3 / 0.1 = 2.999..


def test_planning_map_refused_before_any_device(pkg):
    """the chained call refuses a configuration as the stage's own call does, and a null argument, before the store is read"""
    lib = pkg.load_library()
    lm, hm = pkg.local_map_default_config(), pkg.height_map_default_config()
    pose = (C.c_float * 6)()
    st = C.c_void_p(1)                                         # never dereferenced: every call below is refused first
    call = lambda hm=hm, fill=None, terrain=None, sdf=None, sdf_cfg=None, st=st: lib.lio_kf_store_planning_map(
        st, C.byref(lm), pose, C.byref(hm), None if fill is None else C.byref(fill), None if terrain is None else C.byref(terrain), sdf,
        None if sdf_cfg is None else C.byref(sdf_cfg), None, None, None, None, None, None)
    assert call(st=None) == -1 and b"null" in lib.lio_last_error()
    assert call(hm=pkg.height_map_default_config(fill_holes=2)) == -1
    assert call(fill=pkg.median_fill_default_config(num_erode_dilation_iterations=16)) == -1 and b"iterations" in lib.lio_last_error()
    assert call(fill=pkg.median_fill_default_config(fill_hole_radius=0.2 * 33)) == -1 and b"32 cells" in lib.lio_last_error()
    assert call(terrain=pkg.terrain_default_config(normal_axis=3)) == -1 and b"normal_axis" in lib.lio_last_error()
    assert call(sdf=C.c_void_p(1)) == -1 and b"null" in lib.lio_last_error()       # an sdf without its configuration
    assert call(sdf=C.c_void_p(1), sdf_cfg=pkg.sdf_default_config(nan_policy=2)) == -1 and b"nan_policy" in lib.lio_last_error()
