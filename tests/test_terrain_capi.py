"""The terrain layers' part of the C ABI without a GPU: the library exports the three symbols, the two ctypes structs match
gcc's layout of include/liogpu.h, the defaults are the yaml's literals, and what can be refused before a device is touched
is refused."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in ("lio_terrain_default_config", "lio_terrain_layers", "lio_kf_store_terrain_map"):
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    cfg_fields = [n for n, _ in pkg.TerrainConfig._fields_]
    info_fields = [n for n, _ in pkg.TerrainInfo._fields_]
    lines = ['printf("%zu %zu\\n", sizeof(lio_terrain_config), sizeof(lio_terrain_info));']
    lines += [f'printf("%zu\\n", offsetof(lio_terrain_config, {n}));' for n in cfg_fields]
    lines += [f'printf("%zu\\n", offsetof(lio_terrain_info, {n}));' for n in info_fields]
    lines += ['printf("%d %d %d\\n", LIO_TERRAIN_SMOOTH, LIO_TERRAIN_TRAVERSABILITY, LIO_TERRAIN_N_LAYERS);']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert out[:2] == [C.sizeof(pkg.TerrainConfig), C.sizeof(pkg.TerrainInfo)]
    k = 2
    assert out[k:k + len(cfg_fields)] == [getattr(pkg.TerrainConfig, n).offset for n in cfg_fields]
    k += len(cfg_fields)
    assert out[k:k + len(info_fields)] == [getattr(pkg.TerrainInfo, n).offset for n in info_fields]
    assert out[-3:] == [0, 7, 8] and len(pkg.TERRAIN_LAYERS) == 8


def test_defaults_are_the_yaml_literals(pkg):
    cfg = pkg.terrain_default_config()
    assert (cfg.normal_method, cfg.normal_axis, cfg.normal_radius, cfg.smooth_radius) == (0, 2, 0.05, 0.06)
    assert (cfg.edge_window_size, cfg.edge_window_length) == (0, 0.05)
    f32 = np.float32
    assert (cfg.slope_critical, cfg.roughness_critical, cfg.slope_weight, cfg.roughness_weight) == (f32(0.6), f32(0.1), f32(0.5), f32(0.5))
    assert cfg.layers == 0xff


def test_plans_and_refusals_are_the_recorded_ones(pkg):
    """lio_terrain_check's answers on a grid of no rows (it returns before any device is touched): the return code with the
    message of a refusal, or (edge_window_size, normal_method_used) of the plan.  The literals were recorded from the library
    before the window and the halo came from lio_gridfilter.h's plans: the limits (a window of 65, a radius of 32 cells), the
    texts and the order of the checks are the terrain layers' own."""
    lib = pkg.load_library()
    nan, inf, R = float("nan"), float("inf"), 0.25
    up = math.nextafter(32 * R, inf)
    RES, ODD = "resolution must be at least 1e-4", "edge_window_size must be odd (0: from edge_window_length)"
    LEN = "radii and the window length must be finite and not negative"
    WIN, RAD = "the edge window reaches further than 32 cells", "a radius reaches further than 32 cells"
    table = [
        (nan, {}, RES), (inf, {}, RES), (5e-5, {}, RES),
        (1e-4, {}, WIN),                                        # the default length of 0.05 is 500 cells there
        (R, dict(edge_window_size=-1), ODD), (R, dict(edge_window_size=2), ODD),
        (R, dict(edge_window_size=1), (1, 0)),
        (R, dict(edge_window_size=3, edge_window_length=1e30), (3, 0)),                     # an explicit size: the length is not read
        (R, dict(edge_window_size=65), (65, 0)), (R, dict(edge_window_size=67), WIN),
        (R, dict(edge_window_length=nan), LEN), (R, dict(edge_window_length=-1.0), LEN),
        (R, dict(edge_window_length=0.0), (1, 0)), (R, dict(edge_window_length=0.75), (3, 0)),
        (R, dict(edge_window_length=64 * R), (65, 0)),          # 64 cells: the next odd size
        (R, dict(edge_window_length=65 * R), (65, 0)),
        (R, dict(edge_window_length=65.5 * R), WIN),            # rounds to 66 cells
        (R, dict(edge_window_length=66 * R), WIN), (R, dict(edge_window_length=1e30), WIN),
        (R, dict(normal_radius=32 * R, smooth_radius=32 * R), (1, 0)),
        (R, dict(smooth_radius=up), RAD), (R, dict(normal_radius=up), RAD),
        (R, dict(normal_method=1, normal_radius=up), (1, 0)),   # the raster normals read no radius
        (R, dict(normal_radius=0.0), (1, 1)),                   # the fallback to raster
        (R, dict(normal_radius=nan), LEN),
        (R, dict(edge_window_size=2, smooth_radius=up), ODD),   # the window is asked before the radii
        (R, dict(edge_window_size=67, smooth_radius=up), WIN),
    ]
    ln, ps = (C.c_double * 2)(0.0, 5 * R), (C.c_double * 2)(0.0, 0.0)
    info = pkg.TerrainInfo()
    for res, kw, want in table:
        cfg = pkg.terrain_default_config(**kw)
        rc = lib.lio_terrain_layers(0, None, 0, 5, res, ln, ps, C.byref(cfg), None, 0, C.byref(info))
        if isinstance(want, str):
            assert (rc, lib.lio_last_error().decode()) == (-1, want), (res, kw)
        else:
            assert (rc, info.edge_window_size, info.normal_method_used) == (0,) + want, (res, kw)


def test_refused_before_any_device(pkg):
    """the configuration is checked first: LIO_ERR_ARG, not LIO_ERR_NO_DEVICE, on a machine without a GPU too; an empty grid
    is LIO_OK without one"""
    lib = pkg.load_library()
    grid = np.zeros((4, 5), np.float32, order="F")
    ln, ps = (C.c_double * 2)(4 * 0.2, 5 * 0.2), (C.c_double * 2)(0.0, 0.0)
    info = pkg.TerrainInfo()
    out = np.zeros(8 * 20, np.float32)
    for kw in (dict(normal_method=2), dict(normal_axis=3), dict(smooth_radius=-0.1), dict(edge_window_size=4), dict(layers=0x100),
               dict(smooth_radius=0.2 * 32.5), dict(slope_weight=float("nan"))):
        cfg = pkg.terrain_default_config(**kw)
        assert lib.lio_terrain_layers(0, grid.ctypes.data, 4, 5, 0.2, ln, ps, C.byref(cfg), out.ctypes.data, out.size, C.byref(info)) == -1, kw
    cfg = pkg.terrain_default_config()
    assert lib.lio_terrain_layers(0, grid.ctypes.data, 4, 5, 5e-5, ln, ps, C.byref(cfg), out.ctypes.data, out.size, C.byref(info)) == -1
    assert lib.lio_terrain_layers(0, grid.ctypes.data, 4, 5, 0.2, ln, ps, C.byref(cfg), out.ctypes.data, 8 * 20 - 1, C.byref(info)) == -1
    assert (info.rows, info.cols) == (4, 5)                    # too small a buffer: the size comes back
    assert lib.lio_terrain_layers(0, None, 0, 5, 0.2, ln, ps, C.byref(cfg), out.ctypes.data, out.size, C.byref(info)) == 0
    assert (info.rows, info.cols, info.edge_window_size) == (0, 5, 1)
