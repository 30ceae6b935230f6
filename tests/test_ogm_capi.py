"""The occupancy grid's part of the C ABI without a GPU: the library exports the symbols, the two ctypes structs match gcc's
layout of include/liogpu.h, the defaults are the draft's literals, and what can be refused before a device is touched is
refused."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in ("lio_radius_filter", "lio_ogm_default_config", "lio_occupancy_grid", "lio_kf_store_occupancy_grid"):
        assert hasattr(lib, name), name
    for name in ("OgmConfig", "OgmInfo", "ogm_default_config", "radius_filter", "occupancy_grid"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.KeyframeStore, "occupancy_grid")
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    cfg_fields = [n for n, _ in pkg.OgmConfig._fields_]
    info_fields = [n for n, _ in pkg.OgmInfo._fields_]
    lines = ['printf("%zu %zu\\n", sizeof(lio_ogm_config), sizeof(lio_ogm_info));']
    lines += [f'printf("%zu\\n", offsetof(lio_ogm_config, {n}));' for n in cfg_fields]
    lines += [f'printf("%zu\\n", offsetof(lio_ogm_info, {n}));' for n in info_fields]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert out[:2] == [C.sizeof(pkg.OgmConfig), C.sizeof(pkg.OgmInfo)]
    k = 2
    assert out[k:k + len(cfg_fields)] == [getattr(pkg.OgmConfig, n).offset for n in cfg_fields]
    k += len(cfg_fields)
    assert out[k:k + len(info_fields)] == [getattr(pkg.OgmInfo, n).offset for n in info_fields]
    assert cfg_fields == ["z_min", "z_max", "z_negative", "remove_outliers", "radius", "min_neighbors", "resolution", "whole_box"]
    assert info_fields == ["width", "height", "origin", "n_in", "n_slice", "n_inliers", "n_binned", "n_occupied", "pad"]


def test_defaults_are_the_drafts_literals(pkg):
    cfg = pkg.ogm_default_config()
    f32 = np.float32
    assert (cfg.z_min, cfg.z_max, cfg.z_negative) == (f32(0.2), f32(2.0), 0)
    assert (cfg.remove_outliers, cfg.radius, cfg.min_neighbors) == (1, f32(0.5), 10)
    assert (cfg.resolution, cfg.whole_box) == (0.05, 0)


def test_refused_before_any_device(pkg):
    """the arguments are checked first: LIO_ERR_ARG, not LIO_ERR_NO_DEVICE, on a machine without a GPU too; an empty cloud is
    LIO_OK without one"""
    lib = pkg.load_library()
    pts = np.zeros((8, 3), np.float32)
    grid = np.zeros(64, np.int8)
    info = pkg.OgmInfo()
    nan, inf = float("nan"), float("inf")

    def ogm(**kw):
        cfg = pkg.ogm_default_config(**kw)
        return lib.lio_occupancy_grid(0, pts.ctypes.data, len(pts), 12, C.byref(cfg), grid.ctypes.data, grid.size, C.byref(info))

    for kw in (dict(resolution=5e-5), dict(resolution=nan), dict(resolution=inf), dict(resolution=-0.05), dict(z_min=nan), dict(z_max=inf),
               dict(z_min=2.0, z_max=0.2), dict(z_negative=2), dict(remove_outliers=-1), dict(whole_box=2), dict(radius=0.0),
               dict(radius=-0.5), dict(radius=nan), dict(radius=inf), dict(min_neighbors=-1)):
        assert ogm(**kw) == ERR_ARG, kw
    # the filter's parameters are not looked at when it does not run: this one gets as far as the device
    assert ogm(remove_outliers=0, radius=nan) in (0, -5)       # LIO_OK, or LIO_ERR_NO_DEVICE
    n_out = C.c_size_t(7)
    out = np.zeros((8, 8), np.float32)

    def rad(radius, min_nb):
        return lib.lio_radius_filter(0, pts.ctypes.data, len(pts), 12, radius, min_nb, out.ctypes.data, 32, C.byref(n_out), None)

    for radius, min_nb in ((0.0, 1), (-1.0, 1), (nan, 1), (inf, 1), (0.5, -1)):
        assert rad(radius, min_nb) == ERR_ARG, (radius, min_nb)
    assert lib.lio_radius_filter(0, pts.ctypes.data, len(pts), 10, 0.5, 1, out.ctypes.data, 32, C.byref(n_out), None) == ERR_ARG     # stride
    assert lib.lio_radius_filter(0, pts.ctypes.data, len(pts), 12, 0.5, 1, out.ctypes.data, 16, C.byref(n_out), None) == ERR_ARG     # out stride
    # empty clouds need no device
    cfg = pkg.ogm_default_config()
    info.width = info.height = 5
    assert lib.lio_occupancy_grid(0, None, 0, 12, C.byref(cfg), grid.ctypes.data, grid.size, C.byref(info)) == 0
    assert (info.width, info.height, info.n_in, info.n_occupied) == (0, 0, 0, 0)
    assert lib.lio_radius_filter(0, None, 0, 12, 0.5, 1, None, 32, C.byref(n_out), None) == 0 and n_out.value == 0
    assert lib.lio_kf_store_occupancy_grid(None, 0.0, C.byref(cfg), None, 0, None, C.byref(info)) == ERR_ARG      # no store
