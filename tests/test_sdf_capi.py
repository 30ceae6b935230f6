"""The signed distance field's part of the C ABI without a GPU: the library exports the symbols, the two ctypes structs match
gcc's layout of include/liogpu.h, the defaults are as documented, and what can be refused before a device is touched is
refused for the stated reason."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_sdf_default_config", "lio_sdf_create", "lio_sdf_destroy", "lio_sdf_build", "lio_kf_store_sdf", "lio_sdf_nodes", "lio_sdf_query",
           "lio_occupancy_sdf", "lio_sdf_debug_stage_ms", "lio_sdf_memory")


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    cfg_fields = [n for n, _ in pkg.SdfConfig._fields_]
    info_fields = [n for n, _ in pkg.SdfInfo._fields_]
    lines = ['printf("%zu %zu\\n", sizeof(lio_sdf_config), sizeof(lio_sdf_info));']
    lines += [f'printf("%zu\\n", offsetof(lio_sdf_config, {n}));' for n in cfg_fields]
    lines += [f'printf("%zu\\n", offsetof(lio_sdf_info, {n}));' for n in info_fields]
    lines += ['printf("%d\\n", LIO_SDF_NODE_LIMIT);']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert out[:2] == [C.sizeof(pkg.SdfConfig), C.sizeof(pkg.SdfInfo)]
    k = 2
    assert out[k:k + len(cfg_fields)] == [getattr(pkg.SdfConfig, n).offset for n in cfg_fields]
    k += len(cfg_fields)
    assert out[k:k + len(info_fields)] == [getattr(pkg.SdfInfo, n).offset for n in info_fields]
    assert out[-1] == pkg.SDF_NODE_LIMIT == 1 << 25


def test_defaults(pkg):
    cfg = pkg.sdf_default_config()
    assert math.isnan(cfg.min_height) and math.isnan(cfg.max_height) and cfg.nan_policy == 0 and cfg.pad == 0


def test_refused_before_any_device(pkg):
    """the geometry and the configuration are checked first, before the object is looked at: LIO_ERR_ARG with the reason, on a
    machine without a GPU too (where no object can be created)"""
    lib = pkg.load_library()
    grid = np.zeros((4, 5), np.float32, order="F")
    info = pkg.SdfInfo()

    def build(rows=4, cols=5, res=0.2, length=None, position=(0.0, 0.0), **kw):
        ln = (C.c_double * 2)(*(length or (rows * res, cols * res)))
        ps = (C.c_double * 2)(*position)
        cfg = pkg.sdf_default_config(**kw)
        rc = lib.lio_sdf_build(None, grid.ctypes.data, rows, cols, res, ln, ps, C.byref(cfg), C.byref(info))
        return rc, lib.lio_last_error().decode()

    nan, inf = float("nan"), float("inf")
    for kw, why in ((dict(rows=1), "at least 2"), (dict(cols=1), "at least 2"), (dict(rows=0), "at least 2"), (dict(cols=-3), "at least 2"),
                    (dict(length=(nan, 1.0)), "finite"), (dict(length=(0.8, inf)), "finite"), (dict(position=(nan, 0.0)), "finite"),
                    (dict(position=(0.0, -inf)), "finite"), (dict(res=5e-5), "resolution"), (dict(res=nan), "resolution"), (dict(res=inf), "resolution"),
                    (dict(length=(0.8, 1.2)), "size * resolution"), (dict(length=(1.0, 1.0)), "size * resolution"),
                    (dict(min_height=1.0, max_height=0.5), "max_height"), (dict(min_height=inf), "finite or NaN"),
                    (dict(nan_policy=2), "nan_policy"), (dict(nan_policy=-1), "nan_policy"), (dict(rows=1 << 24), "2^24")):
        rc, msg = build(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    rc, msg = build()                                          # nothing wrong but the object
    assert rc == -1 and "null argument" in msg and (info.rows, info.cols, info.resolution) == (4, 5, 0.2)
    assert lib.lio_sdf_build(None, grid.ctypes.data, 4, 5, 0.2, None, None, None, None) == -1
    # the other entry points
    out = np.zeros(20, np.float32)
    occ = np.zeros((5, 4), np.int8)
    for args, why in (((0, occ.ctypes.data, 0, 5, 0.1, 100, out.ctypes.data), "width and height"), ((0, occ.ctypes.data, 4, -1, 0.1, 100, out.ctypes.data), "width and height"),
                      ((0, occ.ctypes.data, 4, 5, 5e-5, 100, out.ctypes.data), "resolution"), ((0, occ.ctypes.data, 4, 5, nan, 100, out.ctypes.data), "resolution"),
                      ((0, None, 4, 5, 0.1, 100, out.ctypes.data), "null"), ((0, occ.ctypes.data, 4, 5, 0.1, 100, None), "null")):
        assert lib.lio_occupancy_sdf(*args) == -1 and why in lib.lio_last_error().decode(), args
    assert lib.lio_sdf_nodes(None, out.ctypes.data, 20) == -1 and lib.lio_sdf_query(None, None, 0, None, None) == -1
    assert lib.lio_sdf_create(0, None) == -1 and lib.lio_sdf_memory(None, None, None) == -1
    # 2 layers of 4097 x 4096 cells already exceed the node limit: refused before the object or a device is looked at
    big = (C.c_double * 2)(4097 * 0.2, 4096 * 0.2)
    cfg = pkg.sdf_default_config()
    assert lib.lio_sdf_build(None, grid.ctypes.data, 4097, 4096, 0.2, big, (C.c_double * 2)(0.0, 0.0), C.byref(cfg), C.byref(info)) == -3
    lib.lio_sdf_destroy(None)                                  # a null object: nothing happens
    lm, hm, cfg = pkg.local_map_default_config(), pkg.height_map_default_config(), pkg.sdf_default_config()
    pose = (C.c_float * 6)()
    assert lib.lio_kf_store_sdf(None, C.byref(lm), pose, C.byref(hm), C.byref(cfg), None, 0, None, None, None, None) == -1


def test_occupancy_without_a_transform_needs_no_device(pkg):
    """signedDistanceFromOccupancy's two shortcuts: no obstacle +INF, no free cell -INF, decided on the host"""
    occ = np.zeros((5, 4), np.int8)
    assert (pkg.occupancy_sdf(occ, 0.1) == np.inf).all()
    assert (pkg.occupancy_sdf(occ + 100, 0.1) == -np.inf).all()
    assert (pkg.occupancy_sdf(occ + 100, 0.1, occupied_min=101) == np.inf).all()
    assert (pkg.occupancy_sdf(occ + 1, 0.1, occupied_min=1) == -np.inf).all()
