"""The resident layers' part of the C ABI without a GPU: the library exports the symbols, the ctypes structs match gcc's layout
of include/liogpu.h, the defaults are as documented, and what can be refused before a device is touched is refused for the
stated reason."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_sample_default_config", "lio_grid_create", "lio_grid_destroy", "lio_grid_set_layers", "lio_grid_get_layer", "lio_grid_info",
           "lio_grid_memory", "lio_grid_sample", "lio_kf_store_planning_grid", "lio_grid_debug_stage_ms")


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    structs = (("lio_grid_sample_config", pkg.GridSampleConfig), ("lio_grid_sample_info", pkg.GridSampleInfo), ("lio_grid_desc", pkg.GridInfo))
    lines = []
    for cname, cls in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    lines += ['printf("%d %d %d %d %d %d\\n", LIO_GRID_MAX_LAYERS, LIO_GRID_NEAREST, LIO_GRID_LINEAR, LIO_GRID_CUBIC_CONVOLUTION, LIO_GRID_CUBIC, LIO_GRID_OUTSIDE);',
              'printf("%d %d %d %d\\n", LIO_GRID_LAYER_ELEVATION, LIO_GRID_LAYER_FILLED, LIO_GRID_LAYER_TERRAIN, LIO_TERRAIN_N_LAYERS);']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    k = 0
    for cname, cls in structs:
        want = [C.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
        assert out[k:k + len(want)] == want, cname
        k += len(want)
    assert out[k:k + 6] == [pkg.GRID_MAX_LAYERS, pkg.GRID_NEAREST, pkg.GRID_LINEAR, pkg.GRID_CUBIC_CONVOLUTION, pkg.GRID_CUBIC, pkg.GRID_OUTSIDE] == [16, 0, 1, 2, 3, 255]
    assert out[k + 6:] == [pkg.GRID_LAYER_ELEVATION, pkg.GRID_LAYER_FILLED, pkg.GRID_LAYER_TERRAIN, len(pkg.TERRAIN_LAYERS)] == [0, 1, 2, 8]


def test_defaults(pkg):
    cfg = pkg.grid_sample_default_config()
    assert (cfg.method, cfg.border_mode) == (pkg.GRID_NEAREST, 0)
    pkg.load_library().lio_grid_sample_default_config(None)    # a null pointer: nothing happens


def test_refused_before_any_device(pkg):
    """the geometry and the configuration are checked first, before the object is looked at: LIO_ERR_ARG with the reason, on a
    machine without a GPU too (where no object can be created)"""
    lib = pkg.load_library()
    layers = np.zeros((2, 4 * 5), np.float32)
    nan, inf = float("nan"), float("inf")

    def set_layers(n_layers=2, rows=4, cols=5, res=0.2, length=None, position=(0.0, 0.0)):
        ln = (C.c_double * 2)(*(length or (rows * res, cols * res)))
        ps = (C.c_double * 2)(*position)
        rc = lib.lio_grid_set_layers(None, layers.ctypes.data, n_layers, rows, cols, res, ln, ps)
        return rc, lib.lio_last_error().decode()

    for kw, why in ((dict(n_layers=0), "n_layers"), (dict(n_layers=17), "n_layers"), (dict(n_layers=-1), "n_layers"), (dict(rows=0), "at least 1"),
                    (dict(cols=-3), "at least 1"), (dict(rows=1 << 24), "2^24"), (dict(cols=1 << 24), "2^24"), (dict(length=(nan, 1.0)), "finite"),
                    (dict(length=(0.8, inf)), "finite"), (dict(position=(nan, 0.0)), "finite"), (dict(position=(0.0, -inf)), "finite"),
                    (dict(res=5e-5), "resolution"), (dict(res=nan), "resolution"), (dict(res=inf), "resolution"),
                    (dict(length=(0.8, 1.2)), "size * resolution"), (dict(length=(1.0, 1.0)), "size * resolution")):
        rc, msg = set_layers(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    rc, msg = set_layers()                                     # nothing wrong but the object
    assert rc == -1 and "null argument" in msg
    assert lib.lio_grid_set_layers(None, layers.ctypes.data, 2, 4, 5, 0.2, None, None) == -1
    big = (C.c_double * 2)(65536 * 0.25, 32768 * 0.25)        # 2^31 cells a layer: refused before the object or a device is looked at
    assert lib.lio_grid_set_layers(None, layers.ctypes.data, 1, 65536, 32768, 0.25, big, (C.c_double * 2)(0.0, 0.0)) == -3
    # the sampling call: the configuration and the counts first
    ids = (C.c_int32 * 2)(0, 1)
    pos = np.zeros((3, 2), np.float64)
    val = np.zeros((2, 3), np.float32)
    info = pkg.GridSampleInfo()

    def sample(n_layers=2, ids=ids, cfg_ptr=True, **kw):
        cfg = pkg.grid_sample_default_config(**kw)
        rc = lib.lio_grid_sample(None, ids, n_layers, C.byref(cfg) if cfg_ptr else None, pos.ctypes.data, 3, val.ctypes.data, None, C.byref(info))
        return rc, lib.lio_last_error().decode()

    for kw, why in ((dict(method=4), "method"), (dict(method=-1), "method"), (dict(border_mode=2), "border_mode"), (dict(border_mode=-1), "border_mode"),
                    (dict(n_layers=0), "n_layers"), (dict(n_layers=17), "n_layers"), (dict(ids=None), "null"), (dict(cfg_ptr=False), "null")):
        rc, msg = sample(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    rc, msg = sample()
    assert rc == -1 and "null argument" in msg                 # nothing wrong but the object
    cfg = pkg.grid_sample_default_config()
    assert lib.lio_grid_sample(None, ids, 2, C.byref(cfg), None, 3, val.ctypes.data, None, None) == -1
    assert lib.lio_grid_sample(None, ids, 2, C.byref(cfg), pos.ctypes.data, 3, None, None, None) == -1
    # the other entry points
    out = np.zeros(20, np.float32)
    assert lib.lio_grid_get_layer(None, 0, out.ctypes.data, 20) == -1 and lib.lio_grid_info(None, None) == -1
    assert lib.lio_grid_memory(None, None) == -1 and lib.lio_grid_create(0, None) == -1
    lib.lio_grid_destroy(None)                                 # a null object: nothing happens
    lm, hm = pkg.local_map_default_config(), pkg.height_map_default_config()
    pose = (C.c_float * 6)()
    assert lib.lio_kf_store_planning_grid(None, C.byref(lm), pose, C.byref(hm), None, None, None, None, None, None, None, None, None, None, None) == -1
    ms = (C.c_float * 3)()
    assert lib.lio_grid_debug_stage_ms(0, ms) == 0 and list(ms) == [0.0, 0.0, 0.0]
