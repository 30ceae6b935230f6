"""lio_grid_filter_radius's, _window's, _curvature's, _threshold's, lio_grid_duplicate_layer's and lio_grid_delete_layers' part of
the C ABI without a GPU: the library exports the symbols, the numpy record the wrappers pass matches gcc's layout of
include/liogpu.h, and what can be refused before an object is read is refused for the stated reason.  (No object can be created
without a device: the refusals that need one -- an object without layers, an absent layer, a threshold on an absent output layer,
a derived window beyond 32 cells, crop with weights at a derived size -- are in tests/test_gpu_grid_filter.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_filter_radius", "lio_grid_filter_window", "lio_grid_filter_curvature", "lio_grid_filter_threshold", "lio_grid_duplicate_layer",
           "lio_grid_delete_layers", "lio_grid_filter_debug_kernel_ms")


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layout_and_enums_match_c(pkg):
    dt = pkg.GRID_FILTER_INFO_DTYPE
    cname = "lio_grid_filter_info"
    lines = [f'printf("%zu\\n", sizeof({cname}));']
    for n in dt.names:
        lines.append(f'printf("%zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname} *)0)->{n}));')
    lines.append(f"{{ struct {cname} a; {cname} *p = &a; (void)p; }}")           # both spellings name the same type
    enums = ("LIO_GF_MIN", "LIO_GF_MEAN", "LIO_GW_INSIDE", "LIO_GW_CROP", "LIO_GW_EMPTY", "LIO_GW_EDGE_MEAN", "LIO_GW_SUM", "LIO_GW_MEAN_OF_FINITES",
             "LIO_GW_MIN_OF_FINITES", "LIO_GW_MAX_OF_FINITES", "LIO_GW_NUMBER_OF_FINITES", "LIO_GW_STDDEV", "LIO_GW_WEIGHTED_SUM")
    lines += [f'printf("%d\\n", (int){e});' for e in enums]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    want = [dt.itemsize]
    for n in dt.names:
        want += [dt.fields[n][1], dt.fields[n][0].itemsize]
    assert out[:len(want)] == want, (out, want)
    assert dt.names == ("rows", "cols", "window_size", "pad", "n_visited", "n_written", "n_changed")
    assert out[len(want):] == [getattr(pkg, e[4:]) for e in enums] == [0, 1, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6]


def test_refused_before_any_object_is_read(pkg):
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    a = C.create_string_buffer(8)                              # an address that is never read
    A = C.addressof(a)
    k9 = (C.c_float * 9)(*range(9))
    info = np.full(64, -1, np.int8)

    def refused(rc, why, cleared=True):
        got = lib.lio_last_error().decode()
        assert rc == -1 and why in got, (rc, why, got)
        if cleared:
            assert not info[:40].any() and (info[40:] == -1).all()

    # radius
    for kw, why in ((dict(op=2), "op is"), (dict(op=-1), "op is"), (dict(src=16), "outside 0 .. 15"), (dict(src=-1), "outside 0 .. 15"),
                    (dict(dst=16), "outside 0 .. 15"), (dict(dst=3, src=3), "out_layer is in_layer"), (dict(radius=-1e-300), "radius"),
                    (dict(radius=nan), "radius"), (dict(radius=inf), "radius"), (dict(g=None), "null")):
        args = dict(g=A, src=0, dst=1, op=0, radius=0.5)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_filter_radius(args["g"], args["src"], args["dst"], args["op"], args["radius"], info.ctypes.data), why)
    # window
    for kw, why in ((dict(op=7), "op is"), (dict(op=-1), "op is"), (dict(edge=4), "edge_handling"), (dict(edge=-1), "edge_handling"),
                    (dict(src=16), "outside 0 .. 15"), (dict(dst=-2), "outside 0 .. 15"), (dict(size=2), "odd"), (dict(size=64), "odd"), (dict(size=-3), "odd"),
                    (dict(size=67), "32 cells"), (dict(length=-0.1), "window_length"), (dict(length=nan), "window_length"), (dict(size=0, length=inf), "window_length"),
                    (dict(op=6), "needs weights"), (dict(op=5, weights=k9), "reads none"), (dict(op=6, edge=1, weights=k9), "disagree"), (dict(g=None), "null")):
        args = dict(g=A, src=0, dst=0, op=0, edge=1, size=3, length=0.0, weights=None)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_filter_window(args["g"], args["src"], args["dst"], args["op"], args["edge"], args["size"], args["length"], args["weights"],
                                           info.ctypes.data), why)
    # curvature
    for g, src, dst, why in ((A, 16, 0, "outside 0 .. 15"), (A, 0, -1, "outside 0 .. 15"), (A, 2, 2, "out_layer is in_layer"), (None, 0, 1, "null")):
        info[:] = -1
        refused(lib.lio_grid_filter_curvature(g, src, dst, info.ctypes.data), why)
    # threshold
    for g, cond, dst, upper, why in ((A, 0, 0, 2, "upper is 0 or 1"), (A, 0, 0, -1, "upper is 0 or 1"), (A, 16, 0, 0, "outside 0 .. 15"),
                                     (A, 0, 16, 1, "outside 0 .. 15"), (None, 0, 0, 1, "null")):
        info[:] = -1
        refused(lib.lio_grid_filter_threshold(g, cond, dst, upper, 0.5, nan, info.ctypes.data), why)
    # duplicate, delete
    for g, src, dst, why in ((A, 16, 0, "outside 0 .. 15"), (A, 0, -1, "outside 0 .. 15"), (None, 0, 1, "null")):
        refused(lib.lio_grid_duplicate_layer(g, src, dst), why, cleared=False)
    ids = (C.c_int32 * 3)(0, 1, 2)
    for g, p, n, why in ((A, ids, 0, "n_layers"), (A, ids, 17, "n_layers"), (A, ids, -1, "n_layers"), (A, None, 2, "null"),
                         (A, (C.c_int32 * 2)(3, 3), 2, "repeated"), (A, (C.c_int32 * 2)(3, 16), 2, "outside"), (A, (C.c_int32 * 1)(-1), 1, "outside"),
                         (None, ids, 3, "null")):
        refused(lib.lio_grid_delete_layers(g, p, n), why, cleared=False)
    # every call passes info == NULL
    assert lib.lio_grid_filter_radius(A, 0, 1, 2, 0.5, None) == -1
    assert lib.lio_grid_filter_window(A, 0, 1, 7, 1, 3, 0.0, None, None) == -1
    assert lib.lio_grid_filter_curvature(A, 1, 1, None) == -1
    assert lib.lio_grid_filter_threshold(A, 0, 0, 2, 0.0, 0.0, None) == -1
    ms = C.c_float(-1.0)
    assert lib.lio_grid_filter_debug_kernel_ms(0, C.byref(ms)) == 0 and ms.value == 0.0
    assert lib.lio_grid_filter_debug_kernel_ms(0, None) == 0


def test_python_and_cpp_wrappers_name_the_entries(pkg):
    for name in ("filter_radius", "filter_window", "filter_curvature", "filter_threshold", "duplicate_layer", "delete_layers"):
        assert callable(getattr(pkg.Grid, name)), name
    hpp = open(os.path.join(ROOT, "include", "liogpu.hpp")).read()
    for name in SYMBOLS[:6]:
        assert name + "(" in hpp, name
    with tempfile.TemporaryDirectory() as d:                   # the C++ wrapper compiles on the host against the header
        c = os.path.join(d, "t.cpp")
        open(c, "w").write('#include "liogpu.hpp"\nint main() {\n'
                           "void (liogpu::GridLayers::*a)(int32_t, int32_t, int32_t, double, lio_grid_filter_info*) = &liogpu::GridLayers::filterInRadius;\n"
                           "void (liogpu::GridLayers::*b)(int32_t, int32_t, int32_t, int32_t, int32_t, double, const float*, lio_grid_filter_info*) = "
                           "&liogpu::GridLayers::filterSlidingWindow;\n"
                           "void (liogpu::GridLayers::*c)(int32_t, int32_t, lio_grid_filter_info*) = &liogpu::GridLayers::filterCurvature;\n"
                           "void (liogpu::GridLayers::*e)(int32_t, int32_t, bool, double, double, lio_grid_filter_info*) = &liogpu::GridLayers::filterThreshold;\n"
                           "void (liogpu::GridLayers::*f)(int32_t, int32_t) = &liogpu::GridLayers::duplicateLayer;\n"
                           "void (liogpu::GridLayers::*h)(const int32_t*, int32_t) = &liogpu::GridLayers::deleteLayers;\n"
                           "return a && b && c && e && f && h ? 0 : 1; }\n")
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c])
