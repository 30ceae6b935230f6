"""lio_grid_submap's, lio_grid_move's, lio_grid_extend_to_include's and lio_grid_add_data_from's part of the C ABI without a
GPU: the library exports the symbols, the numpy records the wrappers pass match gcc's layout of include/liogpu.h, and what can
be refused before an object is read is refused for the stated reason.  (No object can be created without a device: the
refusals that need one -- a source without layers, absent layers, a basic_mask bit for an absent layer, the capacities, the
shift of 2^30 cells -- are in tests/test_gpu_grid_geom.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_submap", "lio_grid_move", "lio_grid_extend_to_include", "lio_grid_add_data_from", "lio_grid_geom_debug_kernel_ms")


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    structs = (("lio_grid_submap_info", pkg.GRID_SUBMAP_INFO_DTYPE), ("lio_grid_move_info", pkg.GRID_MOVE_INFO_DTYPE),
               ("lio_grid_extend_info", pkg.GRID_EXTEND_INFO_DTYPE), ("lio_grid_add_info", pkg.GRID_ADD_INFO_DTYPE))
    lines = []
    for cname, dt in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for n in dt.names:
            lines.append(f'printf("%zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname} *)0)->{n}));')
        lines.append(f"{{ struct {cname} a; {cname} *p = &a; (void)p; }}")       # both spellings name the same type
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "liogpu.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    k = 0
    for cname, dt in structs:
        want = [dt.itemsize]
        for n in dt.names:
            want += [dt.fields[n][1], dt.fields[n][0].itemsize]
        assert out[k:k + len(want)] == want, (cname, out[k:k + len(want)], want)
        k += len(want)
    assert k == len(out)
    assert pkg.GRID_SUBMAP_INFO_DTYPE.names == ("success", "rows", "cols", "pad", "length", "position", "top_left", "requested_index")
    assert pkg.GRID_MOVE_INFO_DTYPE.names == ("moved", "pad", "index_shift", "position", "n_cells_cleared")
    assert pkg.GRID_EXTEND_INFO_DTYPE.names == ("resized", "rows", "cols", "pad", "length", "position", "n_cells_kept", "n_index_outside")
    assert pkg.GRID_ADD_INFO_DTYPE.names == ("resized", "rows", "cols", "pad", "length", "position", "n_cells_skipped_valid", "n_cells_outside_other",
                                             "n_index_outside", "n_values_copied")


def test_refused_before_any_object_is_read(pkg):
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    a, b = C.create_string_buffer(8), C.create_string_buffer(8)                  # two addresses that are never read
    A, B = C.addressof(a), C.addressof(b)

    def pair(v):
        return (C.c_double * 2)(*v) if v is not None else None

    def last():
        return lib.lio_last_error().decode()

    info = np.full(1, -1, np.int8).repeat(80)                  # cleared by every call, whatever its struct

    def refused(rc, why):
        assert rc == -1 and why in last(), (rc, why, last())

    # submap
    for kw, why in ((dict(position=None), "null"), (dict(length=None), "null"), (dict(src=None), "null"), (dict(dst=None), "null"), (dict(dst=A), "same object"),
                    (dict(position=(nan, 0.0)), "finite"), (dict(position=(0.0, inf)), "finite"), (dict(length=(inf, 1.0)), "finite"),
                    (dict(length=(1.0, nan)), "finite"), (dict(length=(-1.0, 1.0)), "negative"), (dict(length=(1.0, -1e-300)), "negative")):
        args = dict(src=A, position=(0.0, 0.0), length=(1.0, 1.0), dst=B)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_submap(args["src"], pair(args["position"]), pair(args["length"]), args["dst"], info.ctypes.data), why)
        assert not info[:64].any() and (info[64:] == -1).all()
    # move
    for g, position, why in ((None, (0.0, 0.0), "null"), (A, None, "null"), (A, (nan, 0.0), "finite"), (A, (0.0, -inf), "finite")):
        info[:] = -1
        refused(lib.lio_grid_move(g, pair(position), info.ctypes.data), why)
        assert not info[:40].any() and (info[40:] == -1).all()
    # extend_to_include
    for g, other, why in ((None, B, "null"), (A, None, "null"), (None, None, "null"), (A, A, "same object")):
        info[:] = -1
        refused(lib.lio_grid_extend_to_include(g, other, info.ctypes.data), why)
        assert not info[:64].any() and (info[64:] == -1).all()
    # add_data_from
    ids = (C.c_int32 * 3)(0, 1, 2)
    for kw, why in ((dict(g=None), "null"), (dict(other=None), "null"), (dict(other=A), "same object"), (dict(extend=2), "0 or 1"), (dict(extend=-1), "0 or 1"),
                    (dict(overwrite=2), "0 or 1"), (dict(overwrite=-7), "0 or 1"), (dict(n=-1), "n_layers"), (dict(n=17), "n_layers"),
                    (dict(ids=None, n=2), "null"), (dict(ids=(C.c_int32 * 2)(3, 3), n=2), "repeated"), (dict(ids=(C.c_int32 * 2)(3, 16), n=2), "outside"),
                    (dict(ids=(C.c_int32 * 1)(-1), n=1), "outside"), (dict(basic=1 << 16), "basic_mask")):
        args = dict(g=A, other=B, extend=1, overwrite=1, ids=ids, n=3, basic=0)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_add_data_from(args["g"], args["other"], args["extend"], args["overwrite"], args["ids"], args["n"], args["basic"], info.ctypes.data), why)
        assert not info.any()
    ms = C.c_float(-1.0)
    assert lib.lio_grid_geom_debug_kernel_ms(0, C.byref(ms)) == 0 and ms.value == 0.0
    assert lib.lio_grid_geom_debug_kernel_ms(0, None) == 0


def test_python_and_cpp_wrappers_name_the_entries(pkg):
    for name in ("submap", "move", "extend_to_include", "add_data_from"):
        assert callable(getattr(pkg.Grid, name)), name
    hpp = open(os.path.join(ROOT, "include", "liogpu.hpp")).read()
    for name in ("lio_grid_submap(", "lio_grid_move(", "lio_grid_extend_to_include(", "lio_grid_add_data_from("):
        assert name in hpp, name
    with tempfile.TemporaryDirectory() as d:                   # the C++ wrapper compiles on the host against the header
        c = os.path.join(d, "t.cpp")
        open(c, "w").write('#include "liogpu.hpp"\nint main() {\n'
                           "bool (liogpu::GridLayers::*a)(liogpu::GridLayers&, const double*, const double*, lio_grid_submap_info*) = &liogpu::GridLayers::getSubmap;\n"
                           "bool (liogpu::GridLayers::*b)(const double*, lio_grid_move_info*) = &liogpu::GridLayers::move;\n"
                           "bool (liogpu::GridLayers::*c)(liogpu::GridLayers&, lio_grid_extend_info*) = &liogpu::GridLayers::extendToInclude;\n"
                           "void (liogpu::GridLayers::*e)(liogpu::GridLayers&, bool, bool, const int32_t*, int32_t, uint32_t, lio_grid_add_info*) = "
                           "&liogpu::GridLayers::addDataFrom;\nreturn a && b && c && e ? 0 : 1; }\n")
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c])
