"""lio_grid_transform's and lio_grid_to_occupancy's part of the C ABI without a GPU: the library exports the symbols, the numpy
records the wrappers pass match gcc's layout of include/liogpu.h, and what can be refused before a device is touched is refused
for the stated reason.  (No object can be created without a device: the refusals that need one -- grids on different devices,
a source without layers, an absent layer, a new size below 1, the capacities -- are in tests/test_gpu_grid_transform.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_transform", "lio_grid_to_occupancy", "lio_grid_transform_debug_stage_ms")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    structs = (("lio_grid_transform_info", pkg.GRID_TRANSFORM_INFO_DTYPE), ("lio_grid_occupancy_desc", pkg.GRID_OCCUPANCY_DESC_DTYPE))
    lines = []
    for cname, dt in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for n in dt.names:
            lines.append(f'printf("%zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname} *)0)->{n}));')
    lines.append('printf("%d\\n", LIO_GRID_TRANSFORM_MAX_SOURCE_CELLS);')
    # both spellings name the same type
    lines.append("{ struct lio_grid_transform_info a; lio_grid_transform_info *p = &a; struct lio_grid_occupancy_desc b; lio_grid_occupancy_desc *q = &b; "
                 "(void)p; (void)q; }")
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
    assert out[k:] == [pkg.GRID_TRANSFORM_MAX_SOURCE_CELLS] and 5 * out[k] <= 2 ** 31 < 5 * (out[k] + 1)
    assert pkg.GRID_TRANSFORM_INFO_DTYPE.names == ("rows", "cols", "length", "position", "n_source_cells", "n_samples_outside", "n_cells_written")
    assert pkg.GRID_OCCUPANCY_DESC_DTYPE.names == ("width", "height", "resolution", "pad", "origin")


def test_transform_refused_before_any_device(pkg):
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    a, b = C.create_string_buffer(8), C.create_string_buffer(8)                  # two addresses that are never read
    info = np.zeros(1, pkg.GRID_TRANSFORM_INFO_DTYPE)

    def transform(src=a, dst=b, t=IDENTITY, height=0, ratio=0.25):
        arr = (C.c_double * 12)(*t) if t is not None else None
        rc = lib.lio_grid_transform(C.addressof(src) if src is not None else None, arr, height, ratio, C.addressof(dst) if dst is not None else None,
                                    info.ctypes.data)
        return rc, lib.lio_last_error().decode()

    def with_entry(k, v):
        t = list(IDENTITY)
        t[k] = v
        return t

    cases = [(dict(t=None), "null"), (dict(src=None), "null"), (dict(dst=None), "null"), (dict(src=None, dst=None), "null"),
             (dict(ratio=nan), "sample_ratio"), (dict(ratio=inf), "sample_ratio"), (dict(ratio=-inf), "sample_ratio"),
             (dict(dst=a), "same object")]
    cases += [(dict(t=with_entry(k, v)), "transform") for k in range(12) for v in (nan, inf, -inf)]
    for kw, why in cases:
        rc, msg = transform(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    assert not info.view(np.uint8).any()                        # info is cleared, nothing else is written
    ms = (C.c_float * 3)()
    assert lib.lio_grid_transform_debug_stage_ms(0, ms) == 0 and list(ms) == [0.0, 0.0, 0.0]
    assert lib.lio_grid_transform_debug_stage_ms(0, None) == 0


def test_occupancy_refused_before_any_device(pkg):
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    data = np.full(8, 77, np.int8)
    desc = np.zeros(1, pkg.GRID_OCCUPANCY_DESC_DTYPE)

    def occupancy(lo=0.0, hi=1.0, out=data):
        rc = lib.lio_grid_to_occupancy(None, 0, lo, hi, out.ctypes.data if out is not None else None, 8, desc.ctypes.data)
        return rc, lib.lio_last_error().decode()

    for kw, why in ((dict(lo=nan), "data_min"), (dict(hi=nan), "data_min"), (dict(lo=inf), "data_min"), (dict(hi=-inf), "data_min"),
                    (dict(), "null"), (dict(out=None), "null")):
        rc, msg = occupancy(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    assert (data == 77).all()
    rc, _ = occupancy(lo=1.0, hi=1.0)                          # equal bounds are not what is refused: the null grid is
    assert rc == -1 and "null" in lib.lio_last_error().decode()


def test_python_and_cpp_wrappers_name_the_entries(pkg):
    assert callable(pkg.Grid.transform) and callable(pkg.Grid.to_occupancy)
    hpp = open(os.path.join(ROOT, "include", "liogpu.hpp")).read()
    for name in ("lio_grid_transform(", "lio_grid_to_occupancy("):
        assert name in hpp, name
    with tempfile.TemporaryDirectory() as d:                   # the C++ wrapper compiles on the host against the header
        c = os.path.join(d, "t.cpp")
        open(c, "w").write('#include "liogpu.hpp"\nint main() { void (liogpu::GridLayers::*f)(liogpu::GridLayers&, const double*, int32_t, double, '
                           'lio_grid_transform_info*) = &liogpu::GridLayers::transformInto; return f ? 0 : 1; }\n')
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c])
