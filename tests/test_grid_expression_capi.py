"""lio_grid_expression_check's, lio_grid_filter_expression's and lio_debug_grid_expression_host's part of the C ABI without a
GPU: the library exports the symbols, the numpy record the wrappers pass matches gcc's layout of include/liogpu.h, and every
refusal of the expression, the names and the ids is decided before an object is read (an address that is never read stands in
for g).  The refusals that need an object -- no layers, an absent layer that is read -- are in tests/test_gpu_grid_expression.py."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_expression_cases as K                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_expression_check", "lio_grid_filter_expression", "lio_debug_grid_expression_host", "lio_grid_expression_debug_kernel_ms")


def _names(names):
    keys = [k.encode() for k in names]
    return (C.c_char_p * len(keys))(*keys), (C.c_int32 * len(keys))(*names.values()), len(keys)


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layout_matches_c(pkg):
    dt = pkg.GRID_EXPRESSION_INFO_DTYPE
    cname = "lio_grid_expression_info"
    lines = [f'printf("%zu\\n", sizeof({cname}));']
    for n in dt.names:
        lines.append(f'printf("%zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname} *)0)->{n}));')
    lines.append(f"{{ struct {cname} a; {cname} *p = &a; (void)p; }}")           # both spellings name the same type
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
    assert out == want, (out, want)
    assert dt.names == ("rows", "cols", "n_ops", "n_passes", "layers_read", "stack_depth", "n_finite") and dt.itemsize == 32


def test_refused_before_any_object_is_read(pkg):
    lib = pkg.load_library()
    a = C.create_string_buffer(8)                              # an address that is never read
    A = C.addressof(a)
    info = np.full(64, -1, np.int8)

    def refused(rc, code, why):
        got = lib.lio_last_error().decode()
        assert rc == code and why in got, (rc, code, why, got)
        assert not info[:32].any() and (info[32:] == -1).all()

    for expression, names, code, part, _ in K.REFUSED:
        for entry in ("check", "filter", "host"):
            info[:] = -1
            keys, ids, n = _names(names)
            if entry == "check":
                rc = lib.lio_grid_expression_check(expression.encode(), keys, ids, n, info.ctypes.data)
            elif entry == "filter":
                rc = lib.lio_grid_filter_expression(A, expression.encode(), keys, ids, n, 3, info.ctypes.data)
            else:
                info[:32] = 0
                rc = lib.lio_debug_grid_expression_host(expression.encode(), keys, n, None, 4, 4, None)
            refused(rc, code, part)
    # the names and the ids
    for names, part in K.BAD_NAMES:
        info[:] = -1
        keys, ids, n = _names(names)
        refused(lib.lio_grid_filter_expression(A, b"a", keys, ids, n, 0, info.ctypes.data), -1, part)
    keys, ids, n = _names(K.NAMES)
    for call, part in ((lambda: lib.lio_grid_filter_expression(A, None, keys, ids, n, 0, info.ctypes.data), "null"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", None, ids, n, 0, info.ctypes.data), "null"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", keys, None, n, 0, info.ctypes.data), "null"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", keys, ids, 17, 0, info.ctypes.data), "n_names"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", keys, ids, -1, 0, info.ctypes.data), "n_names"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", (C.c_char_p * 2)(b"a", b"a"), ids, 2, 0, info.ctypes.data), "listed twice"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", keys, ids, n, 16, info.ctypes.data), "outside 0 .. 15"),
                       (lambda: lib.lio_grid_filter_expression(A, b"a", keys, ids, n, -1, info.ctypes.data), "outside 0 .. 15"),
                       (lambda: lib.lio_grid_filter_expression(None, b"a", keys, ids, n, 0, info.ctypes.data), "null")):
        info[:] = -1
        refused(call(), -1, part)
    # every call passes info == NULL; n_names == 0 leaves every name unknown
    assert lib.lio_grid_filter_expression(A, b"+a", keys, ids, n, 0, None) == -1
    assert lib.lio_grid_expression_check(b"a", None, None, 0, None) == -1 and "unknown name 'a'" in lib.lio_last_error().decode()
    assert lib.lio_grid_expression_check(b"a + b", keys, ids, n, None) == 0
    ms = (C.c_float * 2)(-1.0, -1.0)
    assert lib.lio_grid_expression_debug_kernel_ms(0, ms) == 0 and list(ms) == [0.0, 0.0]
    assert lib.lio_grid_expression_debug_kernel_ms(0, None) == 0


def test_python_and_cpp_wrappers_name_the_entries(pkg):
    assert callable(pkg.Grid.filter_expression) and callable(pkg.grid_expression_check) and callable(pkg.grid_expression_host)
    hpp = open(os.path.join(ROOT, "include", "liogpu.hpp")).read()
    assert "lio_grid_filter_expression(" in hpp
    with tempfile.TemporaryDirectory() as d:                   # the C++ wrapper compiles on the host against the header
        c = os.path.join(d, "t.cpp")
        open(c, "w").write('#include "liogpu.hpp"\nint main() {\n'
                           "void (liogpu::GridLayers::*a)(const char*, const char* const*, const int32_t*, int32_t, int32_t, lio_grid_expression_info*) = "
                           "&liogpu::GridLayers::filterMathExpression;\nreturn a ? 0 : 1; }\n")
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c])
