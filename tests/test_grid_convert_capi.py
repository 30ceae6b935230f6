"""The grid converters' part of the C ABI without a GPU (lio_grid_to_image, lio_grid_add_layer_from_image,
lio_grid_add_color_layer_from_image, lio_grid_from_occupancy, lio_grid_to_point_cloud, lio_grid_to_grid_cells,
lio_sdf_to_point_cloud): the library exports the symbols, the numpy records the wrappers pass match gcc's layout of
include/liogpu.h, and what can be refused before an object is read is refused for the stated reason.  (No object can be created
without a device: the refusals that need one are in tests/test_gpu_grid_convert.py.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_to_image", "lio_grid_add_layer_from_image", "lio_grid_add_color_layer_from_image", "lio_grid_from_occupancy",
           "lio_grid_to_point_cloud", "lio_grid_to_grid_cells", "lio_sdf_to_point_cloud", "lio_grid_convert_debug_stage_ms")
NAN, INF = float("nan"), float("inf")


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions
    assert (pkg.IMAGE_8U, pkg.IMAGE_16U, pkg.IMAGE_32F) == (0, 1, 2)


def test_struct_layouts_match_c(pkg):
    structs = (("lio_grid_image_info", pkg.GRID_IMAGE_INFO_DTYPE), ("lio_grid_from_image_info", pkg.GRID_FROM_IMAGE_INFO_DTYPE),
               ("lio_grid_from_occupancy_info", pkg.GRID_FROM_OCCUPANCY_INFO_DTYPE))
    lines = ['printf("%d %d %d\\n", LIO_IMAGE_8U, LIO_IMAGE_16U, LIO_IMAGE_32F);']
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
    assert out[:3] == [0, 1, 2]
    k = 3
    for cname, dt in structs:
        want = [dt.itemsize]
        for n in dt.names:
            want += [dt.fields[n][1], dt.fields[n][0].itemsize]
        assert out[k:k + len(want)] == want, (cname, out[k:k + len(want)], want)
        k += len(want)
    assert k == len(out)
    assert pkg.GRID_IMAGE_INFO_DTYPE.names == ("rows", "cols", "lower", "upper", "n_pixels", "n_clamped_low", "n_clamped_high", "n_nonfinite")
    assert pkg.GRID_FROM_IMAGE_INFO_DTYPE.names == ("rows", "cols", "geometry_set", "pad", "n_cells_set", "n_cells_transparent")
    assert pkg.GRID_FROM_OCCUPANCY_INFO_DTYPE.names == ("rows", "cols", "geometry_replaced", "pad", "length", "position", "n_unknown")


def test_refused_before_any_object_is_read(pkg):
    lib = pkg.load_library()
    a, b = C.create_string_buffer(64), C.create_string_buffer(64)                # addresses that are never read as objects
    A, B = C.addressof(a), C.addressof(b)
    info = np.full(80, -1, np.int8)                            # cleared by every call that has one, whatever its struct
    pos = (C.c_double * 2)(0.0, 0.0)

    def refused(rc, why):
        msg = lib.lio_last_error().decode()
        assert rc == -1 and why in msg, (rc, why, msg)

    # to_image: the format and the bounds before the object
    for kw, why in ((dict(ch=2), "channels"), (dict(ch=0), "channels"), (dict(ch=5), "channels"), (dict(depth=3), "depth"), (dict(depth=-1), "depth"),
                    (dict(lo=NAN), "both"), (dict(hi=NAN), "both"), (dict(lo=1.0, hi=1.0), "greater"), (dict(lo=2.0, hi=1.0), "greater"),
                    (dict(lo=-3e38, hi=3e38), "finite"), (dict(lo=-INF, hi=0.0), "finite"), (dict(g=None), "null"), (dict(image=None), "null")):
        args = dict(g=A, ch=1, depth=0, lo=0.0, hi=1.0, image=B)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_to_image(args["g"], 0, args["ch"], args["depth"], args["lo"], args["hi"], args["image"], 64, info.ctypes.data), why)
        assert not info[:48].any() and (info[48:] == -1).all()
    # add_layer_from_image
    for kw, why in ((dict(ch=2), "channels"), (dict(depth=7), "depth"), (dict(ch=3, depth=2), "32F"), (dict(ch=4, depth=2), "32F"), (dict(alpha=-0.1), "alpha_threshold"),
                    (dict(alpha=1.5), "alpha_threshold"), (dict(alpha=NAN), "alpha_threshold"), (dict(image=None), "null"), (dict(layer=16), "layer"),
                    (dict(layer=-1), "layer"), (dict(rows=0), "rows and cols"), (dict(cols=-3), "rows and cols"), (dict(g=None), "null")):
        args = dict(g=A, layer=0, image=B, rows=2, cols=2, ch=1, depth=0, alpha=0.5)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_add_layer_from_image(args["g"], args["layer"], args["image"], args["rows"], args["cols"], args["ch"], args["depth"], 0.0, 1.0,
                                                  args["alpha"], 0.1, pos, info.ctypes.data), why)
        assert not info[:32].any() and (info[32:] == -1).all()
    # add_color_layer_from_image
    for kw, why in ((dict(ch=1), "3 or 4"), (dict(ch=2), "3 or 4"), (dict(depth=1), "8U"), (dict(depth=2), "8U"), (dict(image=None), "null"),
                    (dict(layer=16), "layer"), (dict(rows=0), "rows and cols"), (dict(g=None), "null")):
        args = dict(g=A, layer=0, image=B, rows=2, cols=2, ch=3, depth=0)
        args.update(kw)
        info[:] = -1
        refused(lib.lio_grid_add_color_layer_from_image(args["g"], args["layer"], args["image"], args["rows"], args["cols"], args["ch"], args["depth"], 0.1, pos,
                                                        info.ctypes.data), why)
        assert not info[:32].any()
    # from_occupancy
    for kw, why in ((dict(data=None), "null"), (dict(origin=None), "null"), (dict(layer=16), "layer"), (dict(width=0, n=0), "width and height"),
                    (dict(height=1 << 24, n=5 << 24), "width and height"), (dict(n=14), "width * height"), (dict(n=16), "width * height"),
                    (dict(res=5e-5), "resolution"), (dict(res=NAN), "resolution"), (dict(res=INF), "resolution"), (dict(origin=(NAN, 0.0)), "origin"),
                    (dict(origin=(0.0, -INF)), "origin"), (dict(g=None), "null")):
        args = dict(g=A, layer=0, data=B, n=15, width=5, height=3, res=0.5, origin=(1.0, 2.0))
        args.update(kw)
        info[:] = -1
        origin = (C.c_double * 2)(*args["origin"]) if args["origin"] is not None else None
        refused(lib.lio_grid_from_occupancy(args["g"], args["layer"], args["data"], args["n"], args["width"], args["height"], args["res"], origin, info.ctypes.data),
                why)
        assert not info[:56].any() and (info[56:] == -1).all()
    # to_point_cloud
    n, nf = C.c_size_t(99), C.c_int32(99)
    ids = (C.c_int32 * 3)(0, 1, 2)
    for kw, why in ((dict(ids=None), "null"), (dict(n_out=None), "null"), (dict(points=None), "null"), (dict(n=0), "n_layers"), (dict(n=17), "n_layers"),
                    (dict(ids=(C.c_int32 * 2)(3, 3), n=2), "repeated"), (dict(ids=(C.c_int32 * 2)(3, 16), n=2), "outside"), (dict(ids=(C.c_int32 * 1)(-1), n=1), "outside"),
                    (dict(basic=1 << 16), "basic_mask"), (dict(g=None), "null")):
        args = dict(g=A, ids=ids, n=3, basic=0, points=B, n_out=C.byref(n))
        args.update(kw)
        n.value, nf.value = 99, 99
        refused(lib.lio_grid_to_point_cloud(args["g"], 0, args["ids"], args["n"], args["basic"], args["points"], 1, args["n_out"], C.byref(nf)), why)
        assert nf.value == 0 and (args["n_out"] is None or n.value == 0)
    # to_grid_cells
    for kw, why in ((dict(n_out=None), "null"), (dict(cells=None), "null"), (dict(lo=NAN), "NaN"), (dict(hi=NAN), "NaN"), (dict(g=None), "null")):
        args = dict(g=A, lo=0.0, hi=1.0, cells=B, n_out=C.byref(n))
        args.update(kw)
        n.value = 99
        refused(lib.lio_grid_to_grid_cells(args["g"], 0, args["lo"], args["hi"], args["cells"], 1, args["n_out"]), why)
        assert args["n_out"] is None or n.value == 0
    # sdf_to_point_cloud
    for kw, why in ((dict(n_out=None), "null"), (dict(points=None), "null"), (dict(decimation=0), "decimation"), (dict(decimation=-2), "decimation"),
                    (dict(sdf=None), "null")):
        args = dict(sdf=A, decimation=1, points=B, n_out=C.byref(n))
        args.update(kw)
        n.value = 99
        refused(lib.lio_sdf_to_point_cloud(args["sdf"], args["decimation"], NAN, NAN, args["points"], 1, args["n_out"]), why)
        assert args["n_out"] is None or n.value == 0
    ms = (C.c_float * 3)(-1.0, -1.0, -1.0)
    assert lib.lio_grid_convert_debug_stage_ms(0, 0, ms) == 0 and list(ms) == [0.0, 0.0, 0.0]
    assert lib.lio_grid_convert_debug_stage_ms(0, 0, None) == 0


def test_python_wrappers_name_the_entries(pkg):
    for name in ("to_image", "add_layer_from_image", "add_color_layer_from_image", "from_occupancy", "to_point_cloud", "to_grid_cells"):
        assert callable(getattr(pkg.Grid, name)), name
    assert callable(pkg.Sdf.to_point_cloud)
