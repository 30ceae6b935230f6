"""The region reductions' part of the C ABI without a GPU: the library exports the symbols, the ctypes structs and numpy
records match gcc's layout of include/liogpu.h, the default is as documented, and what can be refused before a device is
touched is refused for the stated reason."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lio_grid_region_default_config", "lio_grid_region_reduce", "lio_grid_region_cells", "lio_grid_region_debug_stage_ms")


def test_symbols_are_exported(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.lio_version() == 102                            # the library only gained functions


def test_struct_layouts_match_c(pkg):
    structs = (("lio_grid_region", pkg.GridRegion), ("lio_grid_region_config", pkg.GridRegionConfig), ("lio_grid_region_stat", pkg.GridRegionStat),
               ("lio_grid_region_info", pkg.GridRegionInfo))
    lines = []
    for cname, cls in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    lines += ['printf("%d %d %d %d %d %d %d %d %d\\n", LIO_REGION_LINE, LIO_REGION_CIRCLE, LIO_REGION_ELLIPSE, LIO_REGION_POLYGON, LIO_REGION_OK, '
              'LIO_REGION_EMPTY, LIO_REGION_INVALID, LIO_REGION_MAX_VERTICES, LIO_REGION_MAX_WALK);']
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
    assert out[k:] == [pkg.REGION_LINE, pkg.REGION_CIRCLE, pkg.REGION_ELLIPSE, pkg.REGION_POLYGON, pkg.REGION_OK, pkg.REGION_EMPTY, pkg.REGION_INVALID,
                       pkg.REGION_MAX_VERTICES, pkg.REGION_MAX_WALK] == [0, 1, 2, 3, 0, 1, 2, 64, 4096]
    # the numpy records the wrappers pass are the same layouts
    for dt, cls in ((pkg.GRID_REGION_DTYPE, pkg.GridRegion), (pkg.GRID_REGION_STAT_DTYPE, pkg.GridRegionStat)):
        assert dt.itemsize == C.sizeof(cls)
        assert [dt.fields[n][1] for n, _ in cls._fields_] == [getattr(cls, n).offset for n, _ in cls._fields_]


def test_defaults(pkg):
    cfg = pkg.grid_region_default_config()
    assert cfg.threshold == 0.5 and cfg.pad == 0
    pkg.load_library().lio_grid_region_default_config(None)    # a null pointer: nothing happens


def test_packing_helpers(pkg):
    rec, verts = pkg.pack_regions([("circle", 1.0, 2.0, 3.0), ("polygon", [(0, 0), (1, 0), (0, 1)]), ("line", 1, 2, 3, 4), ("ellipse", 1, 2, 3, 4, 0.5),
                                   ("polygon", [(5, 5), (6, 5), (6, 6), (5, 6)])])
    assert list(rec["kind"]) == [1, 3, 0, 2, 3] and list(rec["first_vertex"]) == [0, 0, 0, 0, 3] and list(rec["n_vertices"]) == [0, 3, 0, 0, 4]
    assert list(rec["p"][0]) == [1, 2, 3, 0, 0] and list(rec["p"][3]) == [1, 2, 3, 4, 0.5] and verts.shape == (7, 2)
    rec, verts = pkg.footprint_polygons([(1.0, 2.0, 0.0), (0.0, 0.0, np.pi / 2)], 4.0, 2.0)
    assert list(rec["kind"]) == [3, 3] and list(rec["first_vertex"]) == [0, 4] and list(rec["n_vertices"]) == [4, 4]
    assert np.allclose(verts[:4], [(3, 3), (-1, 3), (-1, 1), (3, 1)]) and np.allclose(verts[4:], [(-1, 2), (-1, -2), (1, -2), (1, 2)])


def test_refused_before_any_device(pkg):
    """LIO_ERR_ARG with the reason before the object is looked at, on a machine without a GPU too (where no object can be
    created; the two causes that need one -- an object without layers, an absent layer -- are in tests/test_gpu_grid_region.py)"""
    lib = pkg.load_library()
    nan, inf = float("nan"), float("inf")
    good, gverts = pkg.pack_regions([("circle", 0.0, 0.0, 1.0), ("polygon", [(0, 0), (1, 0), (0, 1)])])
    stats = np.zeros((2, 2), pkg.GRID_REGION_STAT_DTYPE)
    info = pkg.GridRegionInfo()

    def reduce(ids=(0, 1), n_layers=None, cfg_ptr=True, rec=good, verts=gverts, n_vertices=None, stats=stats, regions_ptr=True, **kw):
        cfg = pkg.grid_region_default_config(**kw)
        arr = (C.c_int32 * len(ids))(*ids) if ids is not None else None
        rc = lib.lio_grid_region_reduce(None, arr, len(ids) if n_layers is None else n_layers, C.byref(cfg) if cfg_ptr else None,
                                        rec.ctypes.data if regions_ptr else None, len(rec), verts.ctypes.data if verts is not None else None,
                                        len(verts) if n_vertices is None else n_vertices, stats.ctypes.data if stats is not None else None, None, None,
                                        C.byref(info))
        return rc, lib.lio_last_error().decode()

    def with_region(q, **fields):
        rec = good.copy()
        for k, v in fields.items():
            rec[k][q] = v
        return rec

    cases = [(dict(ids=None, n_layers=1), "null"), (dict(cfg_ptr=False), "null"), (dict(regions_ptr=False), "null"), (dict(stats=None), "null"),
             (dict(verts=None, n_vertices=3), "null"),
             (dict(threshold=nan), "threshold"), (dict(threshold=inf), "threshold"), (dict(threshold=-inf), "threshold"),
             (dict(n_layers=0), "n_layers"), (dict(n_layers=-1), "n_layers"), (dict(ids=tuple(range(16)) + (0,)), "n_layers"),
             (dict(ids=(0, 16)), "layer id"), (dict(ids=(-1,)), "layer id"), (dict(ids=(3, 3)), "repeated"),
             (dict(rec=with_region(0, kind=4)), "kind"), (dict(rec=with_region(0, kind=-1)), "kind"),
             (dict(rec=with_region(1, n_vertices=2)), "vertices"), (dict(rec=with_region(1, n_vertices=65)), "vertices"),
             (dict(rec=with_region(1, first_vertex=1)), "leave"), (dict(rec=with_region(1, first_vertex=-1)), "leave"),
             (dict(rec=with_region(1, first_vertex=1 << 62)), "leave"), (dict(n_vertices=2), "leave")]
    for kw, why in cases:
        rc, msg = reduce(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    rc, msg = reduce()                                         # nothing wrong but the object
    assert rc == -1 and "null argument" in msg
    # more than 2^24 regions: LIO_ERR_CAPACITY before the regions are read
    cfg = pkg.grid_region_default_config()
    ids = (C.c_int32 * 1)(0)
    assert lib.lio_grid_region_reduce(None, ids, 1, C.byref(cfg), good.ctypes.data, (1 << 24) + 1, gverts.ctypes.data, 3, stats.ctypes.data, None, None, None) == -3
    # the cells: the same refusals
    offsets = np.zeros(3, np.int64)
    cells = np.zeros(8, np.int32)

    def get_cells(rec=good, n=None, verts=gverts, n_vertices=3, offsets=offsets, cells=cells, cap=8):
        rc = lib.lio_grid_region_cells(None, rec.ctypes.data, len(rec) if n is None else n, verts.ctypes.data if verts is not None else None, n_vertices,
                                       offsets.ctypes.data if offsets is not None else None, cells.ctypes.data if cells is not None else None, cap, None, None)
        return rc, lib.lio_last_error().decode()

    for kw, why in ((dict(offsets=None), "null"), (dict(cells=None), "null"), (dict(verts=None), "null"), (dict(rec=with_region(0, kind=9)), "kind"),
                    (dict(rec=with_region(1, n_vertices=1)), "vertices"), (dict(n_vertices=1), "leave")):
        rc, msg = get_cells(**kw)
        assert rc == -1 and why in msg, (kw, rc, msg)
    assert get_cells(n=(1 << 24) + 1)[0] == -3
    rc, msg = get_cells()
    assert rc == -1 and "null argument" in msg                 # nothing wrong but the object
    ms = (C.c_float * 4)()
    assert lib.lio_grid_region_debug_stage_ms(0, ms) == 0 and list(ms) == [0.0, 0.0, 0.0, 0.0]
