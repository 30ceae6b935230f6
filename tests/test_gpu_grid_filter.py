"""The layer filters on the device (lio_grid_filter_radius, _window, _curvature, _threshold, lio_grid_duplicate_layer,
lio_grid_delete_layers) through the C ABI against the numpy restatement of tests/grid_filter_restate.py, which
tests/test_grid_filter_cpu.py pins, on the designed cases of tests/grid_filter_cases.py.  The comparison rule everywhere:
values that are not NaN are equal as words (signed zeros and infinities included), a NaN matches a NaN of any payload, a cell the
filter never writes is exactly 0x7fc00000; tolerance 0.  Two cross-checks against code merged before the filters, independent of
the restatement: MEAN in a radius against LIO_TERRAIN_SMOOTH and STDDEV over CROP against LIO_TERRAIN_EDGES, bit for bit.  Parity
with grid_map, EigenLab and Eigen themselves is unpinned (none can be built here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_filter_cases as K                                  # noqa: E402
import grid_filter_restate as R                                # noqa: E402
import terrain_restate as T                                    # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
COUNTS = ("n_visited", "n_written", "n_changed")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def upload(g, layers, res, pos):
    rows, cols = layers[0].shape
    g.set_layers(np.stack(layers), res, (rows * res, cols * res), pos)


def check_info(info, want_counts, shape, size, what):
    assert (info["rows"], info["cols"], info["window_size"]) == (shape[0], shape[1], size), (what, info)
    assert {k: int(info[k]) for k in COUNTS} == {k: want_counts[k] for k in COUNTS}, (what, info, want_counts)


def run_cases(pkg, cases):
    """every case on one object: layer 0 the input, the result in a layer that held something else before"""
    assert cases
    g = pkg.Grid()
    held = None
    for n, case in enumerate(cases):
        kind, key, args = case
        z = K.grid_of(key)
        res, pos = args[0], (args[1] if kind == "radius" else K.POSITIONS[1])     # (no window and no curvature reads the position)
        if held != (key, res, pos):
            upload(g, [z, np.full(z.shape, 7.0, f32)], res, pos)
            held = (key, res, pos)
        out_layer = 1 + n % 3                                  # 1 holds sevens or an earlier result, 2 and 3 are added or replaced
        if kind == "radius":
            info = g.filter_radius(0, out_layer, args[2], args[3])
        elif kind == "window":
            info = g.filter_window(0, out_layer, args[1], args[2], args[3], args[4], args[5])
        else:
            info = g.filter_curvature(0, out_layer)
        want, counts, size = K.expected(case)
        what = K.describe(case)
        assert R.identical(g.layer(out_layer), want, counts["mask"]), what
        check_info(info, counts, z.shape, size, what)
        assert np.array_equal(bits(g.layer(0)), bits(z)), what  # the input is only read
    g.close()


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_radius(pkg, shape):
    run_cases(pkg, K.radius_cases(shape))


def test_radius_of_32_cells(pkg):
    run_cases(pkg, K.radius_max_cases())


@pytest.mark.parametrize("edge", [R.INSIDE, R.CROP, R.EMPTY, R.EDGE_MEAN], ids=["inside", "crop", "empty", "mean"])
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_window(pkg, shape, edge):
    run_cases(pkg, K.window_cases(shape, edge))


@pytest.mark.parametrize("edge", [R.INSIDE, R.CROP, R.EMPTY, R.EDGE_MEAN], ids=["inside", "crop", "empty", "mean"])
def test_window_of_65_cells(pkg, edge):
    run_cases(pkg, K.window_max_cases(edge))


def test_curvature(pkg):
    run_cases(pkg, K.curvature_cases())


def test_threshold(pkg):
    cond, data, want = K.threshold_case()                      # threshold_filter_test.cpp
    g = pkg.Grid()
    for upper, threshold, set_to in ((1, 0.05, float("nan")), (0, 0.05, 7.0), (1, float("nan"), -0.0), (0, 0.03, 2.5), (1, 0.03, float("inf")),
                                     (0, float("nan"), float("nan"))):
        for in_place in (False, True):
            upload(g, [cond, data], 0.02, (1.0, 5.0))
            out_layer = 0 if in_place else 1
            info = g.filter_threshold(0, out_layer, upper, threshold, set_to)
            ref, counts = R.threshold_filter(cond, cond if in_place else data, upper, threshold, set_to)
            got = g.layer(out_layer)
            what = (upper, threshold, set_to, in_place)
            assert R.identical(got, ref), what
            check_info(info, counts, cond.shape, 0, what)
            if set_to != set_to:                               # the cells that were set hold (float)NAN's own word
                was = cond if in_place else data
                assert (bits(got)[np.isnan(ref) & ~np.isnan(was)] == R.QNAN_BITS).all(), what
            if not in_place:
                assert np.array_equal(bits(g.layer(0)), bits(cond)), what
    upload(g, [cond, data], 0.02, (1.0, 5.0))
    g.filter_threshold(0, 1, 1, 0.05, float("nan"))
    assert R.identical(g.layer(1), want)                       # the reference's expected layer
    g.close()


def test_window_in_place_reads_the_old_values(pkg):
    z = K.with_inf(33, 9)
    g = pkg.Grid()
    for op, edge, size, weights in ((R.SUM, R.CROP, 5, None), (R.STDDEV, R.EDGE_MEAN, 3, None), (R.MIN_OF_FINITES, R.INSIDE, 5, None),
                                    (R.WEIGHTED_SUM, R.EMPTY, 3, K.KERNEL_EDGE), (R.MEAN_OF_FINITES, R.INSIDE, 0, None)):
        upload(g, [z], K.RES, K.POSITIONS[1])
        a = g.filter_window(0, 1, op, edge, size, 0.1, weights)
        apart = g.layer(1)
        b = g.filter_window(0, 0, op, edge, size, 0.1, weights)
        assert np.array_equal(bits(g.layer(0)), bits(apart)), (op, edge, size)
        assert a.tolist() == b.tolist() and g.info().layer_mask == 0b11
        want, counts, _ = R.window_filter(z, K.RES, op, edge, size, 0.1, weights)
        assert R.identical(apart, want, counts["mask"])
    g.close()


def test_duplicate_then_delete(pkg):
    z = [K.plane(33, 9), K.with_inf(33, 9), K.all_nan(33, 9)]
    g = pkg.Grid()
    upload(g, z, K.RES, K.POSITIONS[1])
    before = g.info()
    g.duplicate_layer(1, 9)
    g.duplicate_layer(0, 2)                                    # replaces a layer the object holds
    g.duplicate_layer(1, 1)                                    # onto itself: nothing changes
    assert g.info().layer_mask == 0b1000000111
    for k, src in ((0, 0), (1, 1), (2, 0), (9, 1)):
        assert np.array_equal(bits(g.layer(k)), bits(z[src])), k
    g.delete_layers([2, 0])
    i = g.info()
    assert i.layer_mask == 0b1000000010 and (i.rows, i.cols, i.resolution) == (33, 9, K.RES)
    assert tuple(i.position) == tuple(before.position) and tuple(i.length) == tuple(before.length)
    assert np.array_equal(bits(g.layer(9)), bits(z[1]))
    with pytest.raises(pkg.LioError, match="no such layer"):
        g.layer(0)
    lib = pkg.load_library()
    for ids, why in (([0], "does not hold"), ([1, 5], "does not hold"), ([1, 1], "repeated"), ([16], "outside")):
        arr = (C.c_int32 * len(ids))(*ids)
        assert lib.lio_grid_delete_layers(g.h, arr, len(ids)) == -1 and why in lib.lio_last_error().decode(), ids
        assert g.info().layer_mask == 0b1000000010
    g.filter_curvature(9, 0)                                   # a deleted id is free again
    assert g.info().layer_mask == 0b1000000011
    g.delete_layers([0, 1, 9])
    i = g.info()
    assert i.layer_mask == 0 and (i.rows, i.cols) == (0, 0)     # no layer left: as lio_grid_create left it
    with pytest.raises(pkg.LioError, match="holds no layers"):
        g.delete_layers([0])
    g.close()


def test_refusals_leave_the_object_as_it_was(pkg):
    lib = pkg.load_library()
    z = K.with_inf(8, 5)
    sevens = np.full(z.shape, 7.0, f32)
    empty, g = pkg.Grid(), pkg.Grid()
    upload(g, [z, sevens], K.RES_BINARY, K.POSITIONS[0])
    info = np.zeros(1, pkg.GRID_FILTER_INFO_DTYPE)
    k9 = K.KERNEL_EDGE.ravel(order="F").ctypes.data_as(C.POINTER(C.c_float))
    far = K.RADIUS_REFUSED_CELLS * K.RES_BINARY
    on_an_empty_object = (
        lambda h: lib.lio_grid_filter_radius(h, 0, 2, 0, 0.5, info.ctypes.data),
        lambda h: lib.lio_grid_filter_window(h, 0, 2, 0, 1, 3, 0.0, None, info.ctypes.data),
        lambda h: lib.lio_grid_filter_curvature(h, 0, 2, info.ctypes.data),
        lambda h: lib.lio_grid_filter_threshold(h, 0, 0, 1, 0.5, 0.0, info.ctypes.data),
        lambda h: lib.lio_grid_duplicate_layer(h, 0, 2),
    )
    for call in on_an_empty_object:
        assert call(empty.h) == -1 and "holds no layers" in lib.lio_last_error().decode()
        assert empty.info().layer_mask == 0
    more = (
        (lambda: lib.lio_grid_filter_radius(g.h, 5, 2, 0, 0.5, info.ctypes.data), "no such layer"),
        (lambda: lib.lio_grid_filter_window(g.h, 5, 2, 0, 1, 3, 0.0, None, info.ctypes.data), "no such layer"),
        (lambda: lib.lio_grid_filter_curvature(g.h, 5, 2, info.ctypes.data), "no such layer"),
        (lambda: lib.lio_grid_filter_threshold(g.h, 5, 1, 1, 0.5, 0.0, info.ctypes.data), "no such layer"),
        (lambda: lib.lio_grid_filter_threshold(g.h, 0, 5, 1, 0.5, 0.0, info.ctypes.data), "no such layer to set"),      # an absent output layer
        (lambda: lib.lio_grid_filter_radius(g.h, 0, 0, 1, 0.5, info.ctypes.data), "out_layer is in_layer"),
        (lambda: lib.lio_grid_filter_curvature(g.h, 1, 1, info.ctypes.data), "out_layer is in_layer"),
        (lambda: lib.lio_grid_filter_radius(g.h, 0, 1, 0, far, info.ctypes.data), "32 cells"),                         # 32.5 cells
        (lambda: lib.lio_grid_filter_window(g.h, 0, 1, 0, 1, 0, 67 * K.RES_BINARY, None, info.ctypes.data), "32 cells"),        # derives 67
        (lambda: lib.lio_grid_filter_window(g.h, 0, 1, 6, 1, 3, 0.0, k9, info.ctypes.data), "disagree"),               # crop with weights
        (lambda: lib.lio_grid_filter_window(g.h, 0, 1, 6, 1, 0, 3 * K.RES_BINARY, k9, info.ctypes.data), "disagree"),  # at a derived size of 3
    )
    assert lib.lio_grid_duplicate_layer(g.h, 5, 2) == -1 and "no such layer" in lib.lio_last_error().decode() and g.info().layer_mask == 0b11
    for call, why in more:
        info.view(np.int8)[:] = -1
        assert call() == -1 and why in lib.lio_last_error().decode(), (why, lib.lio_last_error().decode())
        assert not info.view(np.int8).any()
        i = g.info()
        assert i.layer_mask == 0b11 and (i.rows, i.cols) == (8, 5)
        assert np.array_equal(bits(g.layer(0)), bits(z)) and np.array_equal(bits(g.layer(1)), bits(sevens))
    # what is allowed next to them: 32 cells, a window of 65, a derived 65, weights at a derived size of 1 with crop
    assert lib.lio_grid_filter_radius(g.h, 0, 1, 0, K.RADIUS_MAX_CELLS * K.RES_BINARY, None) == 0
    assert lib.lio_grid_filter_window(g.h, 0, 1, 0, 1, 65, 0.0, None, None) == 0
    assert lib.lio_grid_filter_window(g.h, 0, 1, 0, 1, 0, 65 * K.RES_BINARY, None, info.ctypes.data) == 0 and info["window_size"][0] == 65
    k1 = (C.c_float * 1)(-2.0)
    assert lib.lio_grid_filter_window(g.h, 0, 1, 6, 1, 0, 0.0, k1, info.ctypes.data) == 0 and info["window_size"][0] == 1
    fin = np.isfinite(z)
    got = g.layer(1)
    assert np.array_equal(got[fin], f32(-2.0) * z[fin])
    for o in (empty, g):
        o.close()


def test_against_the_terrain_layers(pkg):
    """scene A of tests/test_gpu_terrain.py by its recipe: lio_terrain_layers' smooth and edges layers are the same arithmetic
    as MEAN in a radius and STDDEV over CROP"""
    g = pkg.Grid()
    for pos in ((0.0, 0.0), (60.0, -35.0)):
        grid = T.scene_a(pos)
        rows, cols = grid.shape
        assert (rows, cols) == (48, 36)
        cfg = pkg.terrain_default_config(normal_radius=0.3, smooth_radius=0.6, edge_window_length=0.75)
        d, tinfo = pkg.terrain_layers(grid, 0.25, (rows * 0.25, cols * 0.25), pos, cfg)
        upload(g, [grid, d["slope"]], 0.25, pos)
        info = g.filter_radius(0, 2, pkg.GF_MEAN, 0.6)
        assert np.array_equal(bits(g.layer(2)), bits(d["smooth"])), pos        # every word, NaN payloads included
        assert info["n_visited"] == rows * cols and info["n_written"] == np.isfinite(d["smooth"]).sum()
        for size, length in ((tinfo.edge_window_size, 0.0), (0, 0.75)):
            info = g.filter_window(1, 3, pkg.GW_STDDEV, pkg.GW_CROP, size, length)
            assert info["window_size"] == tinfo.edge_window_size == 3
            got, want = g.layer(3), d["edges"]
            assert R.identical(got, want), pos
    g.close()


def test_kernel_time_hook(pkg):
    lib = pkg.load_library()
    g = pkg.Grid()
    upload(g, [K.plane(69, 19)], K.RES, K.POSITIONS[0])
    ms = C.c_float(-1.0)
    assert lib.lio_grid_filter_debug_kernel_ms(1, None) == 0
    g.filter_radius(0, 1, pkg.GF_MEAN, 0.33)
    assert lib.lio_grid_filter_debug_kernel_ms(1, C.byref(ms)) == 0 and ms.value > 0.0
    g.duplicate_layer(0, 2)                                    # no kernel of the library's
    assert lib.lio_grid_filter_debug_kernel_ms(0, C.byref(ms)) == 0 and ms.value == 0.0
    g.filter_curvature(0, 1)
    assert lib.lio_grid_filter_debug_kernel_ms(0, C.byref(ms)) == 0 and ms.value == 0.0            # off again
    g.close()
