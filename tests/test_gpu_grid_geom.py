"""lio_grid_submap, lio_grid_move, lio_grid_extend_to_include and lio_grid_add_data_from on the device through the C ABI: every
layer's words, the geometry and every counter against the restatement (tests/grid_geom_restate.py: the reference's serial
loops, `move` on a real circular buffer and unwrapped), which tests/test_grid_geom_cpu.py holds against the reference's own test
values and against the header the kernels run.  The tolerance is 0: the device does only correctly rounded fp64 operations in
the stated order.  The shapes are tests/grid_geom_cases.py's: rows in {1, 2, 63, 64, 65, 257}, cols in {1, 2, 5}, 1, 10 and 16
layers, cells holding NaN with payloads, +-inf and -0.0f.  (Grids on different devices need two devices: not run here.)"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_restate as gs                               # noqa: E402
import grid_transform_restate as RT                            # noqa: E402
import grid_geom_restate as R                                  # noqa: E402
import grid_geom_cases as K                                    # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SHAPES = K.shapes()
SHAPE_IDS = [f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES]


def upload(pkg, g, layers, grid=None):
    grid = grid or pkg.Grid()
    grid.set_layers(np.asarray(layers, f32), g.res, g.length, g.pos)
    return grid


def ids_of(mask):
    return [k for k in range(16) if (mask >> k) & 1]


def words_of(grid):
    return np.stack([np.ascontiguousarray(grid.layer(k)).view(u32) for k in ids_of(grid.info().layer_mask)])


def same_map(grid, want, what):
    """the object's geometry, layer ids and every word against the restated map"""
    d = grid.info()
    assert (d.rows, d.cols) == want.size and d.resolution == want.res, what
    assert tuple(d.length) == want.length and tuple(d.position) == want.pos, (what, tuple(d.position), want.pos)
    assert ids_of(d.layer_mask) == sorted(want.ids), what
    got, ref = words_of(grid), want.words(sorted(want.ids))
    assert np.array_equal(got, ref), (what, np.argwhere(got != ref)[:5])


def same_geometry(info, want, what):
    assert (info["rows"], info["cols"]) == want.size and tuple(info["length"]) == want.length and tuple(info["position"]) == want.pos, what


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_move(pkg, shape):
    rows, cols, n_layers, res = shape
    g = K.geometry(rows, cols, res)
    layers = K.layers_of((rows, cols), n_layers, rows * 7 + cols)
    grid = pkg.Grid()
    n_moved = 0
    for position in K.move_targets(g):
        upload(pkg, g, layers, grid)
        want, info_want = K.expect_move(g, layers, position)
        info = grid.move(position)
        assert (info["moved"], tuple(info["index_shift"]), tuple(info["position"]), info["n_cells_cleared"]) == \
            (info_want["moved"], info_want["index_shift"], info_want["position"], info_want["n_cells_cleared"]), position
        same_map(grid, want, position)
        n_moved += info["moved"]
    assert n_moved >= 15                                       # (on one row or column, size - 1 is no shift)
    grid.close()


def test_move_by_fractions_of_a_cell(pkg):
    """0.49 resolution: no move (the position keeps its bits); exactly 0.5 resolution: one cell; a resolution of 0.1"""
    for res in (0.25, 0.1):
        g = gs.Geometry(5, 4, res)
        layers = K.layers_of((5, 4), 2, 3)
        for position, shift in (((0.49 * res, -0.49 * res), (0, 0)), ((0.5 * res, 0.0), (-1, 0)), ((0.0, -0.5 * res), (0, 1)), ((-0.5 * res, 0.5 * res), (1, -1))):
            grid = upload(pkg, g, layers)
            want, info_want = K.expect_move(g, layers, position)
            info = grid.move(position)
            assert tuple(info["index_shift"]) == shift == info_want["index_shift"] and info["moved"] == (shift != (0, 0)), (res, position)
            assert tuple(info["position"]) == info_want["position"] == (-shift[0] * res + 0.0, -shift[1] * res + 0.0)
            same_map(grid, want, (res, position))
            grid.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_submap(pkg, shape):
    rows, cols, n_layers, res = shape
    g = K.geometry(rows, cols, res)
    layers = K.layers_of((rows, cols), n_layers, rows * 11 + cols)
    src, dst = upload(pkg, g, layers), pkg.Grid()
    n_fail = 0
    for position, length in K.submap_windows(g):
        want, info_want = K.expect_submap(g, layers, position, length)
        info = src.submap(dst, position, length)
        assert info["success"] == (want is not None), (position, length)
        if want is None:
            n_fail += 1
            assert dst.info().layer_mask == 0 and not info.tobytes().strip(b"\0")
            continue
        same_geometry(info, want, (position, length))
        assert tuple(info["top_left"]) == info_want["top_left"] and tuple(info["requested_index"]) == info_want["requested"], (position, length)
        same_map(dst, want, (position, length))
    assert n_fail >= 3
    assert np.array_equal(words_of(src), layers.view(u32))     # src is only read
    src.close()
    dst.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_extend_and_add(pkg, shape):
    rows, cols, n_layers, res = shape
    g = K.geometry(rows, cols, res)
    layers = K.layers_of((rows, cols), n_layers, rows * 13 + cols)
    grid, other = pkg.Grid(), pkg.Grid()
    resized = []
    for case in K.add_cases(g, n_layers, rows <= 65):
        for extend_only in (True, False):
            want, other_map, cnt = K.expect_add(g, layers, case, extend_only)
            upload(pkg, g, layers, grid)
            other_layers = np.stack([other_map.data[k] for k in case["other_ids"]])
            upload(pkg, case["other"], other_layers, other)
            if extend_only:
                info = grid.extend_to_include(other)
                assert (info["resized"], info["n_cells_kept"], info["n_index_outside"]) == (cnt["resized"], cnt["n_cells_kept"], cnt["n_index_outside"]), case
            else:
                info = grid.add_data_from(other, case["extend"], case["overwrite"], case["layer_ids"], case["basic"])
                names = ("resized", "n_cells_skipped_valid", "n_cells_outside_other", "n_index_outside", "n_values_copied")
                assert tuple(info[k] for k in names) == tuple(cnt[k] for k in names), (case, info)
            same_geometry(info, want, case)
            same_map(grid, want, case)
            assert np.array_equal(words_of(other), other_layers.view(u32)), case           # other is only read
            resized.append(int(info["resized"]))
    assert 1 in resized and (0 in resized or rows > 65)         # (every placement but the disjoint one is left out of the large shapes)
    grid.close()
    other.close()


def nearest(grid, k, p):
    return float(grid.sample([p], (k,))[0][0, 0])


def constant(size, *values):
    return np.stack([np.full(size, v, f32) for v in values])


def test_reference_literals_through_the_abi(pkg):
    """GridMapTest.cpp Move and the three AddDataFrom tests.  An upload's layers are 0 .. n - 1, so where map2 lacks a layer
    of map1 it holds that id all NaN: addDataFrom copies no NaN, which leaves the reference's case."""
    nan = float("nan")
    # Move, :52-89
    m = upload(pkg, gs.Geometry(8, 5, 1.0), constant((8, 5), 0.0))
    info = m.move((-3.0, -2.0))
    valid = np.zeros((8, 5), bool)
    valid[:5, :3] = True
    assert info["moved"] == 1 and tuple(info["index_shift"]) == (3, 2) and tuple(info["position"]) == (-3.0, -2.0) and info["n_cells_cleared"] == 25
    assert np.array_equal(np.isfinite(m.layer(0)), valid)
    # ExtendMapAligned, :359-384: zero 0, one 1, two 2
    m1 = upload(pkg, gs.Geometry(5, 5, 1.0), constant((5, 5), 0.0, 1.0))
    m2 = upload(pkg, gs.Geometry(3, 3, 1.0, (2.0, 2.0)), constant((3, 3), nan, 1.1, 2.0))
    info = m1.add_data_from(m2, True, True, None, (0, 1))
    d = m1.info()
    assert d.layer_mask == 7 and info["resized"] == 1 and tuple(d.length) == (6.0, 6.0) and tuple(d.position) == (0.5, 0.5)
    assert abs(nearest(m1, 1, (2.0, 2.0)) - 1.1) <= 1e-4 and nearest(m1, 1, (-2.0, -2.0)) == 1.0 and nearest(m1, 0, (0.0, 0.0)) == 0.0
    assert nearest(m1, 2, (3.0, 3.0)) == 2.0                   # isInside(3, 3)
    # ExtendMapNotAligned, :386-417: nan 0, one 1, zero 2, two 3
    m1 = upload(pkg, gs.Geometry(6, 6, 1.0), constant((6, 6), nan, 1.0, 0.0))
    m2 = upload(pkg, gs.Geometry(3, 3, 1.0, (3.2, 3.2)), constant((3, 3), 1.0, 1.1, nan, 2.0))
    m1.add_data_from(m2, True, False, [0], (0, 1, 2))
    d = m1.info()
    assert d.layer_mask == 7 and tuple(d.length) == (8.0, 8.0) and tuple(d.position) == (1.0, 1.0)
    assert math.isnan(nearest(m1, 0, (-2.0, -2.0))) and nearest(m1, 1, (0.0, 0.0)) == 1.0 and nearest(m1, 0, (3.0, 3.0)) == 1.0
    assert m1.sample([(4.0, 4.0)], (0,))[1][0, 0] != pkg.GRID_OUTSIDE
    # CopyData, :419-446: zero 0, one 1, two 2
    m1 = upload(pkg, gs.Geometry(5, 5, 1.0), constant((5, 5), 0.0, nan))
    m2 = upload(pkg, gs.Geometry(3, 3, 1.0, (2.0, 2.0)), constant((3, 3), nan, 1.0, 2.0))
    info = m1.add_data_from(m2, False, False, None, (0, 1))
    d = m1.info()
    assert d.layer_mask == 7 and info["resized"] == 0 and tuple(d.length) == (5.0, 5.0) and tuple(d.position) == (0.0, 0.0)
    assert nearest(m1, 1, (2.0, 2.0)) == 1.0 and math.isnan(nearest(m1, 1, (-2.0, -2.0))) and nearest(m1, 0, (0.0, 0.0)) == 0.0
    assert m1.sample([(3.0, 3.0)], (0,))[1][0, 0] == pkg.GRID_OUTSIDE


def test_accumulation_loop(pkg):
    """transform into the map frame, add into a persistent map that extends itself, move it onto the vehicle, sample: equal to
    the same steps done with the restatements"""
    rng = np.random.default_rng(21)
    g = gs.Geometry(24, 17, 0.25, (2.0, -1.0))
    local = np.stack([rng.uniform(-1, 1, (24, 17)), rng.uniform(0, 1, (24, 17))]).astype(f32)
    local[0][rng.random((24, 17)) < 0.1] = np.nan
    yaw = math.radians(30.0)
    T = [[math.cos(yaw), -math.sin(yaw), 0.0, 3.0], [math.sin(yaw), math.cos(yaw), 0.0, -1.0], [0.0, 0.0, 1.0, 0.5]]
    pg = gs.Geometry(12, 9, 0.25, (0.1, 0.3))
    persistent = K.layers_of((12, 9), 2, 22)
    vehicle = (3.3, 0.7)
    # the restatements
    moved = RT.serial(g, local, T, 0, 0.0)
    want = R.GridMap.of(pg, persistent, basic=[0])
    cnt = want.add_data_from(R.GridMap.of(moved.g, moved.words.view(f32)), True, False, True)
    info_move = R.lib_move(want, vehicle)
    positions = np.array(want.pos) + (rng.random((200, 2)) - 0.5) * 1.1 * np.array(want.length)
    vals, used, _ = gs.sample(want, [want.data[0], want.data[1]], positions, gs.LINEAR)
    # the device
    src, frame, grid = upload(pkg, g, local), pkg.Grid(), upload(pkg, pg, persistent)
    src.transform(frame, T, 0, 0.0)
    info = grid.add_data_from(frame, True, False, None, (0,))
    assert all(info[k] == cnt[k] for k in cnt) and info["resized"] == 1, (info, cnt)
    im = grid.move(vehicle)
    assert tuple(im["index_shift"]) == info_move["index_shift"] and im["n_cells_cleared"] == info_move["n_cells_cleared"] and im["moved"] == 1
    same_map(grid, want, "accumulated")
    got, got_used, _ = grid.sample(positions, (0, 1), method=pkg.GRID_LINEAR)
    assert np.array_equal(got.view(u32), vals.view(u32)) and np.array_equal(got_used, used)


def test_memory_does_not_grow(pkg):
    """twenty repeats of each call: what lio_grid_memory reports after the third and later calls never exceeds the first two"""
    g = gs.Geometry(65, 5, 0.25)
    layers = K.layers_of((65, 5), 10, 5)
    other_g = gs.Geometry(7, 4, 0.25, (12.0, 1.0))
    other = upload(pkg, other_g, K.layers_of((7, 4), 10, 6))
    grid, dst = upload(pkg, g, layers), pkg.Grid()
    for call in ("move", "submap", "extend", "add"):
        seen = []
        for k in range(20):
            if call == "move":
                assert grid.move((0.5 * (k % 2), 0.25))["moved"] == 1
            elif call == "submap":
                assert grid.submap(dst, (0.0, 0.0), (3.0, 0.8))["success"] == 1
            else:
                upload(pkg, g, layers, grid)
                info = grid.extend_to_include(other) if call == "extend" else grid.add_data_from(other, True, True, None, (0,))
                assert info["resized"] == 1
            seen.append(grid.memory() + dst.memory())
        assert max(seen[2:]) <= max(seen[:2]), (call, seen)


def test_refusals_that_need_an_object(pkg):
    lib = pkg.load_library()
    g = gs.Geometry(64, 64, 0.25)
    layers = K.layers_of((64, 64), 2, 9)
    grid, empty = upload(pkg, g, layers), pkg.Grid()
    three = upload(pkg, gs.Geometry(4, 3, 0.25, (1.0, 1.0)), K.layers_of((4, 3), 3, 10))
    far = upload(pkg, gs.Geometry(4, 3, 0.25, (5.0e6, 0.0)), K.layers_of((4, 3), 1, 11))
    wide = upload(pkg, gs.Geometry(4, 3, 0.25, (15000.0, 15000.0)), K.layers_of((4, 3), 1, 12))
    held = upload(pkg, gs.Geometry(2, 2, 1.0), constant((2, 2), 5.0))

    def pair(v):
        return (C.c_double * 2)(*v)

    def ids(v):
        return (C.c_int32 * len(v))(*v)

    calls = [(lambda: lib.lio_grid_submap(empty.h, pair((0, 0)), pair((1, 1)), held.h, None), -1, "no layers"),
             (lambda: lib.lio_grid_submap(grid.h, pair((0, 0)), pair((1, 1)), grid.h, None), -1, "same object"),
             (lambda: lib.lio_grid_move(empty.h, pair((0, 0)), None), -1, "no layers"),
             (lambda: lib.lio_grid_move(grid.h, pair((0.25 * 2.0 ** 30, 0.0)), None), -1, "2^30"),
             (lambda: lib.lio_grid_move(grid.h, pair((0.0, -1e300)), None), -1, "2^30"),
             (lambda: lib.lio_grid_extend_to_include(empty.h, grid.h, None), -1, "no layers"),
             (lambda: lib.lio_grid_extend_to_include(grid.h, empty.h, None), -1, "no layers"),
             (lambda: lib.lio_grid_extend_to_include(grid.h, grid.h, None), -1, "same object"),
             (lambda: lib.lio_grid_extend_to_include(grid.h, far.h, None), -3, "2^24"),
             (lambda: lib.lio_grid_extend_to_include(grid.h, wide.h, None), -3, "2^31 - 1024"),
             (lambda: lib.lio_grid_add_data_from(grid.h, far.h, 1, 1, None, 0, 0, None), -3, "2^24"),
             (lambda: lib.lio_grid_add_data_from(grid.h, empty.h, 1, 1, None, 0, 0, None), -1, "no layers"),
             (lambda: lib.lio_grid_add_data_from(empty.h, grid.h, 1, 1, None, 0, 0, None), -1, "no layers"),
             (lambda: lib.lio_grid_add_data_from(grid.h, three.h, 1, 1, ids([3]), 1, 0, None), -1, "other does not hold"),
             (lambda: lib.lio_grid_add_data_from(grid.h, three.h, 1, 1, ids([0, 2, 0]), 3, 0, None), -1, "repeated"),
             (lambda: lib.lio_grid_add_data_from(grid.h, three.h, 1, 1, ids([2]), 1, 1 << 2, None), -1, "basic_mask"),
             (lambda: lib.lio_grid_add_data_from(grid.h, three.h, 3, 1, None, 0, 0, None), -1, "0 or 1")]
    for k, (call, status, why) in enumerate(calls):
        rc = call()
        assert rc == status and why in lib.lio_last_error().decode(), (k, rc, lib.lio_last_error().decode())
        d = grid.info()
        assert (d.rows, d.cols, d.layer_mask, tuple(d.position)) == (64, 64, 3, (0.0, 0.0)) and np.array_equal(words_of(grid), layers.view(u32)), k
        assert held.info().layer_mask == 1 and np.array_equal(held.layer(0), np.full((2, 2), 5.0, f32)), k
    # the largest shift that is not refused clears everything
    info = grid.move((0.25 * (2.0 ** 30 - 1.0), 0.0))
    assert info["moved"] == 1 and info["index_shift"][0] == -(2 ** 30 - 1) and info["n_cells_cleared"] == 64 * 64
    assert (words_of(grid) == R.QNAN_BITS).all()
    # nothing to extend: nothing touched
    upload(pkg, g, layers, grid)
    info = grid.extend_to_include(three)
    assert info["resized"] == 0 and (info["rows"], info["cols"]) == (64, 64) and np.array_equal(words_of(grid), layers.view(u32))
