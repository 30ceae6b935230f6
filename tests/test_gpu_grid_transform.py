"""lio_grid_transform and lio_grid_to_occupancy on the device through the C ABI: every layer's words, the new geometry and the
three counts against the restatement (tests/grid_transform_restate.py: the serial loop of GridMap::getTransformedMap), which
tests/test_grid_transform_cpu.py holds against the reference's own test values and against the header the kernels run.  All
grids are 67 x 45, 64 x 64 or smaller.  (Grids on different devices need two devices and more than
LIO_GRID_TRANSFORM_MAX_SOURCE_CELLS source cells a 1.7 GB layer: neither refusal is run here.)"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_restate as gs                               # noqa: E402
import grid_transform_restate as R                             # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
ROT90 = [[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]                # GridMapTest.cpp:103-119


def rot(yaw=0.0, pitch=0.0, t=(0.0, 0.0, 0.0)):
    """Rz(yaw) Ry(pitch) with the translation t, as rows of [R | t]"""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    return [[cy * cp, -sy, cy * sp, t[0]], [sy * cp, cy, sy * sp, t[1]], [-sp, 0.0, cp, t[2]]]


def index_layer(rows, cols):
    """the source's column-major linear index: which source cell a new cell's values came from"""
    return np.arange(rows * cols, dtype=f32).reshape(cols, rows).T


def upload(pkg, g, layers):
    grid = pkg.Grid()
    grid.set_layers(np.asarray(layers, f32), g.res, g.length, g.pos)
    return grid


def words_of(grid, n_layers):
    return np.stack([np.ascontiguousarray(grid.layer(k)).view(u32) for k in range(n_layers)])


def check(pkg, g, layers, T, height_layer=0, ratio=0.25, what=None):
    """transform on the device, compare with the serial loop -> (dst, the restated map, info)"""
    layers = np.asarray(layers, f32)
    want = R.serial(g, layers, T, height_layer, ratio)
    src, dst = upload(pkg, g, layers), pkg.Grid()
    info = src.transform(dst, T, height_layer, ratio)
    d = dst.info()
    assert (info["rows"], info["cols"]) == (d.rows, d.cols) == want.g.size, what
    assert tuple(info["length"]) == tuple(d.length) == want.g.length and tuple(info["position"]) == tuple(d.position) == want.g.pos, what
    assert d.resolution == g.res and d.layer_mask == (1 << len(layers)) - 1, what
    assert (info["n_source_cells"], info["n_samples_outside"], info["n_cells_written"]) == want.counters(), what
    got = words_of(dst, len(layers))
    assert np.array_equal(got, want.words), (what, np.argwhere(got != want.words)[:5])
    assert np.array_equal(words_of(src, len(layers)), layers.view(u32)), what                  # src is only read
    src.close()
    return dst, want, info


def test_reference_literal(pkg):
    """GridMapTest.cpp:91-129"""
    g = gs.Geometry(10, 20, 0.1)
    layer = np.zeros((1, 10, 20), f32)
    layer[0, 0, 0] = 1.0
    dst, want, info = check(pkg, g, layer, ROT90)
    assert (info["rows"], info["cols"]) == (20, 10) and abs(info["length"][0] - 2.0) <= 1e-6 and abs(info["length"][1] - 1.0) <= 1e-6
    assert dst.layer(0)[19, 0] == 1.0


def test_identity_copies_every_bit(pkg):
    rng = np.random.default_rng(1)
    g = gs.Geometry(24, 17, 0.25)
    other = rng.uniform(-1, 1, (24, 17)).astype(f32)
    other.view(u32)[rng.random((24, 17)) < 0.2] = 0xffc54321
    layers = np.stack([rng.uniform(-3, 3, (24, 17)).astype(f32), other, index_layer(24, 17)])
    layers[0, 4, 4], layers[1, 3, 3] = 0.0, -0.0                 # (a height of -0.0 would come out as -0.0 + t_z = +0.0, as in the reference)
    dst, _, info = check(pkg, g, layers, rot(), ratio=0.0)
    assert np.array_equal(words_of(dst, 3), layers.view(u32))
    assert info["n_cells_written"] == 24 * 17 and info["n_samples_outside"] == 0


def test_ties_show_the_winner(pkg):
    """a flat layer: every sample of a new cell ties, and the index layer shows which one the loop left there"""
    g = gs.Geometry(67, 45, 0.25, (1.5, -2.25))
    _, want, _ = check(pkg, g, [np.ones((67, 45), f32), index_layer(67, 45)], rot(math.radians(30.0), 0.0, (3.0, -1.0, 0.5)))
    cells = want.winner >= 0
    assert np.array_equal(want.layers[1][cells], (want.winner[cells] // 5).astype(f32))
    assert (~cells).any()                                      # the rotated map has corners nothing reaches


def test_float_class_both_branches(pkg):
    """pitch 1e-9 on a flat 1.0: every z rounds to 1.0f, the doubles lie on both sides of it; samples cross into neighbours"""
    g = gs.Geometry(33, 21, 0.25)
    layers = [np.ones((33, 21), f32), index_layer(33, 21)]
    T = rot(0.0, 1e-9)
    ruled = R.by_rule(g, np.asarray(layers, f32), T, 0, 0.6)
    assert (ruled.branch == 0).sum() >= 1 and (ruled.branch == 1).sum() >= 1
    crowded = [v for v in np.unique(ruled.layers[0][ruled.winner >= 0])]
    assert crowded == [f32(1.0)]
    _, want, _ = check(pkg, g, layers, T, ratio=0.6)
    assert np.array_equal(want.winner, ruled.winner)


def test_contention(pkg):
    """an 80 degree pitch folds 64 rows into 11: many source cells per new cell"""
    rng = np.random.default_rng(5)
    g = gs.Geometry(64, 64, 0.25)
    _, want, info = check(pkg, g, [rng.uniform(-1, 1, (64, 64)).astype(f32), index_layer(64, 64)], rot(0.0, math.radians(80.0)))
    assert want.g.size[0] <= 16 and info["n_cells_written"] * 4 < 64 * 64


def test_skipped_and_missing_cells(pkg):
    rng = np.random.default_rng(6)
    g = gs.Geometry(40, 31, 0.2, (1e3, -3e3))
    height = rng.uniform(-1, 1, (40, 31)).astype(f32)
    height[rng.random((40, 31)) < 0.15] = np.nan
    height[rng.random((40, 31)) < 0.05] = np.inf
    height[5, 5] = -np.inf
    other = rng.uniform(-1, 1, (40, 31)).astype(f32)
    other.view(u32)[rng.random((40, 31)) < 0.2] = 0x7fc12345
    dst, want, info = check(pkg, g, [height, other, index_layer(40, 31)], rot(-2.0, 0.05, (-7.0, 2.0, 1.0)), ratio=0.0)
    assert info["n_source_cells"] == np.isfinite(height).sum() < height.size
    got = words_of(dst, 3)
    empty = want.winner < 0
    assert empty.any() and (got[:, empty] == R.QNAN_BITS).all()                # unreached: the quiet NaN in every layer
    assert (got[1] == 0x7fc12345).any()                                        # a NaN of another layer is copied with its bits


def test_ratio_above_a_half_leaves_the_map(pkg):
    g = gs.Geometry(21, 30, 0.25, (-4.0, 9.0))
    rng = np.random.default_rng(7)
    _, want, info = check(pkg, g, [rng.uniform(0, 0.1, (21, 30)).astype(f32), index_layer(21, 30)], rot(), ratio=0.6)
    assert want.n_samples_outside > 0 and info["n_samples_outside"] == want.n_samples_outside


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (3, 1), (5, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_odd_shapes(pkg, shape):
    """new grids of 1, 3 .. cells (no whole quad for the gather) and one that ends inside a quad"""
    rows, cols = shape
    rng = np.random.default_rng(rows * 31 + cols)
    g = gs.Geometry(rows, cols, 0.5, (-2.0, 7.0))
    layers = [rng.uniform(-1, 1, (rows, cols)).astype(f32), index_layer(rows, cols)]
    for T in (rot(), rot(0.7, 0.1), ROT90):
        check(pkg, g, layers, T, what=T)


def test_sixteen_layers(pkg):
    rng = np.random.default_rng(8)
    g = gs.Geometry(19, 23, 0.3, (0.5, 0.25))
    layers = rng.uniform(-1, 1, (16, 19, 23)).astype(f32)
    layers[15] = index_layer(19, 23)
    layers[3][rng.random((19, 23)) < 0.3] = np.nan
    check(pkg, g, layers, rot(1.1, -0.2, (1.0, 2.0, 3.0)), height_layer=7)
    check(pkg, g, layers, rot(1.1, -0.2, (1.0, 2.0, 3.0)), height_layer=3)     # a height layer with holes, not layer 0


def test_repeatable(pkg):
    rng = np.random.default_rng(9)
    g = gs.Geometry(64, 64, 0.25)
    layers = np.stack([np.round(rng.uniform(-1, 1, (64, 64)), 1).astype(f32), index_layer(64, 64)])
    src, a, b = upload(pkg, g, layers), pkg.Grid(), pkg.Grid()
    T = rot(0.4, math.radians(75.0))
    ia, ib = src.transform(a, T, 0, 0.25), src.transform(b, T, 0, 0.25)
    ic = src.transform(a, T, 0, 0.25)                          # into a grid that already holds the result
    assert ia.tobytes() == ib.tobytes() == ic.tobytes()
    assert words_of(a, 2).tobytes() == words_of(b, 2).tobytes()


def test_chaining(pkg):
    """lio_grid_sample and lio_grid_region_reduce on dst equal the same calls on the restated map, uploaded"""
    rng = np.random.default_rng(10)
    g = gs.Geometry(45, 38, 0.25, (2.0, -1.0))
    layers = [rng.uniform(-1, 1, (45, 38)).astype(f32), rng.uniform(0, 1, (45, 38)).astype(f32)]
    dst, want, _ = check(pkg, g, layers, rot(math.radians(30.0), 0.02, (1.0, 1.0, 0.0)))
    ref = upload(pkg, want.g, want.layers)
    lo = np.array(want.g.pos) - 0.55 * np.array(want.g.length)
    pos = lo + rng.random((500, 2)) * 1.1 * np.array(want.g.length)
    for method in (pkg.GRID_NEAREST, pkg.GRID_LINEAR, pkg.GRID_CUBIC):
        va, ua, _ = dst.sample(pos, (0, 1), method=method)
        vb, ub, _ = ref.sample(pos, (0, 1), method=method)
        assert np.array_equal(va.view(u32), vb.view(u32)) and np.array_equal(ua, ub)
    regions = [("circle", want.g.pos[0], want.g.pos[1], 2.0), ("line", lo[0], lo[1], want.g.pos[0], want.g.pos[1]),
               ("polygon", [(want.g.pos[0] - 1, want.g.pos[1] - 1), (want.g.pos[0] + 2, want.g.pos[1]), (want.g.pos[0], want.g.pos[1] + 2)])]
    sa, na, ta, _ = dst.region_reduce(regions, (0, 1))
    sb, nb, tb, _ = ref.region_reduce(regions, (0, 1))
    assert sa.tobytes() == sb.tobytes() and np.array_equal(na, nb) and np.array_equal(ta, tb) and na.sum() > 0


def test_refusals_that_need_an_object(pkg):
    lib = pkg.load_library()
    g = gs.Geometry(67, 45, 0.25)
    src = upload(pkg, g, [np.zeros((67, 45), f32), np.ones((67, 45), f32)])
    held = np.stack([np.full((4, 3), 5.0, f32)])
    dst = upload(pkg, gs.Geometry(4, 3, 1.0), held)
    empty = pkg.Grid()

    def call(s=src, d=dst, T=rot(), height=0, ratio=0.25):
        t = (C.c_double * 12)(*[v for row in T for v in row])
        return lib.lio_grid_transform(s.h, t, height, ratio, d.h, None), lib.lio_last_error().decode()

    def scaled(s):
        return [[s, 0.0, 0.0, 0.0], [0.0, s, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]

    cases = [(dict(s=empty), -1, "no layers"), (dict(height=2), -1, "height_layer"), (dict(height=-1), -1, "height_layer"), (dict(height=16), -1, "height_layer"),
             (dict(d=src), -1, "same object"), (dict(T=rot(0.0, math.pi / 2)), -1, "no cell"), (dict(T=scaled(0.001)), -1, "no cell"),
             (dict(T=[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1e300, 0.0]]), -1, "overflow"),
             (dict(T=scaled(1e6)), -3, "2^24"), (dict(T=scaled(850.0)), -3, "2^31 - 1024")]
    for kw, status, why in cases:
        rc, msg = call(**kw)
        assert rc == status and why in msg, (kw, rc, msg)
        d = dst.info()
        assert (d.rows, d.cols, d.layer_mask) == (4, 3, 1) and np.array_equal(dst.layer(0), held[0]), kw      # dst untouched
    assert call()[0] == 0 and dst.info().layer_mask == 3 and (dst.info().rows, dst.info().cols) == (67, 45)
    # the occupancy call: an object without layers, an absent layer
    data = np.full(67 * 45, 77, np.int8)
    for grid, layer, why in ((empty, 0, "no such layer"), (src, 2, "no such layer"), (src, -1, "no such layer"), (src, 16, "no such layer")):
        assert lib.lio_grid_to_occupancy(grid.h, layer, 0.0, 1.0, data.ctypes.data, data.size, None) == -1 and why in lib.lio_last_error().decode()
    assert (data == 77).all()


def test_occupancy(pkg):
    rng = np.random.default_rng(11)
    g = gs.Geometry(67, 45, 0.25, (3.0, -6.5))
    layer = rng.uniform(-0.5, 1.5, (67, 45)).astype(f32)
    layer.ravel()[:12] = [np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0, 0.25, 0.75, np.nextafter(f32(0.25), f32(0)), np.nextafter(f32(0.75), f32(1)), -7.0, 9.0]
    grid = upload(pkg, g, [np.zeros((67, 45), f32), layer])
    for lo, hi in ((0.0, 1.0), (0.25, 0.75), (0.25, 0.25), (1.0, 0.0), (-1.0, 100.0)):
        data, desc = grid.to_occupancy(1, lo, hi)
        want, width, height, res, origin = R.to_occupancy(g, layer, lo, hi)
        assert np.array_equal(data, want), (lo, hi, np.nonzero(data != want)[0][:5])
        assert (desc["width"], desc["height"]) == (width, height) == (67, 45) and desc["resolution"] == res and tuple(desc["origin"]) == origin
    assert set(np.unique(R.to_occupancy(g, layer, 0.25, 0.25)[0]).tolist()) == {-1, 0, 100}
    # GridMapRosTest.cpp:116-127 on the device
    ones = upload(pkg, gs.Geometry(16, 10, 0.5), [np.ones((16, 10), f32)])
    assert ones.to_occupancy(0, 0.0, 1.0)[0][0] == 100
    # cap_cells one short: LIO_ERR_ARG, data untouched
    lib = pkg.load_library()
    data = np.full(67 * 45, 77, np.int8)
    assert lib.lio_grid_to_occupancy(grid.h, 1, 0.0, 1.0, data.ctypes.data, data.size - 1, None) == -1 and "fewer" in lib.lio_last_error().decode()
    assert (data == 77).all()
    assert lib.lio_grid_to_occupancy(grid.h, 1, 0.0, 1.0, data.ctypes.data, data.size, None) == 0 and np.array_equal(data, R.to_occupancy(g, layer, 0.0, 1.0)[0])
