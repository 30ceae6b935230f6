"""lio_grid_to_image, lio_grid_add_layer_from_image, lio_grid_add_color_layer_from_image, lio_grid_from_occupancy,
lio_grid_to_point_cloud, lio_grid_to_grid_cells and lio_sdf_to_point_cloud on the device through the C ABI: every byte, word,
count and info field against the restatement (tests/grid_convert_restate.py), which tests/test_grid_convert_cpu.py holds against
the reference's own tests and against the header the kernels run.  The tolerance is 0: the same fp32 operations run in the same
order without contraction.  The shapes are tests/grid_convert_cases.py's: one short of, exactly and one past a 64 x 64 tile in
each direction (the tiled image kernels' edges; a workgroup of 256 cells ends inside every one of them too), a single cell,
row and column."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_restate as gs                               # noqa: E402
import grid_convert_restate as R                               # noqa: E402
import grid_convert_cases as K                                 # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
NAN = math.nan
SHAPE_IDS = [f"{s[0]}x{s[1]}" for s in K.SHAPES]
INFO_KEYS = ("rows", "cols", "lower", "upper", "n_pixels", "n_clamped_low", "n_clamped_high", "n_nonfinite")


def upload(pkg, g, layers):
    grid = pkg.Grid()
    grid.set_layers(np.asarray(layers, f32), g.res, g.length, g.pos)
    return grid


def words(grid, k):
    return np.ascontiguousarray(grid.layer(k)).view(u32)


def refused(pkg, code, why, call):
    with pytest.raises(pkg.LioError) as e:
        call()
    assert {-1: "ERR_ARG", -3: "ERR_CAPACITY"}[code] in str(e.value) and why in str(e.value), str(e.value)


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_to_image(pkg, shape):
    """all nine channel / depth pairs, given and automatic bounds: the image's bytes and the info record; the layer is only read"""
    rows, cols = shape
    g = gs.Geometry(rows, cols, 0.25, (1.5, -2.25))
    for depth in (R.IMAGE_8U, R.IMAGE_16U, R.IMAGE_32F):
        layer = K.image_layer(rows, cols, depth)
        grid = upload(pkg, g, [layer, np.full(shape, NAN, f32)])
        for channels in (1, 3, 4):
            for lo, hi in ((K.LOWER, K.UPPER), (NAN, NAN)):
                try:
                    want, winfo = R.to_image(layer, channels, depth, lo, hi)
                except R.Refused:
                    assert rows * cols == 1 and math.isnan(lo)
                    refused(pkg, -1, "extremes are equal", lambda: grid.to_image(0, channels, depth, lo, hi))
                    continue
                img, info = grid.to_image(0, channels, depth, lo, hi)
                assert img.dtype == want.dtype and img.shape == want.shape
                assert img.tobytes() == want.tobytes(), (channels, depth, lo, np.argwhere(img != want)[:5])
                assert [info[k].item() for k in INFO_KEYS] == [winfo[k] for k in INFO_KEYS], (channels, depth, lo)
        assert np.array_equal(words(grid, 0), layer.view(u32))
        refused(pkg, -1, "no finite cell", lambda: grid.to_image(1, 1, depth))             # the all-NaN layer
        grid.close()


def test_to_image_refusals_that_need_an_object(pkg):
    g = gs.Geometry(3, 2, 0.5)
    grid = upload(pkg, g, [np.arange(6, dtype=f32).reshape(3, 2), np.full((3, 2), 4.0, f32), np.array([[-3e38, 3e38], [0, 0], [0, 0]], f32)])
    refused(pkg, -1, "no such layer", lambda: grid.to_image(3, 1, 0, 0.0, 1.0))
    refused(pkg, -1, "no such layer", lambda: grid.to_image(-1, 1, 0, 0.0, 1.0))
    refused(pkg, -1, "extremes are equal", lambda: grid.to_image(1, 1, 0))
    refused(pkg, -1, "must be finite", lambda: grid.to_image(2, 1, 0))
    img = np.full(5, 7, np.uint8)                              # one byte short: untouched
    assert pkg.load_library().lio_grid_to_image(grid.h, 0, 1, 0, 0.0, 1.0, img.ctypes.data, img.nbytes, None) == -1 and (img == 7).all()
    empty = pkg.Grid()
    assert pkg.load_library().lio_grid_to_image(empty.h, 0, 1, 0, 0.0, 1.0, img.ctypes.data, 5, None) == -1
    assert b"no such layer" in pkg.load_library().lio_last_error()
    empty.close()
    grid.close()


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_layers_from_images(pkg, shape):
    """the accepted formats in, grey and colour, onto an empty grid (its geometry from the call) and beside other layers"""
    rows, cols = shape
    for channels, depth in K.FORMATS_IN:
        for color in ((False, True) if depth == R.IMAGE_8U and channels > 1 else (False,)):
            img = K.ingest_image(rows, cols, channels, depth, color=color)
            if color:
                want, transparent = R.add_color_layer_from_image(img), 0
            else:
                layer, transparent = R.add_layer_from_image(img, -0.5, 2.0, 0.5)
                want = layer.view(u32)
            grid = pkg.Grid()                                  # initializeFromImage
            info = grid.add_color_layer_from_image(5, img, 0.1, (3.0, -1.0)) if color else grid.add_layer_from_image(5, img, -0.5, 2.0, 0.5, 0.1, (3.0, -1.0))
            d, wg = grid.info(), R.geometry_from_image(rows, cols, 0.1, (3.0, -1.0))
            assert d.layer_mask == 1 << 5 and (d.rows, d.cols) == wg.size and tuple(d.length) == wg.length and tuple(d.position) == wg.pos
            assert np.array_equal(words(grid, 5), want), (channels, depth, color, np.argwhere(words(grid, 5) != want)[:5])
            assert (info["rows"], info["cols"], info["geometry_set"], info["n_cells_transparent"], info["n_cells_set"]) == (rows, cols, 1, transparent,
                                                                                                                           rows * cols - transparent)
            grid.close()
    # beside other layers: they stay, the layer is replaced when present, the size must match
    g = gs.Geometry(rows, cols, 0.25, (1.5, -2.25))
    others = K.cloud_layers(rows, cols)
    grid = upload(pkg, g, [others[0], others[1]])
    img = K.ingest_image(rows, cols, 4, R.IMAGE_16U)
    for layer_id in (1, 7):
        info = grid.add_layer_from_image(layer_id, img, 0.0, 1.0, 0.5)
        assert info["geometry_set"] == 0 and np.array_equal(words(grid, layer_id), R.add_layer_from_image(img, 0.0, 1.0, 0.5)[0].view(u32))
    d = grid.info()
    assert d.layer_mask == 0b10000011 and tuple(d.position) == g.pos and np.array_equal(words(grid, 0), others[0].view(u32))
    refused(pkg, -1, "size", lambda: grid.add_layer_from_image(2, np.zeros((rows + 1, cols), np.uint8)))
    refused(pkg, -1, "size", lambda: grid.add_color_layer_from_image(2, np.zeros((rows, cols + 1, 3), np.uint8)))
    assert grid.info().layer_mask == 0b10000011
    grid.close()
    empty = pkg.Grid()
    refused(pkg, -1, "resolution", lambda: empty.add_layer_from_image(0, np.zeros((rows, cols), np.uint8), resolution=0.0))
    assert empty.info().layer_mask == 0
    empty.close()


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_image_round_trip_on_the_device(pkg, shape):
    """an 8UC4 image straight from lio_grid_to_image fed back in, as GridMapCvTest's roundTrip8UC4 does: NaN cells come back NaN,
    the rest within the reference's tolerance (max - min) / 255 of the clamped layer; size and length preserved"""
    rows, cols = shape
    g = gs.Geometry(rows, cols, 0.1, (0.5, -0.2))
    layer = K.image_layer(rows, cols, R.IMAGE_8U)
    grid = upload(pkg, g, [layer])
    img, _ = grid.to_image(0, 4, R.IMAGE_8U, K.LOWER, K.UPPER)
    back = pkg.Grid()
    back.add_layer_from_image(0, img, K.LOWER, K.UPPER, 0.5, g.res, g.pos)
    got = back.layer(0)
    want = np.clip(layer, K.LOWER, K.UPPER)                   # (a NaN stays NaN)
    assert np.array_equal(np.isnan(got), np.isnan(layer))
    ok = ~np.isnan(layer)
    assert float(np.abs(got[ok] - want[ok]).max(initial=0.0)) <= (K.UPPER - K.LOWER) / f32(255.0)
    d = back.info()
    assert (d.rows, d.cols) == g.size and tuple(d.length) == g.length
    assert np.array_equal(words(back, 0), R.add_layer_from_image(R.to_image(layer, 4, R.IMAGE_8U, K.LOWER, K.UPPER)[0], K.LOWER, K.UPPER)[0].view(u32))
    grid.close()
    back.close()


def test_occupancy_ingest(pkg):
    """5 x 3 with -1, 0, 100 and 37: onto an empty grid, a matching grid (other layers kept) and a differing one (other layers NaN
    at the new size); then lio_grid_to_occupancy(0, 100) returns the message"""
    data = np.array([-1, 0, 100, 37, 100, 0, -1, 37, 37, -1, 0, 0, 100, 100, -1], np.int8)
    want, wg = R.from_occupancy(data, 5, 3, 0.5, (1.0, -2.0))

    def check(grid, info, replaced, layer_id=0):
        d = grid.info()
        assert (d.rows, d.cols) == (5, 3) and d.resolution == wg.res and tuple(d.length) == wg.length and tuple(d.position) == wg.pos
        assert np.array_equal(words(grid, layer_id), want.view(u32))
        assert (info["rows"], info["cols"], info["geometry_replaced"], info["n_unknown"]) == (5, 3, replaced, 4)
        assert tuple(info["length"]) == wg.length and tuple(info["position"]) == wg.pos
        back, desc = grid.to_occupancy(layer_id, 0.0, 100.0)
        assert np.array_equal(back, data) and (desc["width"], desc["height"], desc["resolution"]) == (5, 3, f32(0.5))
        assert tuple(desc["origin"]) == (1.0, -2.0)

    grid = pkg.Grid()
    check(grid, grid.from_occupancy(0, data, 5, 3, 0.5, (1.0, -2.0)), 1)
    assert grid.info().layer_mask == 1
    # a matching grid: the other layers are kept, the layer itself is replaced
    other = np.arange(15, dtype=f32).reshape(5, 3)
    grid.add_layer_from_image(3, other)                        # (a 32FC1 image: lower 0, upper 1 leave the values)
    info = grid.from_occupancy(2, data, 5, 3, 0.5, (1.0, -2.0))
    check(grid, info, 0, 2)
    assert grid.info().layer_mask == 0b1101 and np.array_equal(words(grid, 3), other.view(u32)) and np.array_equal(words(grid, 0), want.view(u32))
    grid.close()
    # a differing grid (size, then position alone): every other layer reads NaN at the new size
    for g in (gs.Geometry(7, 4, 0.5, (0.0, 0.0)), gs.Geometry(5, 3, 0.5, (0.0, 0.0))):
        grid = upload(pkg, g, [np.ones(g.size, f32), np.zeros(g.size, f32), np.ones(g.size, f32)])
        check(grid, grid.from_occupancy(1, data, 5, 3, 0.5, (1.0, -2.0)), 1, 1)
        assert grid.info().layer_mask == 0b111
        for k in (0, 2):
            assert (words(grid, k) == R.QNAN_BITS).all() and grid.layer(k).shape == (5, 3)
        grid.close()
    grid = upload(pkg, gs.Geometry(5, 3, 0.5), [np.ones((5, 3), f32)])
    refused(pkg, -1, "width * height", lambda: grid.from_occupancy(0, data[:14], 5, 3, 0.5, (1.0, -2.0)))
    assert grid.info().layer_mask == 1 and (grid.layer(0) == 1.0).all()
    grid.close()


def cloud_of(grid, point, ids, basic, cap=None):
    return np.ascontiguousarray(grid.to_point_cloud(point, ids, basic, cap)).view(u32)


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_point_cloud_and_grid_cells(pkg, shape):
    """field order, a point layer absent from the list, a colour layer's bits, basic_mask of 0, one and two layers; the grid is
    only read"""
    rows, cols = shape
    g = gs.Geometry(rows, cols, 0.25, (1.5, -2.25))
    layers = K.cloud_layers(rows, cols)
    grid = upload(pkg, g, [layers[k] for k in range(4)])
    for point, ids, basic in ((0, [0, 1, 2], ()), (0, [2, 1], (1,)), (3, [1, 3, 0], (0, 1)), (1, [0], ()), (0, None, ())):
        want = R.to_point_cloud(g, layers, point, ids or [0, 1, 2, 3], basic)
        got = cloud_of(grid, point, ids, basic)
        assert got.shape == want.shape and np.array_equal(got, want), (point, ids, basic)
    for lo, hi in ((-0.5, 0.5), (-math.inf, math.inf), (2.0, 3.0)):
        want = R.to_grid_cells(g, layers[0], lo, hi)
        got = grid.to_grid_cells(0, lo, hi)
        assert got.shape == want.shape and np.array_equal(got, want), (lo, hi)
    for k in range(4):
        assert np.array_equal(words(grid, k), layers[k].view(u32))
    grid.close()


@pytest.mark.parametrize("which", [0, 1, "one", 256, 257, "all", "last workgroup"], ids=str)
def test_compaction_corners(pkg, which):
    """0, 1 and all survivors, exactly 256 and 257, survivors only in the last workgroup; capacity one short: LIO_ERR_CAPACITY,
    the count reported, the buffer untouched"""
    rows, cols = 67, 45
    g = gs.Geometry(rows, cols, 0.25, (1.5, -2.25))
    height = K.survivors_layer(rows, cols, which)
    other = K.cloud_layers(rows, cols)[1]
    grid = upload(pkg, g, [height, other])
    layers = {0: height, 1: other}
    want = R.to_point_cloud(g, layers, 0, [1, 0])
    n_want = {"all": rows * cols, "one": 1, "last workgroup": None}.get(which, which)
    assert n_want is None or len(want) == n_want
    got = cloud_of(grid, 0, [1, 0], ())
    assert got.shape == want.shape and np.array_equal(got, want)
    cells = grid.to_grid_cells(0, -math.inf, math.inf)
    assert np.array_equal(cells, R.to_grid_cells(g, height, -math.inf, math.inf)) and len(cells) == len(want)
    assert np.array_equal(cloud_of(grid, 0, [1, 0], (), cap=len(want)), want)              # a capacity that just fits
    if len(want):
        lib = pkg.load_library()
        n, nf = C.c_size_t(), C.c_int32()
        ids = (C.c_int32 * 2)(1, 0)
        buf = np.full((len(want) - 1) * 4 + 1, 7.0, f32)
        rc = lib.lio_grid_to_point_cloud(grid.h, 0, ids, 2, 0, buf.ctypes.data, len(want) - 1, C.byref(n), C.byref(nf))
        assert rc == -3 and n.value == len(want) and nf.value == 4 and (buf == 7.0).all()
        buf = np.full((len(want) - 1) * 2 + 1, 7.0, np.float64)
        rc = lib.lio_grid_to_grid_cells(grid.h, 0, -math.inf, math.inf, buf.ctypes.data, len(want) - 1, C.byref(n))
        assert rc == -3 and n.value == len(want) and (buf == 7.0).all()
    grid.close()


def test_compaction_refusals_that_need_an_object(pkg):
    g = gs.Geometry(3, 2, 0.5)
    grid = upload(pkg, g, [np.zeros((3, 2), f32), np.ones((3, 2), f32)])
    refused(pkg, -1, "does not hold", lambda: grid.to_point_cloud(0, [0, 5]))
    refused(pkg, -1, "point_layer", lambda: grid.to_point_cloud(4, [0, 1]))
    refused(pkg, -1, "basic_mask", lambda: grid.to_point_cloud(0, [0, 1], basic_layers=(2,)))
    refused(pkg, -1, "no such layer", lambda: grid.to_grid_cells(2, 0.0, 1.0))
    empty = pkg.Grid()
    refused(pkg, -1, "holds no layers", lambda: empty.to_point_cloud(0, [0]))
    refused(pkg, -1, "no such layer", lambda: empty.to_grid_cells(0, 0.0, 1.0))
    sdf = pkg.Sdf()
    refused(pkg, -1, "no field", lambda: sdf.to_point_cloud())
    sdf.close()
    empty.close()
    grid.close()


@pytest.fixture(scope="module")
def field(pkg):
    """a 9 x 7 grid whose band of 1.0 at 0.25 gives 4 layers; the nodes once"""
    rng = np.random.default_rng(97)
    g = gs.Geometry(9, 7, 0.25, (0.625, -1.1))
    elevation = rng.uniform(0.05, 0.95, g.size).astype(f32)
    sdf = pkg.Sdf()
    info = sdf.build(elevation, g.res, g.length, g.pos, pkg.sdf_default_config(min_height=0.0, max_height=1.0))
    assert 3 <= info.layers <= 5
    nodes = sdf.nodes()
    nodes.setflags(write=False)
    yield sdf, info, nodes
    sdf.close()


@pytest.mark.parametrize("decimation", [1, 2, 3, 10])
def test_field_cloud(pkg, field, decimation):
    """decimation 1, 2, 3 and one larger than every dimension; each bound alone, both, and neither; the field is only read"""
    sdf, info, nodes = field
    origin = tuple(info.origin)
    d = nodes[..., 0]
    lo, hi = float(np.quantile(d, 0.3)), float(np.quantile(d, 0.7))
    for lower, upper in ((NAN, NAN), (lo, NAN), (NAN, hi), (lo, hi), (float(d.max()) + 1.0, NAN)):
        want = R.sdf_to_point_cloud(nodes, origin, info.resolution, decimation, lower, upper)
        got = sdf.to_point_cloud(decimation, lower, upper)
        assert got.shape == want.shape and np.array_equal(got.view(u32), want.view(u32)), (decimation, lower, upper)
    full = R.sdf_to_point_cloud(nodes, origin, info.resolution, decimation)
    assert len(full) == math.ceil(info.layers / decimation) * math.ceil(7 / decimation) * math.ceil(9 / decimation)
    if len(full) > 1:
        n = C.c_size_t()
        buf = np.full((len(full) - 1) * 4 + 1, 7.0, f32)
        rc = pkg.load_library().lio_sdf_to_point_cloud(sdf.h, decimation, NAN, NAN, buf.ctypes.data, len(full) - 1, C.byref(n))
        assert rc == -3 and n.value == len(full) and (buf == 7.0).all()
    assert np.array_equal(sdf.nodes(), nodes)


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_tiled_image_kernels_give_the_same_bytes(pkg, shape):
    """the LDS-tiled form that tools/grid_convert_cost.py times beside the direct one the entries run: every format out and
    in on every shape around its 64 x 64 tile, the same bytes, words and counts"""
    lib = pkg.load_library()
    rows, cols = shape
    g = gs.Geometry(rows, cols, 0.25)
    try:
        assert lib.lio_grid_convert_debug_stage_ms(0, 1, None) == 0
        for channels, depth in K.FORMATS_OUT:
            layer = K.image_layer(rows, cols, depth)
            grid = upload(pkg, g, [layer])
            want, winfo = R.to_image(layer, channels, depth, K.LOWER, K.UPPER)
            img, info = grid.to_image(0, channels, depth, K.LOWER, K.UPPER)
            assert img.tobytes() == want.tobytes(), (channels, depth)
            assert [info[k].item() for k in INFO_KEYS] == [winfo[k] for k in INFO_KEYS], (channels, depth)
            if (channels, depth) in K.FORMATS_IN:
                src = K.ingest_image(rows, cols, channels, depth)
                back = grid.add_layer_from_image(1, src, -0.5, 2.0)
                wl, transparent = R.add_layer_from_image(src, -0.5, 2.0)
                assert np.array_equal(words(grid, 1), wl.view(u32)) and back["n_cells_transparent"] == transparent, (channels, depth)
            grid.close()
    finally:
        lib.lio_grid_convert_debug_stage_ms(0, 0, None)
