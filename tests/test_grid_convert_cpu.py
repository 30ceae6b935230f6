"""The restatement of the grid converters (tests/grid_convert_restate.py) without a GPU: against the reference's own tests
(grid_map_cv/test/GridMapCvTest.cpp:37-143, grid_map_ros/test/GridMapRosTest.cpp:140-238) with their tolerances, then the header
the kernels run (lio-slam_amd/csrc/lio_gridconvert.h, through tools/grid_convert_host_check.cpp, which replays the kernels'
tile walk) against the restatement, word for word, on the cases of tests/test_gpu_grid_convert.py."""
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_convert_cases as K                                 # noqa: E402
import grid_convert_restate as R                               # noqa: E402
import grid_sample_restate as gs                               # noqa: E402
import grid_transform_restate as T                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


# ---- the reference's own tests
@pytest.mark.parametrize("channels,depth", [(3, R.IMAGE_8U), (4, R.IMAGE_8U), (1, R.IMAGE_16U), (1, R.IMAGE_32F)],
                         ids=["roundTrip8UC3", "roundTrip8UC4", "roundTrip16UC1", "roundTrip32FC1"])
def test_reference_image_round_trips(channels, depth):
    """GridMapCvTest.cpp:37-143: 2.0 x 1.0 at 0.1 (20 x 10), random values in [-1, 1], bounds -1 and 1; back within
    (max - min) / 255; length and size preserved"""
    g = gs.Geometry(20, 10, 0.1, (0.5, -0.2))
    layer = np.random.default_rng(37 + channels + depth).uniform(-1, 1, g.size).astype(f32)
    image, info = R.to_image(layer, channels, depth, -1.0, 1.0)
    assert image.shape == (20, 10, channels) and image.dtype == R.DTYPES[depth] and info["n_pixels"] == 200
    back, transparent = R.add_layer_from_image(image, -1.0, 1.0)
    tolerance = (f32(1.0) - f32(-1.0)) / f32(255.0)
    assert transparent == 0 and back.shape == layer.shape and float(np.abs(back - layer).max()) <= tolerance
    out = R.geometry_from_image(image.shape[0], image.shape[1], g.res, g.pos)
    assert out.size == g.size and out.length == g.length


@pytest.mark.parametrize("channels,depth,tolerance", [(4, R.IMAGE_8U, 2.0 / 255.0), (1, R.IMAGE_16U, 300.0 * 2.0 / 65535.0)],
                         ids=["roundTripBGRA8", "roundTripMONO16"])
def test_reference_image_message_round_trips(channels, depth, tolerance):
    """GridMapRosTest.cpp:186-238: 2.0 x 1.0 at 0.01 (200 x 100) through an image and initializeFromImage + addLayerFromImage"""
    g = gs.Geometry(200, 100, 0.01)
    layer = np.random.default_rng(186 + depth).uniform(-1, 1, g.size).astype(f32)
    image, _ = R.to_image(layer, channels, depth, -1.0, 1.0)
    back, transparent = R.add_layer_from_image(image, -1.0, 1.0)
    assert transparent == 0 and float(np.abs(back - layer).max()) <= f32(tolerance)
    out = R.geometry_from_image(image.shape[0], image.shape[1], g.res, (0.0, 0.0))
    assert out.size == g.size and out.length == g.length


def test_reference_occupancy_round_trip():
    """GridMapRosTest.cpp:140-184: 50 x 100 at 0.1 from (3, 6), every cell in [-1, 100], back through toOccupancyGrid(-1, 100)"""
    rng = np.random.default_rng(140)
    data = rng.integers(-1, 101, 50 * 100).astype(np.int8)
    data[:102] = np.arange(-1, 101)
    layer, g = R.from_occupancy(data, 50, 100, 0.1, (3.0, 6.0))
    assert layer.shape == (50, 100) and np.isnan(layer).sum() == (data == -1).sum()
    assert np.array_equal(layer.view(u32), T.from_occupancy(data, 50, 100).view(u32))
    back, width, height, res, origin = T.to_occupancy(g, layer, -1.0, 100.0)
    assert np.array_equal(back, data) and (width, height) == (50, 100) and res == f32(0.1)
    assert origin == pytest.approx((3.0, 6.0), abs=1e-12)      # EXPECT_DOUBLE_EQ


def test_conventions_by_hand():
    nan, inf = math.nan, math.inf
    layer = np.array([[-2.0, -1.0, 0.0], [1.0, 3.0, nan], [inf, -inf, 0.999]], f32)
    img, info = R.to_image(layer, 4, R.IMAGE_8U, -1.0, 1.0)
    assert img[:, :, 0].tolist() == [[0, 0, 127], [255, 255, 0], [255, 0, 254]]            # truncation; a NaN leaves zero
    assert img[:, :, 3].tolist() == [[255, 255, 255], [255, 255, 0], [255, 255, 255]]      # alpha included
    assert (info["n_pixels"], info["n_clamped_low"], info["n_clamped_high"], info["n_nonfinite"]) == (8, 2, 2, 1)
    auto = R.to_image(layer, 1, R.IMAGE_16U)[1]
    assert (auto["lower"], auto["upper"]) == (-2.0, 3.0)       # the finite extremes, +-inf present
    for bad in ((1.0, 1.0), (2.0, 1.0), (nan, 1.0), (-3e38, 3e38)):
        with pytest.raises(R.Refused):
            R.to_image(layer, 1, R.IMAGE_8U, *bad)
    for flat in (np.full((2, 2), nan, f32), np.full((2, 2), 4.0, f32)):
        with pytest.raises(R.Refused):
            R.to_image(flat, 1, R.IMAGE_8U)
    # alpha 126 / 127 / 128 around (unsigned char)(0.5 * 255) = 127
    px = np.array([[[10, 10, 10, 126], [10, 10, 10, 127], [10, 10, 10, 128]]], np.uint8)
    back, transparent = R.add_layer_from_image(px, 0.0, 1.0)
    assert transparent == 1 and np.isnan(back[0, 0]) and back[0, 1] == back[0, 2] == f32(10) / f32(255)
    assert R.grey(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [77, 77, 77]]], np.uint8)).tolist() == [[29, 150, 76, 77]]
    assert sum(R.GREY_WEIGHTS) == 1 << R.GREY_SHIFT
    # the colour quirk: with alpha the channels are swapped first, without they are not
    assert R.add_color_layer_from_image(np.array([[[1, 2, 3]]], np.uint8))[0, 0] == 0x010203
    assert R.add_color_layer_from_image(np.array([[[1, 2, 3, 9]]], np.uint8))[0, 0] == 0x030201
    for bad in (np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 3), f32)):
        with pytest.raises(R.Refused):
            R.add_layer_from_image(bad)
    # a cloud: x, y, z where the point layer is listed; field order is the list's; the iterator's order is column-major
    g = gs.Geometry(2, 2, 1.0)
    layers = {0: np.array([[1.0, nan], [3.0, 4.0]], f32), 1: np.array([[5.0, 6.0], [nan, 8.0]], f32)}
    assert R.to_point_cloud(g, layers, 0, [1, 0]).view(f32).tolist()[0] == [5.0, 0.5, 0.5, 1.0]
    assert R.to_point_cloud(g, layers, 0, [1, 0], basic_layers=[1]).view(f32)[:, 3].tolist() == [1.0, 4.0]
    assert R.to_point_cloud(g, layers, 0, [1]).shape == (3, 1)  # the point layer absent from the list still decides
    assert R.to_grid_cells(g, layers[0], 2.0, 4.0).tolist() == [[-0.5, 0.5], [-0.5, -0.5]]


# ---- the header on the host
@pytest.fixture(scope="module")
def host_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grid_convert_host_check")
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                               os.path.join(ROOT, "tools", "grid_convert_host_check.cpp"), "-o", exe])
        yield exe, d


def run(exe, *args):
    out = subprocess.run([exe] + [a if isinstance(a, str) else repr(float(a)) if isinstance(a, (float, np.floating)) else str(a) for a in args],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_host_check_counts_nothing(host_check):
    """its own run: the tiled walk against the plain loop, every byte and cell written once, the counters, the 8UC4 round trip"""
    exe, _ = host_check
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and out.stdout.rstrip().endswith("inconsistencies: 0")


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_to_image_equals_the_restatement(host_check, shape):
    exe, d = host_check
    rows, cols = shape
    for channels, depth in K.FORMATS_OUT:
        layer = K.image_layer(rows, cols, depth)
        layer.ravel(order="F").tofile(os.path.join(d, "layer"))
        for lo, hi in ((K.LOWER, K.UPPER), (math.nan, math.nan)):
            try:
                want, info = R.to_image(layer, channels, depth, lo, hi)
            except R.Refused:
                assert rows * cols == 1 and math.isnan(lo)     # one cell has no two extremes
                continue
            run(exe, "to_image", rows, cols, channels, depth, float(lo), float(hi), os.path.join(d, "layer"), os.path.join(d, "out"))
            raw = open(os.path.join(d, "out"), "rb").read()
            assert raw[:want.nbytes] == want.tobytes(), (channels, depth, lo)
            assert np.frombuffer(raw, f32, 2, want.nbytes).tolist() == [info["lower"], info["upper"]]
            assert np.frombuffer(raw, np.int64, 4, want.nbytes + 8).tolist() == [info[k] for k in ("n_pixels", "n_clamped_low", "n_clamped_high", "n_nonfinite")]


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_from_image_equals_the_restatement(host_check, shape):
    exe, d = host_check
    rows, cols = shape
    for channels, depth in K.FORMATS_IN:
        for color in ((False, True) if depth == R.IMAGE_8U and channels > 1 else (False,)):
            img = K.ingest_image(rows, cols, channels, depth, color=color)
            img.tofile(os.path.join(d, "image"))
            run(exe, "from_image", rows, cols, channels, depth, int(color), -0.5, 2.0, 0.5, os.path.join(d, "image"), os.path.join(d, "out"))
            raw = open(os.path.join(d, "out"), "rb").read()
            got = np.frombuffer(raw, u32, rows * cols).reshape((rows, cols), order="F")
            if color:
                want, transparent = R.add_color_layer_from_image(img), 0
            else:
                layer, transparent = R.add_layer_from_image(img, -0.5, 2.0, 0.5)
                want = layer.view(u32)
            assert np.array_equal(got, want), (channels, depth, color)
            assert np.frombuffer(raw, np.int64, 1, 4 * rows * cols)[0] == transparent


def test_header_occupancy_equals_the_restatement(host_check):
    exe, d = host_check
    data = np.array([-1, 0, 100, 37] * 4, np.int8)[:15]
    data.tofile(os.path.join(d, "data"))
    run(exe, "occupancy", 15, os.path.join(d, "data"), os.path.join(d, "out"))
    want = R.from_occupancy(data, 5, 3, 0.5, (0.0, 0.0))[0]
    assert np.array_equal(np.fromfile(os.path.join(d, "out"), u32), want.view(u32).ravel(order="F"))


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_compactions_equal_the_restatement(host_check, shape):
    exe, d = host_check
    rows, cols = shape
    g = gs.Geometry(rows, cols, 0.25, (1.5, -2.25))
    layers = K.cloud_layers(rows, cols)
    np.stack([layers[k].ravel(order="F") for k in range(4)]).tofile(os.path.join(d, "layers"))
    for point, ids, basic in ((0, [0, 1, 2], ()), (0, [2, 1], (1,)), (3, [1, 3, 0], (0, 1)), (1, [0], ())):
        want = R.to_point_cloud(g, layers, point, ids, basic)
        run(exe, "cloud", rows, cols, g.res, g.pos[0], g.pos[1], 4, point, ",".join(map(str, ids)), sum(1 << k for k in basic), os.path.join(d, "layers"),
            os.path.join(d, "out"))
        raw = open(os.path.join(d, "out"), "rb").read()
        assert np.frombuffer(raw, np.int64, 1)[0] == len(want)
        assert np.array_equal(np.frombuffer(raw, u32, want.size, 8).reshape(want.shape), want), (point, ids, basic)
    layers[0].ravel(order="F").tofile(os.path.join(d, "layer"))
    for lo, hi in ((-0.5, 0.5), (-math.inf, math.inf), (2.0, 3.0)):
        want = R.to_grid_cells(g, layers[0], lo, hi)
        run(exe, "cells", rows, cols, g.res, g.pos[0], g.pos[1], lo, hi, os.path.join(d, "layer"), os.path.join(d, "out"))
        raw = open(os.path.join(d, "out"), "rb").read()
        assert np.frombuffer(raw, np.int64, 1)[0] == len(want)
        assert np.array_equal(np.frombuffer(raw, np.float64, want.size, 8).reshape(want.shape), want)


def test_header_field_cloud_equals_the_restatement(host_check):
    exe, d = host_check
    rng = np.random.default_rng(9)
    rows, cols, layers = 9, 7, 4
    nodes = rng.uniform(-1, 1, (layers, cols, rows, 4)).astype(f32)
    nodes.tofile(os.path.join(d, "nodes"))
    origin, res = (1.0625, -2.3, 0.171), 0.3
    for decimation in (1, 2, 3, 10):
        for lo, hi in ((math.nan, math.nan), (-0.25, math.nan), (math.nan, 0.25), (-0.25, 0.25)):
            want = R.sdf_to_point_cloud(nodes, origin, res, decimation, lo, hi)
            run(exe, "sdf", rows, cols, layers, origin[0], origin[1], origin[2], res, decimation, lo, hi, os.path.join(d, "nodes"), os.path.join(d, "out"))
            raw = open(os.path.join(d, "out"), "rb").read()
            assert np.frombuffer(raw, np.int64, 1)[0] == len(want), (decimation, lo, hi)
            assert np.array_equal(np.frombuffer(raw, u32, want.size, 8), want.view(u32).ravel())
