"""grid_map_cv's GridMapCvConverter (CV = GridMapCvConverter.hpp: toImage :173-247, addLayerFromImage :58-119,
addColorLayerFromImage :128-159, initializeFromImage :36-44) and GridMapRosConverter's toPointCloud (RC =
GridMapRosConverter.cpp :124-223, :225-281 over SignedDistanceField::filterPoints), toGridCells (:367-388) and
fromOccupancyGrid (:283-327), restated in numpy: one function per entry of the library (lio_grid_to_image, ...), fp32 where the
reference is fp32, each operation rounded once, in the order the source writes it.  Layers are [rows, cols] float32; an image is
[rows, cols, channels]; GridMapIterator's order is column-major (ravel(order="F"))."""
import math

import numpy as np

import grid_sample_restate as gs

f32, u32 = np.float32, np.uint32
IMAGE_8U, IMAGE_16U, IMAGE_32F = 0, 1, 2
DTYPES = {IMAGE_8U: np.uint8, IMAGE_16U: np.uint16, IMAGE_32F: np.float32}
QNAN_BITS = 0x7fc00000
GREY_WEIGHTS, GREY_SHIFT = (1868, 9617, 4899), 14             # cvtColor's BGR2GRAY as published for 8U and 16U (unpinned)


class Refused(ValueError):
    """what the library answers with LIO_ERR_ARG"""


def image_max(depth):
    return {IMAGE_8U: f32(255.0), IMAGE_16U: f32(65535.0), IMAGE_32F: f32(1.0)}[depth]


def finite_extremes(layer):
    """minCoeffOfFinites / maxCoeffOfFinites; None without a finite cell"""
    v = np.asarray(layer, f32)
    v = v[np.isfinite(v)]
    return (f32(v.min()), f32(v.max())) if v.size else None


def to_image(layer, channels, depth, lower=math.nan, upper=math.nan):
    """-> (image [rows, cols, channels], info dict)"""
    if channels not in (1, 3, 4) or depth not in DTYPES:
        raise Refused("format")
    x = np.asarray(layer, f32)
    lo, hi = f32(lower), f32(upper)
    if np.isnan(lo) and np.isnan(hi):
        ext = finite_extremes(x)
        if ext is None:
            raise Refused("no finite cell")
        lo, hi = ext
    elif np.isnan(lo) or np.isnan(hi):
        raise Refused("one bound")
    with np.errstate(all="ignore"):
        if not hi > lo or not np.isfinite(f32(hi - lo)):
            raise Refused("bounds")
        v = np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(f32)              # Clamp: a NaN stays NaN
        ok = np.isfinite(v)
        scaled = (((v - lo).astype(f32) / f32(hi - lo)).astype(f32) * image_max(depth)).astype(f32)
    dt = DTYPES[depth]
    value = np.zeros(x.shape, dt)
    value[ok] = scaled[ok] if depth == IMAGE_32F else np.trunc(scaled[ok]).astype(dt)
    img = np.zeros(x.shape + (channels,), dt)
    for ch in range(min(channels, 3)):
        img[:, :, ch] = value
    if channels == 4:
        img[:, :, 3] = np.where(ok, dt(image_max(depth)), dt(0))
    info = dict(rows=x.shape[0], cols=x.shape[1], lower=lo, upper=hi, n_pixels=int(ok.sum()), n_clamped_low=int((ok & (x < lo)).sum()),
                n_clamped_high=int((ok & (x > hi)).sum()), n_nonfinite=int((~ok).sum()))
    return img, info


def grey(image):
    """cvtColor(BGR2GRAY / BGRA2GRAY) for 8U and 16U: the integer weighted sum, rounded to nearest"""
    c = image.astype(np.uint64)
    return ((c[:, :, 0] * GREY_WEIGHTS[0] + c[:, :, 1] * GREY_WEIGHTS[1] + c[:, :, 2] * GREY_WEIGHTS[2] + (1 << (GREY_SHIFT - 1))) >> GREY_SHIFT).astype(image.dtype)


def _image(image):
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[:, :, None]
    depth = {np.dtype(np.uint8): IMAGE_8U, np.dtype(np.uint16): IMAGE_16U, np.dtype(np.float32): IMAGE_32F}[a.dtype]
    return a, a.shape[2], depth


def add_layer_from_image(image, lower=0.0, upper=1.0, alpha_threshold=0.5):
    """-> (layer [rows, cols] float32, cells below the alpha threshold)"""
    a, channels, depth = _image(image)
    if channels not in (1, 3, 4) or (depth == IMAGE_32F and channels != 1) or not 0.0 <= alpha_threshold <= 1.0:
        raise Refused("format")
    mx = image_max(depth)
    mono = a[:, :, 0] if channels == 1 else grey(a)
    lo, hi = f32(lower), f32(upper)
    with np.errstate(all="ignore"):
        out = (lo + (f32(hi - lo) * (mono.astype(f32) / mx).astype(f32)).astype(f32)).astype(f32)
    transparent = np.zeros(mono.shape, bool)
    if channels == 4:
        transparent = a[:, :, 3] < a.dtype.type(int(alpha_threshold * float(mx)))  # (Type)(alphaThreshold * maxImageValue)
        out.view(u32)[transparent] = QNAN_BITS
    return out, int(transparent.sum())


def add_color_layer_from_image(image):
    """-> the layer's words [rows, cols] uint32"""
    a, channels, depth = _image(image)
    if channels not in (3, 4) or depth != IMAGE_8U:
        raise Refused("format")
    c = a.astype(u32)
    if channels == 4:                                          # cvtColor(BGRA2RGB); without alpha imageRGB = image
        return (c[:, :, 2] << 16) + (c[:, :, 1] << 8) + c[:, :, 0]
    return (c[:, :, 0] << 16) + (c[:, :, 1] << 8) + c[:, :, 2]


def geometry_from_image(rows, cols, resolution, position):
    """initializeFromImage: length = resolution * (rows, cols)"""
    g = gs.Geometry(rows, cols, resolution, position)
    g.length = (resolution * rows, resolution * cols)
    return g


def from_occupancy(data, width, height, resolution, origin):
    """-> (layer [width, height] float32, geometry)"""
    d = np.asarray(data, np.int8)
    if width < 1 or height < 1 or width >= 1 << 24 or height >= 1 << 24 or width * height != d.size or not float(f32(resolution)) >= 1e-4:
        raise Refused("message")
    rev = d[::-1]
    layer = rev.astype(f32)
    layer.view(u32)[rev == -1] = QNAN_BITS
    res = float(f32(resolution))                               # the message's float32 field widened
    g = gs.Geometry(width, height, res)
    g.length = (res * float(width), res * float(height))
    g.pos = (origin[0] + 0.5 * g.length[0], origin[1] + 0.5 * g.length[1])
    return layer.reshape((width, height), order="F"), g


def same_geometry(a, b):
    return a is not None and a.size == b.size and a.res == b.res and a.length == b.length and a.pos == b.pos


def centres(g):
    """getPositionFromIndex of every cell in the iterator's order -> (x [n], y [n]) float64"""
    rows, cols = g.size
    x = np.array([gs.position_from_index(g, (r, 0))[0] for r in range(rows)])
    y = np.array([gs.position_from_index(g, (0, c))[1] for c in range(cols)])
    return np.tile(x, cols), np.repeat(y, rows)


def to_point_cloud(g, layers, point_layer, layer_ids, basic_layers=()):
    """layers: {id: [rows, cols] float32} -> the records' words [n, F] uint32"""
    if len(set(layer_ids)) != len(layer_ids) or not layer_ids or any(k not in layers for k in list(layer_ids) + list(basic_layers) + [point_layer]):
        raise Refused("layers")
    flat = {k: np.asarray(v, f32).ravel(order="F") for k, v in layers.items()}
    keep = np.isfinite(flat[point_layer])
    for k in basic_layers:
        keep &= np.isfinite(flat[k])
    x, y = centres(g)
    cols = []
    for k in layer_ids:
        if k == point_layer:
            cols += [x.astype(f32).view(u32), y.astype(f32).view(u32), flat[k].view(u32)]
        else:
            cols.append(flat[k].view(u32))
    return np.stack(cols, axis=1)[keep]


def to_grid_cells(g, layer, lower, upper):
    """-> [n, 2] float64"""
    v = np.asarray(layer, f32).ravel(order="F")
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(v) & (v >= f32(lower)) & (v <= f32(upper))
    x, y = centres(g)
    return np.stack([x, y], axis=1)[keep]


def sdf_to_point_cloud(nodes, origin, resolution, decimation=1, lower=math.nan, upper=math.nan):
    """nodes: [layers, cols, rows, 4] float32 (data_'s order) -> [n, 4] float32; the loops of filterPoints as written"""
    if decimation < 1:
        raise Refused("decimation")
    layers, cols, rows = nodes.shape[:3]
    lo, hi = f32(lower), f32(upper)
    out = []
    for z in range(0, layers, decimation):
        for y in range(0, cols, decimation):
            for x in range(0, rows, decimation):
                d = nodes[z, y, x, 0]
                if (np.isnan(lo) or d >= lo) and (np.isnan(hi) or d <= hi):
                    out.append((f32(origin[0] - x * resolution), f32(origin[1] - y * resolution), f32(origin[2] + z * resolution), d))
    return np.array(out, f32).reshape(-1, 4)
