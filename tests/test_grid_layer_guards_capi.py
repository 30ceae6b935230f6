"""What the entries over a resident lio_grid refuse about the layers they are given, without a GPU: an id of -1 or 16, a repeated
id, a list of too few or too many, an id or a layer the object does not hold.  No object can be created without a device, so the
object here is a zeroed block that carries nothing but a device id and a layer mask (the first two words of lio_grid,
lio_gridobj.h): every call below is refused on what it reads there or before, and none reaches a device."""
import ctypes as C

import numpy as np

NAN = float("nan")


class _Object(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("mask", C.c_uint32), ("rest", C.c_uint8 * 4088)]


def _holding(mask):
    o = _Object()
    o.mask = mask
    return o


def _ids(*v):
    return (C.c_int32 * len(v))(*v)


def test_layer_lists_are_refused(pkg):
    lib = pkg.load_library()
    g, other = _holding(0b0011), _holding(0b0011)
    G, OTHER = C.addressof(g), C.addressof(other)
    many = _ids(*range(16), 0)
    out = np.zeros(64, np.float64)

    def last():
        return lib.lio_last_error().decode()

    # lio_grid_sample: the list is read after the object
    cfg = pkg.grid_sample_default_config()
    pos = np.zeros((3, 2), np.float64)
    for ids, n in ((_ids(-1), 1), (_ids(16), 1), (_ids(0, 0), 2), (_ids(1, 0, 1), 3), (_ids(0, 1), 0), (many, 17), (_ids(0, 2), 2), (_ids(5), 1)):
        for obj in (G, None):
            assert lib.lio_grid_sample(obj, ids, n, C.byref(cfg), pos.ctypes.data, 3, out.ctypes.data, None, None) == -1, (list(ids), n, obj)
    # lio_grid_region_reduce: the list before the object, the absent layer after it
    rcfg = pkg.grid_region_default_config()
    rec, verts = pkg.pack_regions([("circle", 0.0, 0.0, 1.0)])
    stats = np.zeros((2, 1), pkg.GRID_REGION_STAT_DTYPE)

    def reduce(obj, ids, n):
        return lib.lio_grid_region_reduce(obj, ids, n, C.byref(rcfg), rec.ctypes.data, 1, verts.ctypes.data, len(verts), stats.ctypes.data, None, None, None)

    for ids, n, why in ((_ids(-1), 1, "layer id"), (_ids(16), 1, "layer id"), (_ids(0, 0), 2, "repeated"), (_ids(0, 1), 0, "n_layers"), (many, 17, "n_layers")):
        for obj in (G, None):
            assert reduce(obj, ids, n) == -1 and why in last(), (list(ids), n, obj, last())
    assert reduce(G, _ids(0, 2), 2) == -1
    assert reduce(G, _ids(5), 1) == -1
    # lio_grid_add_data_from: an empty list is every layer of other; the list before the objects, the absent layer after them
    def add(a, b, ids, n):
        return lib.lio_grid_add_data_from(a, b, 1, 1, ids, n, 0, None)

    for ids, n, why in ((_ids(-1), 1, "outside"), (_ids(16), 1, "outside"), (_ids(0, 0), 2, "repeated"), (_ids(0, 1), -1, "n_layers"), (many, 17, "n_layers")):
        for a, b in ((G, OTHER), (None, None)):
            assert add(a, b, ids, n) == -1 and why in last(), (list(ids), n, a, last())
    assert add(G, OTHER, _ids(0, 2), 2) == -1 and "other does not hold" in last()
    assert add(G, OTHER, _ids(5), 1) == -1 and "other does not hold" in last()
    # lio_grid_to_point_cloud
    n_out, n_fields = C.c_size_t(99), C.c_int32(99)

    def cloud(obj, point_layer, ids, n):
        return lib.lio_grid_to_point_cloud(obj, point_layer, ids, n, 0, out.ctypes.data, 1, C.byref(n_out), C.byref(n_fields))

    for ids, n, why in ((_ids(-1), 1, "outside"), (_ids(16), 1, "outside"), (_ids(0, 0), 2, "repeated"), (_ids(0, 1), 0, "n_layers"), (many, 17, "n_layers")):
        for obj in (G, None):
            assert cloud(obj, 0, ids, n) == -1 and why in last(), (list(ids), n, obj, last())
    assert cloud(G, 0, _ids(0, 2), 2) == -1 and "does not hold" in last()
    assert cloud(G, 0, _ids(5), 1) == -1 and "does not hold" in last()
    for point_layer in (-1, 16, 2):
        assert cloud(G, point_layer, _ids(0, 1), 2) == -1 and "point_layer" in last(), point_layer
    assert n_out.value == 0 and n_fields.value == 0


def test_single_layers_are_refused(pkg):
    lib = pkg.load_library()
    g, dst = _holding(0b0011), _holding(0)
    G, DST = C.addressof(g), C.addressof(dst)
    out = np.zeros(64, np.float64)
    n_out = C.c_size_t(99)
    identity = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    for layer in (-1, 16, 2, 15):
        for rc in (lib.lio_grid_get_layer(G, layer, out.ctypes.data, 64),
                   lib.lio_grid_to_image(G, layer, 1, 0, 0.0, 1.0, out.ctypes.data, 64, None),
                   lib.lio_grid_to_image(G, layer, 1, 0, NAN, NAN, out.ctypes.data, 64, None),
                   lib.lio_grid_to_occupancy(G, layer, 0.0, 1.0, out.ctypes.data, 64, None),
                   lib.lio_grid_to_grid_cells(G, layer, 0.0, 1.0, out.ctypes.data, 1, C.byref(n_out))):
            assert rc == -1 and "no such layer" in lib.lio_last_error().decode(), (layer, rc, lib.lio_last_error())
        assert lib.lio_grid_transform(G, identity, layer, 0.0, DST, None) == -1 and "height_layer" in lib.lio_last_error().decode(), layer
    assert n_out.value == 0 and dst.mask == 0 and g.mask == 0b0011
