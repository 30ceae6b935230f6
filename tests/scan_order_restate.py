"""The contract of the upload-time tile sort (lio_kernels.hip, "scan tile sort (upload)"; lio_plan_scan_tiles in
lio_gridplan.h), restated in plain numpy -- not a port of either form of the sort:

  * the scan's box is taken per axis over the coordinates with |v| <= 3.0e38 (an axis without one is [0, 0]);
  * tiles of the asked edge are laid over it, the edge doubled until the grid has at most 262144 tiles;
  * a point's tile coordinate is floor((v - origin) * inv_tile) in fp32, clamped into the grid (NaN -> 0);
  * tile ids are x-fastest, or shard-axis-slowest when the map is sharded;
  * the sorted order is tile id ascending, the caller's index ascending inside a tile.
"""
import numpy as np

BOX_LIMIT = np.float32(3.0e38)          # (below FLT_MAX = 3.4028235e38)
MAX_TILES = 262144.0
EMPTY_KEY = 0xffffffff                  # what the one-launch form marks an empty slot with


def box(xyz):
    """-> (lo[3], hi[3]) float32 over the coordinates with |v| <= 3.0e38, axis by axis."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        v = xyz[:, a]
        v = v[np.abs(v) <= BOX_LIMIT]                       # (NaN compares false)
        if len(v):
            lo[a], hi[a] = v.min(), v.max()
    return lo, hi


def plan_box(lo, hi, tile0, shard_axis=-1):
    """The grid over the box [lo, hi]: dict(n = tiles per axis, k = key strides per axis, o = origin, inv = 1 / edge (fp32),
    tile = the edge used, doublings)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    tile = np.float32(tile0)
    doublings = 0
    with np.errstate(over="ignore"):
        while True:
            inv = np.float32(1.0) / tile                    # IEEE fp32 quotient
            e = [float(np.floor((np.float64(hi[a]) - np.float64(lo[a])) * np.float64(inv))) + 1.0 for a in range(3)]
            if e[0] * e[1] * e[2] <= MAX_TILES:
                break
            tile = np.float32(tile * np.float32(2.0))
            doublings += 1
    n = [int(v) for v in e]
    if shard_axis == 0:
        k = [n[2] * n[1], n[2], 1]
    elif shard_axis == 1:
        k = [1, n[0] * n[2], n[0]]
    else:
        k = [1, n[0], n[0] * n[1]]
    return dict(n=n, k=k, o=lo.copy(), inv=inv, tile=tile, doublings=doublings)


def plan(xyz, tile0=4.0, shard_axis=-1):
    lo, hi = box(xyz)
    return plan_box(lo, hi, tile0, shard_axis)


def tile_coords(xyz, p):
    """[n, 3] int64 tile coordinates, fp32 arithmetic."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros(xyz.shape, np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            c = np.floor((xyz[:, a] - np.float32(p["o"][a])) * np.float32(p["inv"]))
            assert c.dtype == np.float32
            c = np.where(np.isnan(c), np.float32(0.0), c)                   # fmaxf(NaN, 0) = 0
            c = np.minimum(np.maximum(c, np.float32(0.0)), np.float32(p["n"][a] - 1))
            out[:, a] = c.astype(np.int64)
    return out


def tile_ids(xyz, p):
    c = tile_coords(xyz, p)
    return c[:, 0] * p["k"][0] + c[:, 1] * p["k"][1] + c[:, 2] * p["k"][2]


def order(xyz, tile0=4.0, shard_axis=-1):
    """order[j] = the caller's index of the point at sorted position j."""
    return np.argsort(tile_ids(xyz, plan(xyz, tile0, shard_axis)), kind="stable")


def n_tiles(p):
    return p["n"][0] * p["n"][1] * p["n"][2]


def passes(p):
    """8-bit passes of the one-launch form: over the bits of the largest tile id the grid can hold."""
    bits = 1
    while bits < 18 and (1 << bits) < n_tiles(p):
        bits += 1
    return (bits + 7) // 8


def batch_perm(scans, tile0=4.0, shard_axis=-1):
    """The permutation of a whole batch: perm[base + j] = base + order(scan)[j], scans in batch order."""
    out, base = [], 0
    for s in scans:
        out.append(base + order(s, tile0, shard_axis) if len(s) else np.zeros(0, np.int64))
        base += len(s)
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
