"""Designed inputs for the upload-time tile sort (tests/test_gpu_scan_order.py runs them on the device,
tests/test_scan_order_cases_cpu.py proves on the restatement that each reaches what its name claims).  Seeded and cached,
numpy only.  The sizes are the smallest that reach each edge: no scan of the one-launch form has more than 16383 points,
no batch more than about 70 k.

build_case(name) -> (scans: list of [n, 3] float32, cfg, note).  cfg holds ScanToMap settings (tile_size) and two keys
that are not: "shard_axis" (0..2: lio_s2m_set_shard on that axis before the upload) and "forms" (the cfg.sort_scan
values the case runs under: 2 = the one-launch form where every scan has fewer than 16384 points, 3 = the multi-kernel
form).  The arrays are shared between tests and read-only."""
import functools
import zlib

import numpy as np

ONE_LAUNCH_MAX = 16383                  # points per scan the one-launch form takes (lio_s2m_upload.hip)
TILE_CAP = 1024                         # LIO_TILE_CAP: occupancy above which a tile goes to k_scan_tile_bigsort
BIGSORT_WGS = 64                        # workgroups of k_scan_tile_bigsort
SCAN_CHUNK = 4096                       # LIO_SCAN_TILE: keys per workgroup of the three-phase scan
SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16383)
BOTH = (2, 3)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _cloud(rng, n, ext, lo=(0.0, 0.0, 0.0)):
    """n points uniform in the box [lo, lo + ext]; both corners are among them (when n >= 2), at seeded places."""
    lo = np.asarray(lo, np.float64)
    p = lo + rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(ext, np.float64)
    if n >= 2:
        i, j = rng.choice(n, 2, replace=False)
        p[i], p[j] = lo, lo + np.asarray(ext, np.float64)
    return p.astype(np.float32)


def _in_tiles(rng, coords, tile, jitter=0.8):
    """One point inside each tile of `coords` ([n, 3] integer tile coordinates of a grid with origin 0)."""
    c = np.asarray(coords, np.float64)
    return ((c + 0.1 + jitter * rng.uniform(0.0, 1.0, c.shape)) * tile).astype(np.float32)


def _with_corners(pts, n_tiles_axis, tile):
    """Overwrites the first two points so that the box is [0, (n - 1/2) * tile] per axis: a grid of exactly n_tiles_axis
    tiles with origin 0."""
    pts[0] = 0.0
    pts[1] = (np.asarray(n_tiles_axis, np.float64) - 0.5) * tile
    return pts


def _sizes(n):
    return [_cloud(_rng(f"size_{n}"), n, (100.0, 100.0, 10.0))], {}, f"one scan of {n} points, 2028 tiles"


def _size_ragged():
    rng = _rng("size_ragged")
    lens = list(SIZES[:6]) + [0] + list(SIZES[6:]) + [16383]
    scans = [_cloud(rng, n, (100.0, 100.0, 10.0), lo=(-50.0 + 3.0 * k, 20.0 * k, -5.0)) for k, n in enumerate(lens)]
    return scans, {}, "every length in one batch with an empty scan and two 16383-point scans: short scans under ROWS = 32"


def _pass1():
    return [_cloud(_rng("pass1"), 3000, (20.0, 20.0, 4.0))], {}, "72 tiles: one radix pass"


def _pass2():
    return [_cloud(_rng("pass2"), 5000, (100.0, 100.0, 10.0))], {}, "2028 tiles: two radix passes"


def _pass3():
    return [_cloud(_rng("pass3"), 12000, (60.0, 60.0, 30.0))], dict(tile_size=1.0), "115351 tiles: three radix passes"


def _limit_64cubed():
    rng = _rng("limit_64cubed")
    p = _cloud(rng, ONE_LAUNCH_MAX, (63.5, 63.5, 63.5))
    p[0] = 0.0
    p[-1] = 63.5                                            # index 16382 in tile 262143: key 0xfffffffe
    return [p], dict(tile_size=1.0), "64 x 64 x 64 = 262144 tiles (accepted by <=), the largest key the one-launch form can see"


def _top_digit():
    rng = _rng("top_digit")
    n = 4000
    c = np.zeros((n, 3), np.int64)
    c[:, 0], c[:, 1] = 17, 41
    c[:, 2] = 5 + 16 * rng.integers(0, 4, n)                # tile id bits 16..17 = tz >> 4: the third pass's digit
    p = _with_corners(_in_tiles(rng, c, 1.0), (64, 64, 64), 1.0)
    return [p], dict(tile_size=1.0), "ids that differ only in the top digit of a 262144-tile grid"


def _double_once():
    return [_cloud(_rng("double_once"), 8000, (100.0, 100.0, 40.0))], dict(tile_size=1.0), "418241 tiles at 1 m: one doubling, 54621 tiles"


def _double_twice():
    return [_cloud(_rng("double_twice"), 8000, (100.0, 100.0, 40.0))], dict(tile_size=0.5), "two doublings from 0.5 m"


def _double_262145():
    return ([_cloud(_rng("double_262145"), 6000, (64.5, 36.5, 108.5))], dict(tile_size=1.0),
            "65 x 37 x 109 = 262145 tiles, one above the limit: one doubling")


def _one_tile_copies():
    return [np.tile(np.array([[1.25, -2.5, 0.75]], np.float32), (ONE_LAUNCH_MAX, 1))], {}, "16383 copies of one point"


def _one_tile_distinct():
    return [_cloud(_rng("one_tile_distinct"), ONE_LAUNCH_MAX, (3.9, 3.9, 3.9), lo=(10.0, 10.0, 10.0))], {}, "16383 distinct points of one tile"


def _lattice16():
    g = np.arange(16)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1]     # x fastest: row i is tile id i


def _own_tile():
    rng = _rng("own_tile")
    c = _lattice16()[rng.permutation(4096)]
    return [(c * 4.0 + 2.0).astype(np.float32)], {}, "4096 points, each alone in its tile, shuffled"


def _descending():
    c = _lattice16()[::-1]
    return [(c * 4.0 + 2.0).astype(np.float32)], {}, "tile ids strictly descending in the caller's order"


def _interleave(stride):
    rng = _rng(f"interleave_{stride}")
    n = 4096
    in_a = (np.arange(n) // stride) % 2 == 0
    c = np.where(in_a[:, None], np.array([[7, 3, 1]]), np.array([[2, 3, 1]]))          # the first run sits in the HIGHER tile
    p = _in_tiles(rng, c, 4.0)
    p[stride] = c[stride] * 4.0                             # (the lower tile's own corner: the box starts on a tile face)
    return [p], {}, f"two tiles alternating every {stride} points: ties across lane, row and wave boundaries"


def _crowded():
    rng = _rng("crowded")
    single = _cloud(rng, 5000, (60.0, 60.0, 30.0))
    crowd = [_cloud(rng, 1000, (0.9, 0.9, 0.9), lo=lo) for lo in ((10.0, 20.0, 5.0), (40.0, 7.0, 22.0), (59.0, 59.0, 29.0))]
    p = np.concatenate([single] + crowd)
    p = p[rng.permutation(len(p))]
    return [p], dict(tile_size=1.0), "three tiles of about 1000 points among thousands of singletons"


def _shard(axis):
    return ([_cloud(_rng(f"shard_{axis}"), 3000, (34.0, 18.0, 10.0), lo=(-3.0, 5.0, -1.0))], dict(shard_axis=axis),
            f"9 x 5 x 3 tiles, shard axis {axis} slowest")


def _nonfinite_single():
    rng = _rng("nonfinite_single")
    p = _cloud(rng, 5000, (60.0, 40.0, 8.0), lo=(-30.0, -20.0, -2.0))
    bad = rng.choice(np.arange(2, 5000), 400, replace=False)
    p[bad, rng.integers(0, 3, 400)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 400)
    return [p], {}, "NaN, +inf and -inf in single coordinates of 8 % of the points"


def _edge_3e38():
    rng = _rng("edge_3e38")
    p = _cloud(rng, 3000, (60.0, 40.0, 8.0))
    p[5, 0], p[6, 0], p[7, 1] = 3.0e38, -3.0e38, 3.0e38     # inside the box limit: they stretch the box
    p[100:110, 0], p[110:120, 0], p[120:130, 1] = 3.2e38, -3.2e38, 3.2e38       # outside it: clamped into the end tiles
    p[130:140, 2] = 3.2e38
    return [p], {}, "coordinates at 3.0e38 (in the box) and 3.2e38 (outside, clamped)"


def _all_nonfinite():
    rng = _rng("all_nonfinite")
    p = rng.choice(np.array([np.nan, np.inf, -np.inf, 3.2e38, -3.3e38], np.float32), (1000, 3))
    return [p], {}, "no coordinate inside the box limit: box [0, 0], one tile, the caller's order"


def _tile_faces():
    rng = _rng("tile_faces")
    p = (-8.0 + 4.0 * rng.integers(0, 11, (3000, 3))).astype(np.float32)
    p[::3] += np.float32(2.0)
    p[0], p[1] = -8.0, 32.0
    return [p], {}, "points exactly on tile faces o + k * tile"


def _far_origin():
    return ([_cloud(_rng("far_origin"), 5000, (50.0, 50.0, 10.0), lo=(1.0e6, -1.0e6, 1.0e6))], {},
            "a cloud 10^6 m from the origin (fp32 spacing 1/16 m)")


def _neg_zero():
    rng = _rng("neg_zero")
    vals = np.array([-0.0, 0.0, -4.0, 4.0, -1.0e-30, 1.0e-30, 3.5, -3.5, 8.0], np.float32)
    a = rng.choice(vals, (2000, 3))
    b = np.abs(rng.choice(vals, (2000, 3)))
    b[::2] = np.where(b[::2] == 0.0, np.float32(-0.0), b[::2])      # the smallest coordinate is a negative zero
    return [a, b], {}, "negative zeros, inside the box and as its minimum"


def _tile_odd(tile):
    rng = _rng(f"tile_{tile}")
    p = _cloud(rng, 6000, (40.0, 40.0, 8.0))
    k = rng.integers(0, 26, (1500, 3)).astype(np.float32) * np.float32(tile)         # (on the faces of the asked grid)
    p[2:1502] = np.minimum(k, np.array([40.0, 40.0, 8.0], np.float32))
    return [p], dict(tile_size=tile), f"tile edge {tile}: the quotient 1 / tile is not exact"


def _handover(n):
    return ([_cloud(_rng(f"handover_{n}"), n, (100.0, 100.0, 10.0))], dict(forms=(2,)),
            f"{n} points under sort_scan = 2: handed to the multi-kernel form")


OCCUPANCIES = (1023, 1024, 1025, 2047, 2048, 2049, 5000)


def _occupancy_edges():
    rng = _rng("occupancy_edges")
    parts = [_cloud(rng, m, (3.5, 3.5, 3.5), lo=(8.0 * k + 0.25, 4.25, 0.25)) for k, m in enumerate(OCCUPANCIES)]
    parts.append(_cloud(rng, 200, (60.0, 3.5, 3.5), lo=(0.0, 8.5, 0.25)))          # (the next row of tiles: the counts above stay exact)
    p = np.concatenate(parts)
    p = p[rng.permutation(len(p))]
    return [p], {}, "tile occupancies on both sides of 1024 and 2048, and 5000: ranksort against bigsort, odd bitonic sizes"


def _oversized_70():
    rng = _rng("oversized_70")
    scans = []
    for s in range(5):
        parts = [_cloud(rng, TILE_CAP + 1, (3.5, 3.5, 3.5), lo=(8.0 * k + 0.25, 4.0 * s + 0.25, 0.25)) for k in range(14)]
        p = np.concatenate(parts)
        scans.append(p[rng.permutation(len(p))])
    return scans, {}, "70 tiles of 1025 points in one batch: more than the 64 workgroups of the big-tile sort"


def _many_keys():
    rng = _rng("many_keys")
    scans = []
    for s in range(5):
        p = _cloud(rng, 2000 + 37 * s, (63.5, 63.5, 63.5), lo=(100.0 * s, -30.0, 2.0 * s))
        scans.append(p)
    return scans, dict(tile_size=1.0), "five grids of 262144 tiles: 1310720 keys, more than one chunk of the offset scan"


_CASES = {f"size_{n}": functools.partial(_sizes, n) for n in SIZES}
_CASES.update({
    "size_ragged": _size_ragged, "pass1": _pass1, "pass2": _pass2, "pass3": _pass3, "limit_64cubed": _limit_64cubed,
    "top_digit": _top_digit, "double_once": _double_once, "double_twice": _double_twice, "double_262145": _double_262145,
    "one_tile_copies": _one_tile_copies, "one_tile_distinct": _one_tile_distinct, "own_tile": _own_tile, "descending": _descending,
    "interleave_1": functools.partial(_interleave, 1), "interleave_64": functools.partial(_interleave, 64),
    "interleave_512": functools.partial(_interleave, 512), "crowded": _crowded,
    "shard_0": functools.partial(_shard, 0), "shard_1": functools.partial(_shard, 1), "shard_2": functools.partial(_shard, 2),
    "nonfinite_single": _nonfinite_single, "edge_3e38": _edge_3e38, "all_nonfinite": _all_nonfinite, "tile_faces": _tile_faces,
    "far_origin": _far_origin, "neg_zero": _neg_zero, "tile_1.5": functools.partial(_tile_odd, 1.5),
    "tile_0.3": functools.partial(_tile_odd, 0.3),
    "handover_16384": functools.partial(_handover, 16384), "handover_16385": functools.partial(_handover, 16385),
    "occupancy_edges": _occupancy_edges, "oversized_70": _oversized_70, "many_keys": _many_keys,
})
NAMES = tuple(_CASES)

# what the summary of a run counts the cases by
GROUPS = {
    "sizes": tuple(f"size_{n}" for n in SIZES) + ("size_ragged",),
    "radix passes": ("pass1", "pass2", "pass3", "limit_64cubed", "top_digit"),
    "tile doubling": ("double_once", "double_twice", "double_262145"),
    "order and stability": ("one_tile_copies", "one_tile_distinct", "own_tile", "descending", "interleave_1", "interleave_64",
                            "interleave_512", "crowded"),
    "shard axis": ("shard_0", "shard_1", "shard_2"),
    "coordinates": ("nonfinite_single", "edge_3e38", "all_nonfinite", "tile_faces", "far_origin", "neg_zero"),
    "tile sizes": ("tile_1.5", "tile_0.3"),
    "multi-kernel form": ("handover_16384", "handover_16385", "occupancy_edges", "oversized_70", "many_keys"),
}


@functools.lru_cache(maxsize=None)
def build_case(name):
    scans, cfg, note = _CASES[name]()
    scans = [np.ascontiguousarray(s, np.float32).reshape(-1, 3) for s in scans]
    for s in scans:
        s.flags.writeable = False
    cfg = dict(cfg)
    cfg.setdefault("forms", BOTH)
    return scans, cfg, note


def tile0_of(cfg):
    """The tile edge the upload asks for under cfg (cfg.tile_size <= 0: 4 m)."""
    t = cfg.get("tile_size", 0.0)
    return t if t > 0.0 else 4.0


def handle_cfg(cfg):
    """The ScanToMap settings of cfg (without the keys that are not)."""
    return {k: v for k, v in cfg.items() if k not in ("shard_axis", "forms")}
