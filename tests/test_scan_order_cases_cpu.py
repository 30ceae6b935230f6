"""The designed inputs of tests/scan_order_cases.py checked without a GPU: on the restatement alone
(tests/scan_order_restate.py) every case reaches what its name claims -- radix passes, doublings, the tile count at the limit,
the highest key, occupancies on both sides of LIO_TILE_CAP, more oversized tiles than workgroups, more keys than one chunk
of the offset scan, an anisotropic grid, the share of non-finite coordinates -- and the restatement's grid equals the one
the library itself lays out (lio_plan_scan_tiles through the host-only hook lio_debug_scan_tile_plan), field for field,
inv_tile by bits."""
import importlib

import numpy as np
import pytest

import scan_order_cases as sc
import scan_order_restate as so

F = np.float32


def _plans(name):
    scans, cfg, _ = sc.build_case(name)
    return scans, cfg, [so.plan(s, sc.tile0_of(cfg), cfg.get("shard_axis", -1)) for s in scans]


def _occupancy(scan, p):
    return np.bincount(so.tile_ids(scan, p), minlength=so.n_tiles(p))


def test_every_case_is_grouped_once_and_within_the_size_limits():
    grouped = [n for g in sc.GROUPS.values() for n in g]
    assert sorted(grouped) == sorted(sc.NAMES) and len(set(grouped)) == len(grouped)
    for name in sc.NAMES:
        scans, cfg, note = sc.build_case(name)
        assert note and all(s.dtype == F and s.ndim == 2 and s.shape[1] == 3 for s in scans)
        assert sum(len(s) for s in scans) <= 72000, name
        if 3 in cfg["forms"]:                              # (runs under both forms: the one-launch form must take every scan)
            assert cfg["forms"] == sc.BOTH and max(len(s) for s in scans) <= sc.ONE_LAUNCH_MAX, name
        assert sc.build_case(name)[0][0] is scans[0]        # cached: one reference shared by the tests


def test_sizes():
    for n in sc.SIZES:
        (scan,), _, (p,) = _plans(f"size_{n}")
        assert len(scan) == n
        assert n < 3 or (so.n_tiles(p) == 2028 and so.passes(p) == 2)
    scans, _, _ = _plans("size_ragged")
    lens = [len(s) for s in scans]
    assert set(sc.SIZES) | {0} == set(lens) and max(lens) == 16383 > 16 * 512 and lens[-1] == 16383
    # rows = ceil(n / 512), first = wave * rows * 64: lengths with idle waves, a last row partly filled, and exactly full rows
    rows = {n: -(-n // 512) for n in sc.SIZES}
    assert any(7 * rows[n] * 64 >= n for n in sc.SIZES) and any(n % 64 for n in sc.SIZES) and any(n % 512 == 0 for n in sc.SIZES)
    assert rows[8192] == 16 and rows[8193] == 17 and rows[16383] == 32


@pytest.mark.parametrize("name,tiles,n_pass", [("pass1", 72, 1), ("pass2", 2028, 2), ("pass3", 61 * 61 * 31, 3),
                                               ("limit_64cubed", 262144, 3), ("top_digit", 262144, 3)])
def test_radix_passes(name, tiles, n_pass):
    (scan,), _, (p,) = _plans(name)
    assert so.n_tiles(p) == tiles and so.passes(p) == n_pass and p["doublings"] == 0
    ids = so.tile_ids(scan, p)
    if name == "limit_64cubed":
        assert len(scan) == 16383 and ids[-1] == 262143 and ids.max() == 262143
        assert (int(ids[-1]) << 14 | (len(scan) - 1)) == so.EMPTY_KEY - 1          # the largest key, one below the empty-slot marker
    if name == "top_digit":
        rest = ids[2:]                                      # (the two corner points only fix the box)
        assert len(np.unique(rest)) == 4 and len(np.unique(rest & 0xffff)) == 1 and len(np.unique(rest >> 16)) == 4
        assert np.any(np.diff(rest) < 0)                    # not already in order


@pytest.mark.parametrize("name,first,doublings,tiles", [("double_once", 101 * 101 * 41, 1, 51 * 51 * 21),
                                                        ("double_twice", 201 * 201 * 81, 2, 51 * 51 * 21),
                                                        ("double_262145", 262145, 1, 33 * 19 * 55)])
def test_tile_doubling(name, first, doublings, tiles):
    (scan,), cfg, (p,) = _plans(name)
    lo, hi = so.box(scan)
    t0 = sc.tile0_of(cfg)
    at_first = np.prod([np.floor((float(hi[a]) - float(lo[a])) / t0) + 1 for a in range(3)])
    assert at_first == first > 262144
    assert p["doublings"] == doublings and so.n_tiles(p) == tiles and p["tile"] == F(t0 * 2 ** doublings)


def test_order_and_stability_cases():
    for name in ("one_tile_copies", "one_tile_distinct"):
        (scan,), cfg, (p,) = _plans(name)
        assert len(scan) == 16383 and so.n_tiles(p) == 1
        assert np.array_equal(so.order(scan, sc.tile0_of(cfg)), np.arange(len(scan)))
        assert len(np.unique(scan, axis=0)) == (1 if name == "one_tile_copies" else len(scan))
    (scan,), _, (p,) = _plans("own_tile")
    ids = so.tile_ids(scan, p)
    assert so.n_tiles(p) == 4096 == len(scan) and np.array_equal(np.sort(ids), np.arange(4096)) and np.any(np.diff(ids) < 0)
    (scan,), _, (p,) = _plans("descending")
    assert np.array_equal(so.tile_ids(scan, p), np.arange(4096)[::-1])
    for stride in (1, 64, 512):
        (scan,), _, (p,) = _plans(f"interleave_{stride}")
        ids = so.tile_ids(scan, p)
        a, b = ids[0], ids[stride]
        assert a > b and np.array_equal(ids, np.where((np.arange(len(ids)) // stride) % 2 == 0, a, b))
        assert len(scan) == 4096 and -(-len(scan) // 512) * 64 == 512              # a wave holds 512 consecutive points
        assert len(np.unique(scan, axis=0)) == len(scan)
    (scan,), _, (p,) = _plans("crowded")
    occ = _occupancy(scan, p)
    assert np.sum(occ >= 900) == 3 and np.sum(occ == 1) > 4000 and so.passes(p) == 3


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_shard_axis_cases(axis):
    (scan,), cfg, (p,) = _plans(f"shard_{axis}")
    assert cfg["shard_axis"] == axis and p["n"] == [9, 5, 3]
    slow = int(np.argmax(p["k"]))
    assert slow == axis and sorted(p["k"])[0] == 1
    # three different extents: the id under any other axis order, or under swapped strides, differs for some point
    ids = so.tile_ids(scan, p)
    for other in (-1, 0, 1, 2):
        q = so.plan(scan, sc.tile0_of(cfg), other)
        same = np.array_equal(np.argsort(so.tile_ids(scan, q), kind="stable"), np.argsort(ids, kind="stable"))
        assert same == (q["k"] == p["k"])
    assert len(np.unique(ids)) == 9 * 5 * 3                 # every tile is hit


def test_coordinate_cases():
    (scan,), cfg, (p,) = _plans("nonfinite_single")
    bad = ~np.isfinite(scan)
    assert 0.07 <= bad.any(axis=1).mean() <= 0.09 and bad.sum(axis=1).max() == 1
    assert np.isnan(scan).any() and np.isposinf(scan).any() and np.isneginf(scan).any()
    c = so.tile_coords(scan, p)
    assert np.all(c[np.isnan(scan)] == 0) and np.all(c[np.isneginf(scan)] == 0)
    assert np.all(c[np.isposinf(scan)] == (np.array(p["n"]) - 1)[np.nonzero(np.isposinf(scan))[1]])

    (scan,), cfg, (p,) = _plans("edge_3e38")
    lo, hi = so.box(scan)
    assert lo[0] == F(-3.0e38) and hi[0] == F(3.0e38) and hi[1] == F(3.0e38) and hi[2] < 10.0 and p["doublings"] > 100
    assert np.isfinite(p["inv"]) and p["inv"] > 0.0 and so.n_tiles(p) > 1
    c = so.tile_coords(scan, p)
    assert np.all(c[scan[:, 0] == F(3.2e38), 0] == p["n"][0] - 1) and np.all(c[scan[:, 0] == F(-3.2e38), 0] == 0)
    assert np.all(c[scan[:, 1] == F(3.2e38), 1] == p["n"][1] - 1) and F(3.2e38) > so.BOX_LIMIT and np.isfinite(F(3.2e38))

    (scan,), cfg, (p,) = _plans("all_nonfinite")
    assert not np.any(np.abs(scan) <= so.BOX_LIMIT) and np.isfinite(scan).any()
    assert np.all(so.box(scan)[0] == 0) and np.all(so.box(scan)[1] == 0) and so.n_tiles(p) == 1
    assert np.array_equal(so.order(scan), np.arange(len(scan)))

    (scan,), cfg, (p,) = _plans("tile_faces")
    rel = (scan.astype(np.float64) - p["o"]) / 4.0
    assert p["n"] == [11, 11, 11] and np.mean(rel == np.floor(rel)) > 0.6
    assert np.array_equal(so.tile_coords(scan, p), np.minimum(np.floor(rel), 10))

    (scan,), cfg, (p,) = _plans("far_origin")
    assert np.abs(scan).min() > 9.9e5 and np.spacing(F(1.0e6)) == 0.0625 and so.passes(p) == 2

    scans, cfg, plans = _plans("neg_zero")
    for s in scans:
        assert np.any(np.signbit(s) & (s == 0.0)) and np.any(~np.signbit(s) & (s == 0.0))
    assert np.all(scans[1] >= 0.0) and np.all(plans[1]["o"] == 0.0) and np.all(plans[0]["o"] < 0.0)


@pytest.mark.parametrize("tile", [1.5, 0.3])
def test_tile_sizes_that_are_no_power_of_two(tile):
    (scan,), cfg, (p,) = _plans(f"tile_{tile}")
    inv = F(1.0) / F(p["tile"])
    assert p["inv"].dtype == F and p["inv"].view(np.uint32) == inv.view(np.uint32)
    assert float(inv) * float(p["tile"]) != 1.0                                 # the quotient is rounded
    assert p["doublings"] == (0 if tile == 1.5 else 1)
    on_face = np.isin(scan[:, 0], np.arange(27, dtype=F) * F(tile)).mean()             # x = k * tile, the product in fp32
    assert on_face > 0.2


def test_multi_kernel_cases():
    for n in (16384, 16385):
        (scan,), cfg, _ = _plans(f"handover_{n}")
        assert len(scan) == n > sc.ONE_LAUNCH_MAX and cfg["forms"] == (2,)
    (scan,), _, (p,) = _plans("occupancy_edges")
    occ = _occupancy(scan, p)
    big = np.sort(occ[occ > 500])
    assert list(big) == sorted(sc.OCCUPANCIES)
    assert {sc.TILE_CAP - 1, sc.TILE_CAP, sc.TILE_CAP + 1} <= set(big) and np.sum(big > sc.TILE_CAP) == 5
    assert not np.all(np.diff(so.tile_ids(scan, p)) >= 0)

    scans, _, plans = _plans("oversized_70")
    over = sum(int(np.sum(_occupancy(s, p) > sc.TILE_CAP)) for s, p in zip(scans, plans))
    assert over == 70 > sc.BIGSORT_WGS
    assert all(set(_occupancy(s, p)) == {0, sc.TILE_CAP + 1} for s, p in zip(scans, plans))

    scans, _, plans = _plans("many_keys")
    keys = sum(so.n_tiles(p) for p in plans)
    assert keys == 5 * 262144 > 256 * sc.SCAN_CHUNK and len(scans) == 5
    assert all(so.n_tiles(p) > sc.SCAN_CHUNK for p in plans[:-1])                # key_offset of every later scan crosses chunks


# ------------------------------------------------------------------------------------ the library's own plan
def _same_plan(api, lo, hi, tile, axis):
    p = so.plan_box(lo, hi, tile, axis)
    q = api.debug_scan_tile_plan(lo, hi, tile, axis)
    assert [q["ntx"], q["nty"], q["ntz"]] == p["n"], (lo, hi, tile, axis)
    assert [q["mx"], q["my"], q["mz"]] == p["k"], (lo, hi, tile, axis)
    assert np.array_equal(np.array([q["ox"], q["oy"], q["oz"]], F).view(np.uint32), np.asarray(lo, F).view(np.uint32))
    assert F(q["inv_tile"]).view(np.uint32) == F(p["inv"]).view(np.uint32), (lo, hi, tile, axis, q["inv_tile"], p["inv"])


def test_library_plan_equals_the_restatement(pkg):
    api = importlib.import_module("lio-slam_amd.api")
    n = 0
    for name in sc.NAMES:
        scans, cfg, _ = sc.build_case(name)
        for s in scans:
            lo, hi = so.box(s)
            _same_plan(api, lo, hi, sc.tile0_of(cfg), cfg.get("shard_axis", -1))
            n += 1
    assert n >= len(sc.NAMES)
    rng = np.random.default_rng(20)
    for i in range(400):
        lo = (rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(-2, 6, 3)).astype(F)
        ext = (10.0 ** rng.uniform(-3, 4, 3)).astype(F)
        if i % 7 == 0:
            ext[rng.integers(0, 3)] = 0.0
        hi = (lo + ext).astype(F)
        tile = float(F(rng.choice([4.0, 1.0, 0.5, 1.5, 0.3, 0.1, 16.0, 1.0e4, float(10.0 ** rng.uniform(-2, 2))])))
        _same_plan(api, lo, hi, tile, int(rng.integers(-1, 3)))
    zero = np.zeros(3, F)
    for axis in (-1, 0, 1, 2):
        for tile in (4.0, 0.3, 1.0e-3):
            for at in (zero, np.array([5.5, -7.25, 1.0e6], F)):
                _same_plan(api, at, at, tile, axis)                                   # degenerate: mn == mx, one tile
            huge_lo, huge_hi = np.full(3, -3.0e38, F), np.full(3, 3.0e38, F)          # extent 6e38: beyond FLT_MAX in fp32
            _same_plan(api, huge_lo, huge_hi, tile, axis)
            _same_plan(api, np.array([-3.0e38, 0.0, 0.0], F), np.array([3.0e38, 40.0, 0.0], F), tile, axis)
    p = so.plan_box(zero, zero, 4.0)
    assert p["n"] == [1, 1, 1] and so.passes(p) == 1
    p = so.plan_box(np.full(3, -3.0e38, F), np.full(3, 3.0e38, F), 4.0)
    assert so.n_tiles(p) <= 262144 and p["doublings"] > 100 and p["inv"] > 0.0


def test_plan_hook_refuses_what_it_cannot_plan(pkg):
    api = importlib.import_module("lio-slam_amd.api")
    z = np.zeros(3, F)
    for tile, axis in ((0.0, -1), (-1.0, 0), (float("nan"), 1), (4.0, 3), (4.0, -2)):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            api.debug_scan_tile_plan(z, z, tile, axis)
