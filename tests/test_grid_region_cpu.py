"""The region iterators without a GPU: the restatement (tests/grid_region_restate.py) against the cell sequences the reference's
own tests hold and against independent membership tests; the closed-form Bresenham the kernels use against the serial loop;
the bound of the fixed-order sum; then the header the kernels run (lio-slam_amd/csrc/lio_gridregion.h, through
tools/grid_region_host_check.cpp) against the restatement, word for word."""
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_region_restate as R                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
# lio_grid_region of include/liogpu.h (tests/test_grid_region_capi.py holds its layout against gcc's)
REGION_DTYPE = np.dtype({"names": ["kind", "n_vertices", "first_vertex", "p"], "formats": [np.int32, np.int32, np.int64, (np.float64, 5)],
                         "offsets": [0, 4, 8, 16], "itemsize": 56})


def reference_map():
    return R.Geometry(8, 5, 1.0)                               # setGeometry(Length(8.0, 5.0), 1.0, Position(0.0, 0.0)): bufferSize(8, 5)


def cells_of(region, g=None):
    status, cells, _ = R.region_cells(g or reference_map(), region)
    return status, cells


def test_polygon_iterator_sequences():
    # PolygonIteratorTest.cpp:25-63 FullCover: (0,0), (0,1), (0,2), ... (7,4), 40 cells
    st, cells = cells_of(("polygon", ((-100.0, 100.0), (100.0, 100.0), (100.0, -100.0), (-100.0, -100.0))))
    assert st == R.OK and cells == [(r, c) for r in range(8) for c in range(5)]
    # :65-79 Outside: past the end at once
    st, cells = cells_of(("polygon", ((99.0, 101.0), (101.0, 101.0), (101.0, 99.0), (99.0, 99.0))))
    assert st == R.EMPTY and cells == []
    # :81-125 Square
    st, cells = cells_of(("polygon", ((-1.0, 1.5), (1.0, 1.5), (1.0, -1.5), (-1.0, -1.5))))
    assert st == R.OK and cells == [(3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3)]
    # :127-149 TopLeftTriangle: (0,0), then (1,0)
    st, cells = cells_of(("polygon", ((-40.1, 20.6), (40.1, 20.4), (-40.1, -20.6))))
    assert st == R.OK and cells[:2] == [(0, 0), (1, 0)]


def test_ellipse_iterator_sequence():
    # EllipseIteratorTest.cpp:23-55 OneCellWideEllipse: column 2, rows 0 .. 7
    st, cells = cells_of(("ellipse", 0.0, 0.0, 8.0, 1.0, 0.0))
    assert st == R.OK and cells == [(r, 2) for r in range(8)]


def test_line_iterator_sequences():
    # LineIteratorTest.cpp:17-40 StartOutsideMap
    st, cells = cells_of(("line", 2.0, 2.0, 0.0, 0.0))
    assert st == R.OK and cells == [(2, 0), (3, 1), (4, 2)]
    # :42-70 EndOutsideMap: (4,2), (3,1), (2,1), two more increments inside, the next one past the end
    st, cells = cells_of(("line", 0.0, 0.0, 9.0, 6.0))
    assert st == R.OK and cells[:3] == [(4, 2), (3, 1), (2, 1)] and len(cells) == 5
    # :72-98 StartAndEndOutsideMap: (5,4), (4,3), (3,2), then past the end at the third further increment
    st, cells = cells_of(("line", -7.0, -9.0, 8.0, 8.0))
    assert st == R.OK and cells[:3] == [(5, 4), (4, 3), (3, 2)] and len(cells) == 5
    # :100-106 StartAndEndOutsideMapWithoutIntersectingMap: the constructor throws
    st, cells = cells_of(("line", -8.0, 8.0, 8.0, 8.0))
    assert st == R.EMPTY and cells == []


GRIDS = [(8, 5, 1.0, (0.0, 0.0)), (3, 3, 1.0, (0.0, 0.0)), (1, 1, 0.2, (0.0, 0.0)), (70, 50, 0.2, (1e3, -3e3))]


def test_circle_against_brute_force():
    """every lattice circle against (centre - c)^2 <= r^2 over all cells of the grid, written with numpy over the whole grid:
    the window never cuts a member off"""
    for rows, cols, res, pos in GRIDS:
        g = R.Geometry(rows, cols, res, pos)
        x = pos[0] + (0.5 * g.length[0] - 0.5 * res) + res * -np.arange(rows, dtype=np.float64)
        y = pos[1] + (0.5 * g.length[1] - 0.5 * res) + res * -np.arange(cols, dtype=np.float64)
        n = 0
        for region in R.lattice(g):
            if region[0] != "circle":
                continue
            st, cells, _ = R.region_cells(g, region)
            if st == R.INVALID:
                continue
            cx, cy, r = region[1:4]
            dx, dy = x[:, None] - cx, y[None, :] - cy
            want = sorted(zip(*np.nonzero(dx * dx + dy * dy <= r * r)))
            assert sorted(cells) == [(int(a), int(b)) for a, b in want], region
            assert cells == sorted(cells)                      # SubmapIterator's order is the lexicographic one
            n += 1
        assert n >= 10


def _winding_inside(vertices, p):
    """a second, differently written even-odd test: counts the edges whose crossing with the horizontal ray lies to the right,
    through the sign of a cross product instead of a division"""
    inside = False
    n = len(vertices)
    for i in range(n):
        (x0, y0), (x1, y1) = vertices[i], vertices[(i + 1) % n]
        if (y0 <= p[1]) == (y1 <= p[1]):
            continue
        cross = (x1 - x0) * (p[1] - y0) - (p[0] - x0) * (y1 - y0)
        if (cross > 0) == (y1 > y0):
            inside = not inside
    return inside


def _edge_distance(vertices, p):
    best = math.inf
    n = len(vertices)
    for i in range(n):
        (x0, y0), (x1, y1) = vertices[i], vertices[(i + 1) % n]
        ex, ey = x1 - x0, y1 - y0
        L2 = ex * ex + ey * ey
        t = 0.0 if L2 == 0 else min(1.0, max(0.0, ((p[0] - x0) * ex + (p[1] - y0) * ey) / L2))
        best = min(best, math.hypot(p[0] - (x0 + t * ex), p[1] - (y0 + t * ey)))
    return best


def test_polygon_against_independent_tests():
    """random polygons on the 70 x 50 grid against matplotlib.path where it is installed and against a second even-odd test
    written without the division, on the centres at least 1e-9 away from every edge; the window never cuts a member off"""
    try:
        from matplotlib.path import Path
    except Exception:                                          # not installed: the second test alone
        Path = None
    g = R.Geometry(70, 50, 0.2, (3.0, -2.0))
    centres = [(r, c, R.position_from_index(g, (r, c))) for r in range(70) for c in range(50)]
    checked = 0
    for region in [r for r in R.random_regions(g, 120, 7) if r[0] == "polygon"]:
        st, cells, _ = R.region_cells(g, region)
        got = set(cells)
        verts = [tuple(v) for v in region[1]]
        path = Path(np.asarray(verts + verts[:1]), closed=True) if Path is not None else None
        for r, c, p in centres:
            if _edge_distance(verts, p) < 1e-9:
                continue
            want = _winding_inside(verts, p)
            assert ((r, c) in got) == want, (region, r, c)
            if path is not None:                               # (the polygons are star-shaped: simple, so every fill rule agrees)
                assert bool(path.contains_point(p)) == want, (region, r, c)
            checked += 1
    assert checked > 50000


def test_closed_form_bresenham_equals_the_serial_loop():
    """all 63 x 63 = 3969 start / end pairs of a 9 x 7 grid"""
    cells = [(r, c) for r in range(9) for c in range(7)]
    n = 0
    for a in cells:
        for b in cells:
            serial = R.line_cells(a, b)
            assert serial[0] == a and serial[-1] == b
            assert [R.line_cell_closed_form(a, b, k) for k in range(len(serial))] == serial, (a, b)
            n += 1
    assert n == 3969


def test_sum_bound():
    """the 64 partial sums and the tree add n finite values in some order of depth at most n: the result lies within
    n 2^-53 sum|v| of the exact sum (every one of at most n - 1 additions on a path rounds by at most 2^-53 of a partial sum
    that is at most sum|v| (1 + 2^-53)^n) -- derived, not tuned"""
    g = R.Geometry(70, 50, 0.2)
    rng = np.random.default_rng(5)
    layer = ((rng.random((70, 50)) - 0.5) * 10.0 ** rng.integers(-3, 6, (70, 50))).astype(f32)
    layer[rng.random((70, 50)) < 0.1] = np.nan
    n_checked = 0
    for region in R.random_regions(g, 150, 11) + [("circle", 0.0, 0.0, 100.0)]:
        st, cells, ranks = R.region_cells(g, region)
        s, _, _, n_finite, _ = R.reduce_cells(layer, cells, ranks, 0.5)
        vals = [float(layer[r, c]) for r, c in cells if np.isfinite(layer[r, c])]
        assert len(vals) == n_finite
        exact = math.fsum(vals)
        bound = len(vals) * 2.0 ** -53 * math.fsum(abs(v) for v in vals)
        print(region[0], len(vals), abs(s - exact), bound)
        assert abs(s - exact) <= bound
        n_checked += 1 if vals else 0
    assert n_checked > 100


def pack(regions):
    rec = np.zeros(len(regions), REGION_DTYPE)
    verts = []
    for q, r in enumerate(regions):
        rec["kind"][q] = R.KIND[r[0]]
        if r[0] == "polygon":
            rec["first_vertex"][q], rec["n_vertices"][q] = len(verts), len(r[1])
            verts += [tuple(v) for v in r[1]]
        else:
            rec["p"][q, :len(r) - 1] = r[1:]
    return rec, np.asarray(verts, np.float64).reshape(-1, 2)


def host_check_dump(exe, d, g, layer, regions, threshold):
    rec, verts = pack(regions)
    np.asarray(layer, f32).ravel(order="F").tofile(os.path.join(d, "layer"))
    rec.tofile(os.path.join(d, "regions"))
    verts.tofile(os.path.join(d, "verts"))
    out = subprocess.run([exe, "dump", str(g.size[0]), str(g.size[1]), repr(g.res), repr(g.pos[0]), repr(g.pos[1]), repr(float(threshold)),
                          os.path.join(d, "layer"), os.path.join(d, "regions"), str(len(rec)), os.path.join(d, "verts"), str(len(verts)),
                          os.path.join(d, "out")], capture_output=True, text=True)
    assert out.returncode == 0 and "out-of-range accesses: 0, inconsistencies: 0" in out.stdout, out.stdout + out.stderr
    raw = open(os.path.join(d, "out"), "rb").read()
    n = len(rec)
    k = 0
    stat = np.frombuffer(raw[k:k + 24 * n], R.STAT_DTYPE); k += 24 * n
    n_cells = np.frombuffer(raw[k:k + 4 * n], np.int32); k += 4 * n
    status = np.frombuffer(raw[k:k + n], np.uint8); k += n
    offsets = np.frombuffer(raw[k:k + 8 * (n + 1)], np.int64); k += 8 * (n + 1)
    cells = np.frombuffer(raw[k:], np.int32)
    return stat, n_cells, status, offsets, cells


def assert_same_words(got, want, what):
    """(stat, n_cells, status, offsets, cells) against the restatement's, every word"""
    stat, n_cells, status, offsets, cells = got
    w_stat, w_n, w_status, w_off, w_cells = want
    assert np.array_equal(status, w_status), (what, "status", np.nonzero(status != w_status)[0][:5])
    assert np.array_equal(n_cells, w_n), (what, "n_cells", np.nonzero(n_cells != w_n)[0][:5])
    assert np.array_equal(offsets, w_off), (what, "offsets")
    assert np.array_equal(cells, w_cells), (what, "cells")
    for name in ("n_finite", "n_below", "min", "max"):
        assert np.array_equal(stat[name], w_stat[name]), (what, name, np.nonzero(stat[name] != w_stat[name]))
    assert np.array_equal(stat["sum"].view(np.uint64), w_stat["sum"].view(np.uint64)), (what, "sum", np.nonzero(stat["sum"] != w_stat["sum"]))


def restated(g, layer, regions, threshold):
    stat, n_cells, status = R.regions_reduce(g, [layer], regions, threshold)
    offsets, cells, status2 = R.regions_cells(g, regions)
    assert np.array_equal(status, status2)
    return stat[0], n_cells, status, offsets, cells


@pytest.fixture(scope="module")
def host_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grid_region_host_check")
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                               os.path.join(ROOT, "tools", "grid_region_host_check.cpp"), "-o", exe])
        yield exe, d


def test_host_check_counts_nothing(host_check):
    """the header's own run on its lattice: no read outside a layer, the two numberings name the same cells, a line's cells
    are neighbours from its start to its end"""
    exe, _ = host_check
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and out.stdout.rstrip().endswith("out-of-range accesses: 0, inconsistencies: 0")


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_header_on_the_host_equals_the_restatement(host_check, grid, holes):
    """cells, order, status, n_cells, the counts, min / max words and sum words of the header equal the restatement's on the
    lattice (every INVALID cause, the lines' special cases, windows of exactly 64, 65, 256 and 257 cells where the grid has room)"""
    exe, d = host_check
    rows, cols, res, pos = grid
    g = R.Geometry(rows, cols, res, pos)
    layer = R.make_layer(rows, cols, holes, seed=rows + cols)
    regions = R.lattice(g) + R.exact_windows(g)
    want = restated(g, layer, regions, 0.5)
    got = host_check_dump(exe, d, g, layer, regions, 0.5)
    assert_same_words(got, want, (rows, cols, holes))
    assert set(want[2]) == {R.OK, R.EMPTY, R.INVALID}
    if (rows, cols) == (70, 50):
        exact = R.exact_windows(g)
        sizes = sorted(int(v) for v in want[1][len(regions) - len(exact):])
        assert sizes == [64, 64, 65, 65, 256, 256], sizes      # (257 needs a line of the grid that long: test_exact_window_257)
        if holes:
            mn, mx = want[0]["min"], want[0]["max"]
            assert (mn == 0x80000000).any() and (mx == 0).any()                # -0.0 as a minimum, +0.0 as a maximum somewhere
            assert ((want[0]["n_finite"] == 0) & (want[1] > 0)).any()          # a region with cells and no finite one
            assert (mn[want[0]["n_finite"] == 0] == R.QNAN_BITS).all()


def test_exact_window_257(host_check):
    """a 257-cell window (1 x 257 and 257 x 1): five sweeps of a wave, the last with one cell"""
    exe, d = host_check
    for rows, cols in ((1, 300), (300, 1)):
        g = R.Geometry(rows, cols, 0.5, (-2.0, 7.0))
        layer = R.make_layer(rows, cols, True, seed=3)
        regions = R.exact_windows(g)
        want = restated(g, layer, regions, 0.25)
        assert 257 in list(want[1])
        assert_same_words(host_check_dump(exe, d, g, layer, regions, 0.25), want, (rows, cols))


def test_zero_signs_and_no_finite_cell(host_check):
    """-0.0 and +0.0 together: min is -0.0 and max is +0.0 whatever their order; a region on NaN alone: both quiet NaN"""
    exe, d = host_check
    g = R.Geometry(3, 3, 1.0)
    for flip in (False, True):
        layer = np.zeros((3, 3), f32)
        layer[::2, :] = -0.0
        if flip:
            layer = -layer
        layer[1, 1] = np.nan
        regions = [("circle", 0.0, 0.0, 5.0), ("circle", 0.0, 0.0, 0.1), ("line", 1.0, 1.0, -1.0, -1.0)]
        want = restated(g, layer, regions, 0.0)
        assert want[0]["min"][0] == 0x80000000 and want[0]["max"][0] == 0 and want[0]["n_below"][0] == 0
        assert want[0]["min"][1] == want[0]["max"][1] == R.QNAN_BITS and want[1][1] == 1 and want[0]["n_finite"][1] == 0
        assert_same_words(host_check_dump(exe, d, g, layer, regions, 0.0), want, flip)
