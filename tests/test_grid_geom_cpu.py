"""The restatement of lio_grid_submap, lio_grid_move, lio_grid_extend_to_include and lio_grid_add_data_from
(tests/grid_geom_restate.py) without a GPU, against the reference's own test values (grid_map_core/test/GridMapTest.cpp: Move,
AddDataFrom.*; GridMapMathTest.cpp: getSubmapInformation.*, getIndexShiftFromPositionShift.All); then the header the kernels
run (lio-slam_amd/csrc/lio_gridgeom.h, through tools/grid_geom_host_check.cpp) against the restatement, word for word."""
import math
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_sample_restate as gs                               # noqa: E402
import grid_geom_restate as R                                  # noqa: E402
import grid_geom_cases as K                                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


def double_eq(a, b):
    """EXPECT_DOUBLE_EQ: within 4 ulps"""
    ia, ib = struct.unpack("<q", struct.pack("<d", a))[0], struct.unpack("<q", struct.pack("<d", b))[0]
    return a == b or (a * b > 0 and abs(ia - ib) <= 4)


def at_position(m, k, p):
    """atPosition(layer, position), nearest"""
    verdict, index = R.index_from_position(m, p, m.start)
    assert verdict
    return float(m.data[k][index])


def new_map(length, res, pos, layers):
    """setGeometry, then add(layer, value) per entry of {id: value}"""
    m = R.GridMap()
    m.set_geometry(length, res, pos)
    for k, v in layers.items():
        m.add(k, v)
    m.basic = list(m.ids)
    return m


# ---- GridMapTest.cpp
def test_move_literal():
    """GridMapTest.cpp:52-89 on the circular buffer, then unwrapped"""
    m = new_map((8.1, 5.1), 1.0, (0.0, 0.0), {0: 0.0})
    assert m.size == (8, 5)
    moved, regions, shift = m.move((-3.0, -2.0))
    assert moved and shift == (3, 2) and m.start == (3, 2) and m.pos == (-3.0, -2.0)
    want = np.zeros((8, 5), bool)
    want[3:, 2:] = True                                        # the test's isValidExpected, by buffer index
    got = np.array([[m.is_valid((r, c)) for c in range(5)] for r in range(8)])
    assert np.array_equal(got, want)
    assert regions == [((0, 0), (3, 5)), ((0, 0), (8, 2))]
    m.convert_to_default_start_index()
    want = np.zeros((8, 5), bool)
    want[:5, :3] = True
    assert m.start == (0, 0) and np.array_equal(np.isfinite(m.data[0]), want)


@pytest.mark.parametrize("target", [(-3.0, -2.0), (3.0, 2.0), (-1.0, 4.0), (7.0, -1.0), (8.0, 0.0), (0.0, 0.0), (0.4, -0.4), (-2.5, 2.5), (100.0, -1.0)])
def test_move_unwrapped_is_a_shifted_copy(target):
    """twice in a row, so that the second move starts from a wrapped buffer: new cell (r, c) = old cell (r + shift0, c + shift1)"""
    layers = K.layers_of((8, 5), 3, 4)
    m = R.GridMap.of(gs.Geometry(8, 5, 1.0), layers)
    held = [layers[k].copy() for k in range(3)]
    for t in (target, (target[0] * 0.5 + 1.0, -target[1])):
        _, _, shift = m.move(t)
        held = [R.shifted_copy(h, shift) for h in held]
        flat = m.copy()
        flat.convert_to_default_start_index()
        assert np.array_equal(flat.words(), np.stack(held).view(u32)), (t, shift)
    one = R.GridMap.of(gs.Geometry(8, 5, 1.0), layers)
    info = R.lib_move(one, target)
    kept = max(0, 8 - abs(info["index_shift"][0])) * max(0, 5 - abs(info["index_shift"][1]))
    assert info["n_cells_cleared"] == (40 - kept if info["moved"] else 0)


def test_add_data_from_extend_map_aligned():
    """GridMapTest.cpp:359-384"""
    m1 = new_map((5.1, 5.1), 1.0, (0.0, 0.0), {0: 0.0, 1: 1.0})                  # zero, one
    m2 = new_map((3.1, 3.1), 1.0, (2.0, 2.0), {1: 1.1, 2: 2.0})                  # one, two
    out = m1.add_data_from(m2, True, True, True)
    assert 2 in m1.ids and gs.within_map(m1, (3.0, 3.0)) and out["resized"] == 1
    assert double_eq(6.0, m1.length[0]) and double_eq(6.0, m1.length[1]) and double_eq(0.5, m1.pos[0]) and double_eq(0.5, m1.pos[1])
    assert abs(at_position(m1, 1, (2.0, 2.0)) - 1.1) <= 1e-4
    assert at_position(m1, 1, (-2.0, -2.0)) == 1.0 and at_position(m1, 0, (0.0, 0.0)) == 0.0
    assert out["n_index_outside"] == 0 and out["n_values_copied"] == 18 and out["n_cells_outside_other"] == 27


def test_add_data_from_extend_map_not_aligned():
    """GridMapTest.cpp:386-417"""
    m1 = new_map((6.1, 6.1), 1.0, (0.0, 0.0), {0: R.QNAN, 1: 1.0, 2: 0.0})       # nan, one, zero
    m2 = new_map((3.1, 3.1), 1.0, (3.2, 3.2), {0: 1.0, 1: 1.1, 3: 2.0})          # nan, one, two
    m1.add_data_from(m2, True, False, False, [0])
    _, index = R.index_from_position(m1, (-2.0, -2.0))
    assert 3 not in m1.ids and gs.within_map(m1, (4.0, 4.0))
    assert double_eq(8.0, m1.length[0]) and double_eq(8.0, m1.length[1]) and double_eq(1.0, m1.pos[0]) and double_eq(1.0, m1.pos[1])
    assert not m1.is_valid(index, [0])
    assert at_position(m1, 1, (0.0, 0.0)) == 1.0 and at_position(m1, 0, (3.0, 3.0)) == 1.0


def test_add_data_from_copy_data():
    """GridMapTest.cpp:419-446"""
    m1 = new_map((5.1, 5.1), 1.0, (0.0, 0.0), {0: 0.0, 1: R.QNAN})                # zero, one
    m2 = new_map((3.1, 3.1), 1.0, (2.0, 2.0), {1: 1.0, 2: 2.0})                  # one, two
    out = m1.add_data_from(m2, False, False, True)
    _, index = R.index_from_position(m1, (-2.0, -2.0))
    assert 2 in m1.ids and not gs.within_map(m1, (3.0, 3.0)) and out["resized"] == 0
    assert m1.length == (5.0, 5.0) and m1.pos == (0.0, 0.0)
    assert at_position(m1, 1, (2.0, 2.0)) == 1.0 and not m1.is_valid(index, [1]) and at_position(m1, 0, (0.0, 0.0)) == 0.0


# ---- GridMapMathTest.cpp
def plain(size, res, length, pos):
    return types.SimpleNamespace(size=size, res=res, length=length, pos=pos)


def test_submap_information_literals():
    g = plain((5, 4), 1.0, (5.0, 4.0), (0.0, 0.0))
    for clamp in (False, True):
        s = R.submap_information(g, (0.0, 0.5), (0.9, 2.9), clamp=clamp)                       # Simple, :488-521
        assert s["top_left"] == (2, 0) and s["size"] == (1, 3) and s["requested"] == (0, 1)
        assert double_eq(0.0, s["position"][0]) and double_eq(0.5, s["position"][1]) and double_eq(1.0, s["length"][0]) and double_eq(3.0, s["length"][1])
        s = R.submap_information(g, (-1.0, -0.5), (0.0, 0.0), clamp=clamp)                     # Zero, :523-557
        assert s["top_left"] == (3, 2) and s["size"] == (1, 1) and s["requested"] == (0, 0)
        assert double_eq(-1.0, s["position"][0]) and double_eq(-0.5, s["position"][1]) and double_eq(1.0, s["length"][0]) and double_eq(1.0, s["length"][1])
        s = R.submap_information(g, (2.0, 1.5), (2.9, 2.9), clamp=clamp)                       # ExceedingBoundaries, :578-592
        assert s["top_left"] == (0, 0) and s["size"] == (2, 2) and s["requested"] == (0, 0)
        assert double_eq(1.5, s["position"][0]) and double_eq(1.0, s["position"][1]) and double_eq(2.0, s["length"][0]) and double_eq(2.0, s["length"][1])
        s = R.submap_information(g, (0.0, 0.0), (1e6, 1e6), clamp=clamp)                       # :594-609
        assert s["top_left"] == (0, 0) and s["size"] == (5, 4) and s["requested"][0] == 2 and 1 <= s["requested"][1] <= 2
        assert double_eq(0.0, s["position"][0]) and double_eq(0.0, s["position"][1]) and double_eq(5.0, s["length"][0]) and double_eq(4.0, s["length"][1])
        # a requested centre outside the map fails
        assert R.submap_information(g, (10.0, 0.0), (1.0, 1.0), clamp=clamp) is None
        assert R.submap_information(g, (0.0, -2.5), (1.0, 1.0), clamp=clamp) is None
    s = R.submap_information(plain((83, 83), 0.06, (4.98, 4.98), (-4.98, -5.76)), (-7.44, -3.42), (0.12, 0.12), start=(0, 13))     # Debug1, :682-709
    assert s["size"] == (2, 3) and double_eq(0.12, s["length"][0]) and double_eq(0.18, s["length"][1])
    s = R.submap_information(plain((83, 83), 0.06, (4.98, 4.98), (2.46, -25.26)), (0.24, -26.82), (0.624614, 0.462276), start=(42, 6))   # Debug2, :711-738
    assert s["size"][0] > 0 and s["size"][1] > 0 and s["length"][0] > 0.0 and s["length"][1] > 0.0


def test_index_shift_from_position_shift_literals():
    """GridMapMathTest.cpp:247-271"""
    for shift, res, want in (((0.0, 0.0), 1.0, (0, 0)), ((0.35, -0.45), 1.0, (0, 0)), ((0.55, -0.45), 1.0, (-1, 0)), ((-1.3, -2.65), 1.0, (1, 3)),
                             ((-0.4, 0.09), 0.2, (2, 0))):
        assert tuple(R.index_shift(s, res) for s in shift) == want
    assert R.index_shift(0.5, 1.0) == -1 and R.index_shift(-0.5, 1.0) == 1 and R.index_shift(0.49, 1.0) == 0
    for bad in (2.0 ** 30, -2.0 ** 30, math.inf, math.nan):
        with pytest.raises(ValueError):
            R.index_shift(bad, 1.0)


def test_clamped_corner_rule_agrees_on_every_window():
    """the library's corner rule (lio_gm_bound_index's clamp) against the reference's verdict over the windows the tests use"""
    n = 0
    for rows, cols, _, res in K.shapes():
        g = K.geometry(rows, cols, res)
        for position, length in K.submap_windows(g):
            a, b = R.submap_information(g, position, length), R.submap_information(g, position, length, clamp=True)
            if a is not None:
                assert a == b
                n += 1
    assert n > 100


# ---- the header on the host
@pytest.fixture(scope="module")
def host_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grid_geom_host_check")
        subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                               os.path.join(ROOT, "tools", "grid_geom_host_check.cpp"), "-o", exe])
        yield exe, d


def geo_args(g, mask):
    return [str(g.size[0]), str(g.size[1]), repr(g.res), repr(g.pos[0]), repr(g.pos[1]), str(mask)]


def put_layers(path, layers):
    np.stack([np.asarray(l, f32).ravel(order="F") for l in layers]).tofile(path)


def run(exe, d, args):
    out = subprocess.run([exe] + args + [os.path.join(d, "out")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(os.path.join(d, "out"), "rb").read()
    head = np.frombuffer(raw, np.int32, 8)
    geo = np.frombuffer(raw, np.float64, 4, 32)
    cnt = np.frombuffer(raw, np.int64, 6, 64)
    rows, cols, mask = int(head[1]), int(head[2]), int(head[3])
    n = bin(mask).count("1")
    words = np.frombuffer(raw, u32, n * rows * cols, 112).reshape(n, cols, rows).transpose(0, 2, 1)
    assert len(raw) == 112 + 4 * n * rows * cols
    return head, tuple(geo[:2]), tuple(geo[2:]), [int(v) for v in cnt], words


def test_host_check_counts_nothing(host_check):
    exe, _ = host_check
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2500:])
    assert out.returncode == 0 and out.stdout.rstrip().endswith("inconsistencies: 0")


@pytest.mark.parametrize("shape", K.shapes(), ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_header_on_the_host_equals_the_restatement(host_check, shape):
    exe, d = host_check
    rows, cols, n_layers, res = shape
    g = K.geometry(rows, cols, res)
    layers = K.layers_of((rows, cols), n_layers, rows * 7 + cols)
    mask = (1 << n_layers) - 1
    put_layers(os.path.join(d, "g"), layers)
    for position in K.move_targets(g):
        want, info = K.expect_move(g, layers, position)
        head, length, pos, cnt, words = run(exe, d, ["move"] + geo_args(g, mask) + [repr(position[0]), repr(position[1]), os.path.join(d, "g")])
        assert (head[0], tuple(head[4:6])) == (info["moved"], info["index_shift"]) and pos == want.pos and cnt[0] == info["n_cells_cleared"], position
        assert np.array_equal(words, want.words()), position
    n_fail = 0
    for position, length in K.submap_windows(g):
        want, info = K.expect_submap(g, layers, position, length)
        head, ln, pos, cnt, words = run(exe, d, ["submap"] + geo_args(g, mask) + [repr(v) for v in position + length] + [os.path.join(d, "g")])
        assert head[0] == (want is not None), (position, length)
        if want is None:
            n_fail += 1
            assert head[3] == 0
            continue
        assert (head[1], head[2]) == want.size and ln == want.length and pos == want.pos
        assert tuple(head[4:6]) == info["top_left"] and tuple(head[6:8]) == info["requested"] and np.array_equal(words, want.words())
    assert n_fail >= 3
    for case in K.add_cases(g, n_layers, rows <= 65):
        for extend_only in (False, True):
            want, other, cnt_want = K.expect_add(g, layers, case, extend_only)
            put_layers(os.path.join(d, "o"), [other.data[k] for k in sorted(other.ids)])
            omask = sum(1 << k for k in other.ids)
            ids = case["layer_ids"]
            listed = omask if ids is None else sum(1 << k for k in ids)
            flags = ["1", "0", "0", "0", "0"] if extend_only else [str(int(case["extend"])), "1", str(int(case["overwrite"])), str(listed),
                                                                   str(sum(1 << k for k in case["basic"]))]
            head, ln, pos, cnt, words = run(exe, d, ["add"] + geo_args(g, mask) + geo_args(case["other"], omask) + flags + [os.path.join(d, "g"), os.path.join(d, "o")])
            assert head[0] == cnt_want["resized"] and (head[1], head[2]) == want.size and ln == want.length and pos == want.pos, case
            assert head[3] == sum(1 << k for k in want.ids), case
            if extend_only:
                assert (cnt[1], cnt[4]) == (cnt_want["n_cells_kept"], cnt_want["n_index_outside"]), case
            else:
                assert cnt[2:] == [cnt_want[k] for k in ("n_cells_skipped_valid", "n_cells_outside_other", "n_index_outside", "n_values_copied")], case
            assert np.array_equal(words, want.words(sorted(want.ids))), case
