"""The planning local map, the part that needs no GPU: the numpy restatement (tests/localmap_restate.py) against scipy and
closed forms, the inputs of the device tests (their threshold brackets must be empty), the ABI structs and defaults, refused
arguments."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_restate as L                              # noqa: E402
from test_icp_cpu import street_loop_case                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def xyzi(xyz, rng=None):
    xyz = np.asarray(xyz, np.float32)
    w = np.zeros((len(xyz), 1), np.float32) if rng is None else rng.uniform(0, 255, (len(xyz), 1)).astype(np.float32)
    return np.concatenate([xyz[:, :3], w], 1)


def loop_case(synth, oracle, kind):
    if kind not in _CACHE:
        _CACHE[kind] = street_loop_case(synth, oracle) if kind == "street" else street_loop_case(synth, oracle, kind="corridor", seed=5)
    return _CACHE[kind]


def sor_cases(synth, oracle):
    """name -> (cloud [n, 4], mean_k): the inputs of the device tests of lio_sor_filter, the smallest at which the kernel can
    go wrong.  Built once."""
    if "sor" in _CACHE:
        return _CACHE["sor"]
    rng = np.random.default_rng(21)
    cases = {}
    cases["street"] = (xyzi(loop_case(synth, oracle, "street")["tgt"], rng), 10)          # VLP-16 submaps at leaf 0.4: 15 k points
    cases["corridor"] = (xyzi(loop_case(synth, oracle, "corridor")["src"], rng), 10)      # ... and 5 k
    for n in (257, 513):                                                                   # workgroup boundaries
        pts = xyzi(rng.uniform(-6, 6, (n, 3)) * np.array([1, 1, 0.2]), rng)
        for k in (1, 10, 32):
            cases[f"n{n}_k{k}"] = (pts, k)
    body = rng.uniform(-10, 10, (3000, 3)) * np.array([1, 1, 0.1])
    d = rng.normal(size=(20, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(100, 1000, (20, 1))   # many shells, clipped at the grid
    pts = np.concatenate([body, far], 0)
    cases["isolated"] = (xyzi(pts[rng.permutation(len(pts))], rng), 10)
    half = rng.uniform(-8, 8, (1200, 3)) * np.array([1, 1, 0.15])
    cases["duplicated"] = (xyzi(np.concatenate([half, half], 0)[rng.permutation(2400)], rng), 10)
    flat = rng.uniform(-15, 15, (2000, 3))
    flat[:, 2] = 1.25                                                                      # the grid is one cell thick
    cases["planar"] = (xyzi(flat, rng), 10)
    small = xyzi(rng.uniform(-2, 2, (11, 3)), rng)
    cases["k_plus_1"] = (small, 10)
    cases["k_points"] = (small[:10], 10)
    cases["empty"] = (small[:0], 10)
    good = xyzi(rng.uniform(-8, 8, (2000, 3)) * np.array([1, 1, 0.2]), rng)
    mixed = np.zeros((3000, 4), np.float32)                                               # every third record spoiled
    mixed[0::3], mixed[1::3] = good[:1000], good[1000:]
    spoil = good[:1000].copy()
    spoil[0::3, 0] = np.nan; spoil[1::3, 1] = np.inf; spoil[2::3, 2] = -np.inf
    mixed[2::3] = spoil
    cases["nonfinite"] = (mixed, 10)
    cases["nonfinite_clean"] = (mixed[np.isfinite(mixed[:, :3]).all(1)], 10)
    _CACHE["sor"] = cases
    return cases


def sor_reference(synth, oracle, name):
    """The restatement's answer for one case, computed once."""
    key = ("ref", name)
    if key not in _CACHE:
        pts, k = sor_cases(synth, oracle)[name]
        _CACHE[key] = L.sor(pts, k, 1.0)
    return _CACHE[key]


def assert_bracket_empty(ref, what):
    if ref["rc"] != 0:
        return
    thr = ref["stats"][2]
    d = ref["mean_dist"][np.isfinite(ref["mean_dist"])].astype(np.float64)
    gap = np.abs(d - thr).min()
    assert gap > L.bracket(thr, ref["n_finite"]), (what, gap, L.bracket(thr, ref["n_finite"]))


def test_mean_distances_are_the_kdtree_ones():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(1)
    pts = (rng.uniform(-10, 10, (2000, 3)) * np.array([1, 1, 0.2])).astype(np.float32)
    for k in (1, 10, 32):
        d = L.mean_distances(pts, k)
        dk, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=k + 1)
        ref = dk[:, 1:].sum(1) / k
        assert np.abs(d.astype(np.float64) - ref).max() <= 1e-6 * ref.max()
        assert (np.abs(d.astype(np.float64) - ref) / ref).max() <= 1e-6


def test_lattice_loses_only_its_far_point():
    g = np.stack(np.meshgrid(*[np.arange(10.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([g[:500], [[50.0, 4.0, 4.0]], g[500:]], 0).astype(np.float32)
    r = L.sor(pts, 10, 1.0)
    assert r["rc"] == 0 and r["n_finite"] == 1001
    assert np.array_equal(np.nonzero(~r["keep"])[0], [500])
    inner = r["mean_dist"][np.all((pts > 0.5) & (pts < 8.5), 1)]
    assert np.allclose(inner, (6 + 4 * math.sqrt(2.0)) / 10, rtol=1e-6)      # six at 1, then four of the twelve at sqrt 2
    assert r["mean_dist"][500] > 40.0


def test_duplicates_count_as_neighbours_at_distance_zero():
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]] * 2, np.float32)
    r = L.sor(pts, 2, 1.0)
    assert r["rc"] == 0
    assert np.array_equal(r["mean_dist"], np.array([0.5, 0.5, 1.0] * 2, np.float32))       # (0 + 1) / 2, (0 + 1) / 2, (0 + 2) / 2
    # the answer is a function of the multiset of distances: any order of the same records gives the same per-point values
    perm = np.array([3, 0, 5, 1, 4, 2])
    assert np.array_equal(L.sor(pts[perm], 2, 1.0)["mean_dist"], r["mean_dist"][perm])


def test_size_limits_and_non_finite_points():
    rng = np.random.default_rng(2)
    pts = rng.uniform(-2, 2, (11, 3)).astype(np.float32)
    r = L.sor(pts, 10, 1.0)
    assert r["rc"] == 0 and r["n_finite"] == 11 and np.isfinite(r["stats"][2])
    ref = np.sqrt(np.sort(((pts[:, None] - pts[None]) ** 2).sum(-1).astype(np.float64), 1)[:, 1:]).mean(1)
    assert np.allclose(r["mean_dist"], ref, rtol=1e-6)
    p = L.sor(pts[:10], 10, 1.0)
    assert p["rc"] == 1 and p["keep"].all() and p["stats"] == (0.0, 0.0, math.inf) and not p["mean_dist"].any()
    e = L.sor(pts[:0], 10, 1.0)
    assert e["rc"] == 1 and len(e["keep"]) == 0
    bad = np.concatenate([pts, [[np.nan, 0, 0], [0, np.inf, 0]]], 0).astype(np.float32)
    b = L.sor(bad, 10, 1.0)
    assert b["rc"] == 0 and np.array_equal(b["mean_dist"][:11], r["mean_dist"]) and np.isnan(b["mean_dist"][11:]).all()
    assert not b["keep"][11:].any() and np.array_equal(b["keep"][:11], r["keep"]) and b["stats"] == r["stats"]
    for k, m in ((0, 1.0), (33, 1.0), (10, float("nan"))):
        with pytest.raises(ValueError):
            L.sor(pts, k, m)


def test_crop_keeps_its_four_limits():
    pose = np.zeros(6, np.float32)
    up, dn = lambda v: np.nextafter(np.float32(v), np.float32(np.inf)), lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    pts = np.array([[40, 0, 1, 7], [up(40), 0, 1, 7], [-40, 0, 1, 7], [dn(-40), 0, 1, 7],
                    [0, 70, 1, 7], [0, up(70), 1, 7], [0, -20, 1, 7], [0, dn(-20), 1, 7], [np.nan, 0, 0, 7]], np.float32)
    out, keep = L.crop(pts, pose)
    assert keep.tolist() == [True, False] * 4 + [False]
    assert np.array_equal(out, pts[keep])                                       # the zero pose moves nothing
    # a quarter turn to the left about a vehicle at (10, 5, 2): world +y is the vehicle's +x
    pose = np.array([0.3, -0.2, math.pi / 2, 10, 5, 2], np.float32)
    out, keep = L.crop(np.array([[10, 45, 2, 1], [10, 46, 2, 1], [-60, 5, 2, 1], [-61, 5, 2, 1]], np.float32), pose)
    assert keep.tolist() == [True, False, True, False]
    assert np.allclose(out[:, :3], [[40, 0, 0], [0, 70, 0]], atol=1e-4) and np.array_equal(out[:, 3], [1, 1])


def test_device_test_inputs_leave_the_bracket_empty(synth, oracle):
    """tests/test_gpu_localmap.py compares kept index sets outside |dist - thr| <= 64 n 2^-52 thr; for its inputs nothing is
    inside, so the sets must be equal."""
    sizes = {}
    for name in sor_cases(synth, oracle):
        ref = sor_reference(synth, oracle, name)
        assert_bracket_empty(ref, name)
        sizes[name] = (ref["n_finite"], int(ref["keep"].sum()))
    print("device test inputs (finite points, inliers):", sizes)
    assert sizes["isolated"] == (3020, 3000) and sizes["street"][0] > 3000 and sizes["corridor"][0] > 3000
    a, b = sor_reference(synth, oracle, "nonfinite"), sor_reference(synth, oracle, "nonfinite_clean")
    fin = np.isfinite(a["mean_dist"])
    assert np.array_equal(a["mean_dist"][fin], b["mean_dist"]) and a["stats"] == b["stats"]


def test_struct_layouts_and_defaults(pkg):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "liogpu.h"
    int main(void) {
        printf("%zu %zu\n", sizeof(lio_local_map_config), sizeof(lio_local_map_info));
        printf("%zu %zu %zu\n", offsetof(lio_local_map_config, right), offsetof(lio_local_map_config, stddev_mul), offsetof(lio_local_map_config, leaf));
        printf("%zu %zu %zu\n", offsetof(lio_local_map_info, n_inliers), offsetof(lio_local_map_info, voxel_passthrough), offsetof(lio_local_map_info, sor_threshold));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        v = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    cfg, info = pkg.LocalMapConfig, pkg.LocalMapInfo
    assert v == [C.sizeof(cfg), C.sizeof(info), cfg.right.offset, cfg.stddev_mul.offset, cfg.leaf.offset,
                 info.n_inliers.offset, info.voxel_passthrough.offset, info.sor_threshold.offset]
    c = pkg.local_map_default_config()
    got = {k: getattr(c, k) for k in L.DEFAULTS}
    assert got == L.DEFAULTS and got["leaf"] == np.float32(0.01)               # UT:219-229


def test_bad_arguments_are_refused_before_any_device(pkg):
    lib = pkg.load_library()
    pts = np.zeros((16, 8), np.float32)
    n_out = C.c_size_t()
    for k, m in ((0, 1.0), (33, 1.0), (-1, 1.0), (10, float("nan")), (10, float("inf"))):
        assert lib.lio_sor_filter(0, pts.ctypes.data, 16, 32, k, m, pts.ctypes.data, 32, C.byref(n_out), None, None) == -1, (k, m)
    assert lib.lio_sor_filter(0, pts.ctypes.data, 16, 10, 10, 1.0, pts.ctypes.data, 32, C.byref(n_out), None, None) == -1
    assert lib.lio_sor_filter(0, pts.ctypes.data, 16, 32, 10, 1.0, pts.ctypes.data, 32, None, None, None) == -1
    assert lib.lio_sor_filter(0, None, 0, 32, 10, 1.0, None, 32, C.byref(n_out), None, None) == 1 and n_out.value == 0     # the empty cloud
    pose = np.zeros(6, np.float32)
    cfg = pkg.local_map_default_config()
    assert lib.lio_kf_store_local_map(None, C.byref(cfg), pose.ctypes.data_as(C.POINTER(C.c_float)), None, 32, 0, C.byref(n_out), None) == -1
