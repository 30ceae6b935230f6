"""The designed inputs of tests/sor_cases.py do what they claim -- shown on the numpy restatement alone (localmap_restate:
knn_d2, sor_grid, walk), no GPU: the emulated shell walk with the kernel's exit rule is exact on every case, the wrong rules
("no_slack", "one_shell_early", "stop_when_full") fail where a case says they must, the probes end in the shells they were
designed for, the grids do not move with the probes, the threshold brackets are empty, and the points beyond 1e15 m take no
part."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restate as R                                   # noqa: E402
import localmap_restate as L                              # noqa: E402
import sor_cases as S                                     # noqa: E402
from test_localmap_cpu import assert_bracket_empty        # noqa: E402

_WALKS = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def taking_part(name):
    cloud, k, _, note = S.build_case(name)
    ok = np.ones(len(cloud), bool)
    if "bad" in note:
        ok[note["bad"]] = False
    return cloud[ok], k, note, np.cumsum(ok) - 1          # the last: index in the cloud -> index among the participants


def walked(name, rule):
    if (name, rule) not in _WALKS:
        pts, k, _, _ = taking_part(name)
        _WALKS[name, rule] = L.walk(pts, k, rule)
    return _WALKS[name, rule]


def wrong_points(name, rule):
    pts, k, _, _ = taking_part(name)
    return np.nonzero((bits(walked(name, rule)[0]) != bits(L.knn_d2(pts, k + 1))).any(1))[0]


@pytest.mark.parametrize("name", S.WALKED)
def test_the_walk_is_exact_and_the_wrong_rules_are_not(name):
    cloud, k, mul, note = S.build_case(name)
    G = L.sor_grid(cloud, k)
    assert len(cloud) <= 2000
    assert len(wrong_points(name, "real")) == 0
    shells = walked(name, "real")[1]
    hist = dict(zip(*(v.tolist() for v in np.unique(shells, return_counts=True))))
    wrong = {rule: len(wrong_points(name, rule)) for rule in L.WALK_RULES[1:]}
    print(f"  {name}: n {len(cloud)}, mean_k {k}, grid {G['nx']} x {G['ny']} x {G['nz']} edge {G['edge']} occupied {G['occupied']}; "
          f"shells walked {hist}; points a wrong rule gets wrong {wrong}; defeats {[r for r, c in wrong.items() if c]}")
    if note.get("wrong"):
        assert wrong[note["wrong"]] > 0, (name, note["wrong"])


def test_slack_origin_needs_the_slack():
    cloud, k, _, note = S.build_case("slack_origin")
    G = note["grid"]
    print(f"  slack_origin: cells {note['c']} + 1 and + 2 of {G['nx']}: boundaries {note['gap']} apart at edge {note['edge']}, "
          f"closer than nominal by {note['margin']:.3e} relative (the factor 0.99999 absorbs 5e-6)")
    assert note["decides"] and note["margin"] > 5.0e-6 and note["c"] >= 460 and G["nx"] == 501 and G["origin"][0] == -90
    q, P, X = note["q"], note["P"], note["X"]
    cells = R.grid_cells(G, cloud)
    assert np.abs(cells[P] - cells[q]).max() == 2 and np.abs(cells[X] - cells[q]).max() <= 1
    d2 = L.knn_d2(cloud, 2)
    assert d2[q, 1] == S.d2_of(cloud[q], cloud[P]) < S.d2_of(cloud[q], cloud[X])
    assert wrong_points("slack_origin", "no_slack").tolist() == [q]
    assert walked("slack_origin", "no_slack")[0][q, 1] == S.d2_of(cloud[q], cloud[X])       # it answers X ...
    assert walked("slack_origin", "no_slack")[1][q] == 2 and walked("slack_origin", "real")[1][q] == 3   # ... having left before shell 2
    assert same(G, L.sor_grid(cloud, k))


def same(G, H):
    return all(np.array_equal(np.asarray(G[key]), np.asarray(H[key])) for key in G)


@pytest.mark.parametrize("name", ["shell_exit", "shell_exit_mirror"])
def test_shell_exit_probes_end_in_their_shells(name):
    cloud, k, _, note = S.build_case(name)
    d2, shells = walked(name, "real")
    early = wrong_points(name, "one_shell_early")
    per_axis = set()
    for p in note["probes"]:
        q = p["q"]
        assert shells[q] == p["shells"], (p, shells[q])
        dA, dN = S.d2_of(cloud[q], cloud[p["A3"]]), S.d2_of(cloud[q], cloud[p["N"]])
        if note["mirror"]:
            assert dA == S.up(p["T"]) and dN == S.up(p["T"], 2) and d2[q, 3] == dA       # one ulp past the bound: A3 stays, shell r is walked
        else:
            assert dA == p["T"] and dN == S.up(p["T"], -1) and d2[q, 3] == dN             # the largest worst entry that passes; N is the neighbour
        if q in early:
            per_axis.add((p["axis"], p["sign"]))
    print(f"  {name}: 'one_shell_early' is wrong on the probes of the axis directions {sorted(per_axis)}")
    if not note["mirror"]:
        assert per_axis == set(S.AXES)
        assert all(q in early for q in (p["q"] for p in note["probes"] if p["r"] == 3))
    assert same(note["grid"], L.sor_grid(cloud, k))


def test_cell_edges_land_in_the_cells_the_sort_gives_them():
    cloud, k, _, note = S.build_case("cell_edges")
    G = note["grid"]
    assert same(G, L.sor_grid(cloud, k)) and (G["nx"], G["edge"]) == (65, np.float32(0.5))
    cells = R.grid_cells(G, cloud)
    assert cells.min() == 0 and cells.max() == 64                      # the box's maximum: cell nx - 1 by the formula itself, no clamp needed
    d2 = L.knn_d2(cloud, k + 1)
    for g in note["groups"]:
        ids = g["ids"]
        if g["axis"] is not None and len(ids) == 3:
            assert len({int(cells[i, g["axis"]]) for i in ids}) == 2   # the group straddles a boundary ...
        assert (d2[ids, 1] < 1e-9).all()                               # ... and its members are each other's nearest


@pytest.mark.parametrize("name", S.NAMES)
def test_brackets_are_empty_or_the_sign_is_safe(name):
    cloud, k, mul, note = S.build_case(name)
    ref = S.reference(name)
    n = ref["n_finite"]
    if note.get("bracket") != "sign":
        assert ref["rc"] == 0 and math.isfinite(ref["stats"][2])
        assert_bracket_empty(ref, name)
        assert 0 < int(ref["keep"].sum()) < n                          # the threshold decides something
        return
    d = ref["mean_dist"]
    assert len(np.unique(bits(d))) == 1                                # all dist_i are bit-identical
    d = np.float64(d[0])
    err = abs(np.float64(np.float32(d) * np.float32(d)) - d * d)
    print(f"  {name}: d {d!r}, fl32(d d) - d^2 = {np.float64(np.float32(d) * np.float32(d)) - d * d!r}, var {ref['var']!r}, stats {ref['stats']}")
    if name == "equal_spacing_nan":
        assert ref["var"] < 0 and math.isnan(ref["stats"][1]) and math.isnan(ref["stats"][2]) and not ref["keep"].any()
        assert ref["stats"][0] == d == 1.0 + 3.0 * 2.0 ** -12
        assert err * n >= 1000.0 * n * n * 2.0 ** -52 * d * d          # no order of summation can change the sign
    else:
        # d is a small multiple of 2^-4 and n < 2^10: every partial sum of d and of d * d is exact in fp64, in any order
        assert err == 0.0 and d * 16 == int(d * 16) and d < 1 and n < 1024
        assert ref["var"] == 0.0 and ref["stats"] == (d, 0.0, d) and ref["keep"].all() and int(ref["keep"].sum()) == len(cloud)


@pytest.mark.parametrize("name", ["big_coords", "big_coords_edge"])
def test_points_beyond_the_bound_take_no_part(name):
    """The contract (include/liogpu.h lio_sor_filter): a coordinate beyond 1e15 m takes no part -- NaN
    mean_dist, dropped, not counted -- and changes nothing for the others, though it may widen the box."""
    cloud, k, mul, note = S.build_case(name)
    ref, clean = S.reference(name), L.sor(note["clean"], k, mul)
    bad = np.zeros(len(cloud), bool)
    bad[note["bad"]] = True
    assert np.isfinite(cloud).all() and np.array_equal(L.finite_mask(cloud), ~bad) and L.crop_finite_mask(cloud).all()
    assert ref["n_finite"] == clean["n_finite"] == len(cloud) - int(bad.sum())
    assert np.isnan(ref["mean_dist"][bad]).all() and not ref["keep"][bad].any()
    assert np.array_equal(bits(ref["mean_dist"][~bad]), bits(clean["mean_dist"])) and np.array_equal(ref["keep"][~bad], clean["keep"])
    assert ref["stats"] == clean["stats"]
    G, H = L.sor_grid(cloud, k), L.sor_grid(note["clean"], k)
    if name == "big_coords":
        assert G["origin"][2] == -11 and H["origin"][2] > -2 and G["nz"] > H["nz"]          # the record that takes no part widened the box
    else:
        assert same(G, H) and (G["nx"], G["ny"], G["nz"]) == (501, 1, 1)                   # the edge at its clamp ext / 500
        shells = walked(name, "real")[1]
        far = taking_part(name)[3][note["far"]]
        assert shells[far] == 501 and (np.delete(shells, far) == 2).all() and not ref["keep"][note["far"]]


def test_named_geometries_are_what_they_say():
    G = L.sor_grid(S.build_case("long_thin")[0], 10)
    assert (G["nx"], G["ny"], G["nz"]) == (118, 1, 1)
    for name in ("one_cell_tiny", "one_cell_copies"):
        G = L.sor_grid(S.build_case(name)[0], 10)
        assert (G["n_cells"], G["occupied"], G["edge"]) == (1, -1, 1.0)
    assert S.reference("one_cell_copies")["stats"] == (0.0, 0.0, 0.0)
    for name in ("crowded_cells_k32", "crowded_cells_k1"):
        shells = walked(name, "real")[1]
        assert (shells == 2).sum() >= 900 and shells.max() >= 20, shells.max()
    cloud, k, _, _ = S.build_case("far_offset")
    assert np.abs(cloud[:, :2]).min() > 2.9e5 and np.spacing(cloud[:, 0]).min() >= 0.03
    n = len(S.build_case("wg_257")[0])
    assert n == 257 * 256 + 1 and (n + 255) // 256 == 258 and n >= 65537
    # the lattice: interior points hold 6 neighbours at 0.5 and tie beyond
    d2 = L.knn_d2(S.build_case("lattice_ties_k10")[0], 20)
    inner = (d2[:, 1] == 0.25) & (d2[:, 6] == 0.25) & (d2[:, 7] == 0.5)
    assert inner.sum() >= 330 and (d2[inner][:, 7:19] == 0.5).all()


@pytest.mark.parametrize("name", S.WALKED)
def test_fast_knn_is_the_brute_force(name):
    """Where equal distances keep the candidates from separating, knn_d2_fast refuses (it never guesses) and is asked again
    with more candidates; what it answers is the brute force bit for bit."""
    pts, k, _, _ = taking_part(name)
    for extra in (8, 40, len(pts)):                       # (all points as candidates: nothing left to separate from)
        try:
            fast = L.knn_d2_fast(pts, k + 1, extra)
            break
        except ValueError:
            assert extra < len(pts), name
    print(f"  {name}: knn_d2_fast answered with k + {extra} candidates")
    assert np.array_equal(bits(fast), bits(L.knn_d2(pts, k + 1))), name


def test_fast_knn_on_the_size_case_and_a_sample_of_it():
    cloud, k, _, _ = S.build_case("wg_257")
    ref = S.reference("wg_257")
    rows = np.random.default_rng(0).integers(0, len(cloud), 600)
    p = cloud[:, :3]
    dx, dy, dz = p[rows, None, 0] - p[None, :, 0], p[rows, None, 1] - p[None, :, 1], p[rows, None, 2] - p[None, :, 2]
    d2 = np.sort(((dx * dx) + dy * dy) + dz * dz, axis=1)[:, :2]
    want = np.sqrt(d2[:, 1]).astype(np.float64).astype(np.float32)
    assert np.array_equal(bits(ref["mean_dist"][rows]), bits(want))
    with pytest.raises(ValueError):                                     # the condition is asserted, not assumed
        L.knn_d2_fast(np.zeros((50, 3), np.float32), 2)


def test_grid_of_default_is_the_alignments_grid():
    """grid_of gained per_cell; its default must give the bits tests/test_icp_cases_cpu.py pins, and 4 is 4."""
    import icp_cases
    for name in ("cell_edges", "slack_origin", "far_long"):
        tgt = icp_cases.build_case(name)[1]
        assert same(R.grid_of(tgt), R.grid_of(tgt, np.float32(4.0)))
    tgt = icp_cases.build_case("cell_edges")[1]
    G = R.grid_of(tgt)
    assert (G["edge"], G["inv_cell"], G["nx"], G["occupied"]) == (1.0, 1.0, 33, len(tgt))
    assert not same(G, R.grid_of(tgt, L.sor_per_cell(10))) and L.sor_per_cell(10) == np.float32(11) / np.float32(3)
    empty = L.sor_grid(np.full((3, 3), np.nan, np.float32), 10)
    assert (empty["n_cells"], empty["occupied"], empty["edge"]) == (1, -1, 1.0) and not empty["origin"].any()


def test_the_hook_refuses_what_the_filter_refuses(pkg):
    import ctypes as C
    lib = pkg.load_library()
    pts = np.zeros((16, 8), np.float32)
    out = pkg.IcpGridInfo()
    fn = lib.lio_sor_debug_grid
    for k in (0, 33, -1):
        assert fn(0, pts.ctypes.data, 16, 32, k, C.byref(out)) == -1                       # LIO_ERR_ARG before any device
    assert fn(0, pts.ctypes.data, 16, 10, 10, C.byref(out)) == -1 and fn(0, pts.ctypes.data, 16, 32, 10, None) == -1
    assert fn(0, None, 16, 32, 10, C.byref(out)) == -1
    # no device, no fallback: without one the hook answers LIO_ERR_NO_DEVICE exactly where the filter does
    try:
        pkg.sor_filter(pts[:, :4], 10, 1.0)
    except pkg.LioError as err:
        assert "ERR_NO_DEVICE" in str(err)
        with pytest.raises(pkg.LioError, match="ERR_NO_DEVICE"):
            pkg.sor_debug_grid(pts, 10)
        assert fn(0, pts.ctypes.data, 16, 32, 10, C.byref(out)) == -5 and fn(0, None, 0, 32, 10, C.byref(out)) == -5
        return
    G = pkg.sor_debug_grid(pts, 10)
    assert (G.n_cells, G.occupied, G.edge, G.any) == (1, -1, 1.0, 1)
