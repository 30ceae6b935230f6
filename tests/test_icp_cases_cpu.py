"""The designed ICP cases (tests/icp_cases.py) hit what they name -- proved on the restatement alone (icp_restate, grid_of),
no GPU: tie multiplicities, the shells of winner and runner-up, the side of the gate, the cells on both sides of a cell
boundary, the iteration at which the pairs run out, the rank of a degenerate covariance.  tests/test_gpu_icp_edges.py then
runs the same cases on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC   # noqa: E402
import icp_restate as R   # noqa: E402

F = np.float32


def d2_all(q, tgt):
    """fp32 squared distances of one query to every target point, FLANN's order of operations"""
    d = np.asarray(q, F)[None, :] - np.asarray(tgt, F)
    with np.errstate(over="ignore"):
        return ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def shells(G, q, pts):
    """Chebyshev distance, in cells, of the points' cells from the query's cell"""
    cq = R.grid_cells(G, np.asarray(q, F)[None, :])[0]
    return np.abs(R.grid_cells(G, pts) - cq[None, :]).max(1).astype(int)


def start(src, guess):
    return R.transform_points(np.eye(4, dtype=F) if guess is None else guess, src)


def cfg_of(over):
    return dict(R.DEFAULTS, **{k: v for k, v in over.items() if k in R.DEFAULTS})


def test_every_case_is_small_seeded_and_framed_as_said():
    for name in IC.NAMES:
        src, tgt, over, guess, note = IC.build_case(name)
        src2, tgt2, _, _, _ = IC.build_case(name)
        assert np.array_equal(src.view(np.uint32), src2.view(np.uint32)) and np.array_equal(tgt.view(np.uint32), tgt2.view(np.uint32)), name
        assert len(tgt) <= 5000 and len(src) <= 1100 and over["max_iters"] <= 6, name
        if note.get("edge") is not None:
            G = R.grid_of(tgt)
            assert (G["edge"], G["inv_cell"], G["nx"], G["ny"], G["nz"]) == (F(note["edge"]), F(1.0), 33, 33, 33), (name, G)


def test_nn_brute_is_the_kdtree_on_every_untied_probe():
    from scipy.spatial import cKDTree
    for name in IC.NAMES:
        src, tgt, over, guess, note = IC.build_case(name)
        if note.get("what") == "big_coords":
            src = src[:-note["n_bad_src"]]                    # (sources up to FLT_MAX: their squared distances overflow, no tree orders them)
        cur = start(src, guess)
        idx, d2 = R.nn_brute(cur, tgt)
        ok = R.target_ok(tgt)
        ids = np.nonzero(ok)[0]
        dk, ik = cKDTree(tgt[ok].astype(np.float64)).query(cur.astype(np.float64), k=min(2, len(ids)))
        dk, ik = dk.reshape(len(cur), -1), ik.reshape(len(cur), -1)
        untied = np.ones(len(cur), bool) if dk.shape[1] < 2 else (dk[:, 1] - dk[:, 0] > 1e-5 * np.maximum(dk[:, 1], 1e-3))
        assert np.array_equal(idx[untied], ids[ik[untied, 0]]), name
        assert untied.any() or note.get("what") in ("ties", "one_point") or note.get("rank") == 0, name       # (targets made of repeated points)


@pytest.mark.parametrize("name", ["lattice_ties", "far_lattice"])
def test_ties(name):
    src, tgt, over, guess, note = IC.build_case(name)
    G = R.grid_of(tgt)
    idx, d2 = R.nn_brute(src, tgt)
    multi_shell = not_first = 0
    seen = set()
    for i, q in enumerate(src):
        d = d2_all(q, tgt)
        tied = np.nonzero(d == d.min())[0]
        assert len(tied) == note["multiplicity"][i], (i, len(tied))
        assert idx[i] == tied.min()
        sh = shells(G, q, tgt[tied])
        cells = R.grid_cells(G, tgt[tied])
        if len(np.unique(cells, axis=0)) > 1:
            seen.add(len(tied))
        multi_shell += len(set(sh)) > 1
        # the walk visits shells outwards, within a shell z, then y, then x: is the lowest index met first?
        order = sorted(range(len(tied)), key=lambda j: (sh[j], cells[j][2], cells[j][1], cells[j][0], tied[j]))
        not_first += tied[order[0]] != tied.min()
    print(f"{name}: {multi_shell} queries whose tied points lie in different shells, {not_first} whose lowest index is not the first met")
    assert multi_shell >= note["min_multi_shell"] and not_first >= 100 and {2, 4, 8} <= seen


@pytest.mark.parametrize("name", ["cell_edges", "far_edges"])
def test_cell_edges(name):
    src, tgt, over, guess, note = IC.build_case(name)
    G = R.grid_of(tgt)
    assert np.array_equal(G["origin"].astype(np.float64), note["origin"])
    cells = R.grid_cells(G, src)
    idx, d2 = R.nn_brute(src, tgt)
    seen = {}
    for p in note["probes"]:
        i = p["src"]
        want = p["k"] - 1 if p["ulp"] < 0 else p["k"]
        for a in p["axes"]:
            assert cells[i, a] == want, (p, cells[i])
        sh = shells(G, src[i], tgt[[idx[i]]])[0]
        d = float(np.sqrt(np.float64(d2[i])))
        print(f"{name} probe k={p['k']} ulp {p['ulp']:+d} axes {p['axes']}: cell {cells[i].astype(int).tolist()}, nearest {idx[i]} in shell {sh} at {d:.6f}")
        assert idx[i] >= note["n_frame"]
        seen.setdefault(int(idx[i]), {})[p["ulp"]] = sh
        if len(p["axes"]) == 1:
            assert abs(d - 1.0) <= 2.0 ** -9 + 2.0 ** -5 * (name == "far_edges")
    for t, sh in seen.items():
        # the three probes of one boundary share their nearest point; across the boundary it moves by one shell, and on one
        # side or the other it lies in a neighbouring cell
        assert set(sh) == {-1, 0, 1} and abs(sh[-1] - sh[0]) == 1 and sh[0] == sh[1] and max(sh.values()) >= 1, (t, sh)
    assert len(seen) == 21
    sides = {(p["k"], p["ulp"]) for p in note["probes"]}
    assert sides == {(k, u) for k in (0, 16, 33) for u in (-1, 0, 1)}


@pytest.mark.parametrize("name", ["shell_exit", "shell_exit_mirror"])
def test_shell_exit(name):
    src, tgt, over, guess, note = IC.build_case(name)
    G = R.grid_of(tgt)
    e = float(G["edge"])
    for p in note["probes"]:
        q = src[p["src"]]
        d = d2_all(q, tgt)
        rank = np.argsort(d, kind="stable")
        sh = shells(G, q, tgt[[p["A"], p["B"], p["C"]]])
        print(f"{name} r={p['r']} axis {p['axis']} sign {p['sign']:+d}: d2 A {d[p['A']]!r} (shell {sh[0]}), B {d[p['B']]!r} (shell {sh[1]}), C {d[p['C']]!r} (shell {sh[2]})")
        assert rank[0] == p["C"] and d[rank[0]] < d[rank[1]]
        if note["mirror"]:
            assert sh[2] <= 1 and np.sqrt(d[p["C"]]) < (sh[1] - 1) * e * 0.99          # the walk may stop before B's shell
        else:
            assert list(rank[:3]) == [p["C"], p["B"], p["A"]] and d[rank[2]] < d[rank[3]]
            assert list(sh) == [p["r"], p["r"] + 1, p["r"] + 2]
    assert {(p["r"], p["axis"], p["sign"]) for p in note["probes"]} == {(r, a, s) for r in (1, 2, 3) for a in range(3) for s in (1, -1)}
    for p in note["slack"]:
        q = src[p["src"]]
        d = d2_all(q, tgt)
        rank = np.argsort(d, kind="stable")
        sh = shells(G, q, tgt[[p["X"], p["P"]]])
        print(f"{name} slack probe sign {p['sign']:+d}: d X {np.sqrt(d[p['X']])!r} (shell {sh[0]}), d P {np.sqrt(d[p['P']])!r} (shell {sh[1]})")
        if not note["mirror"]:
            # P, the nearest, is in shell 2 and X, the best of the earlier shells, lies within e + 1e-3 e: a bound of e PLUS the slack would stop the walk
            assert list(rank[:2]) == [p["P"], p["X"]] and sh[0] <= 1 and sh[1] == 2
            assert e < np.sqrt(d[p["P"]]) < np.sqrt(d[p["X"]]) < e * (1 + 1.0e-3) * np.sqrt(0.99999)


def test_slack_origin():
    """The case that needs the slack: p in shell 2 is the nearest, X in an earlier shell is at most sqrt(0.99999) e away."""
    src, tgt, over, guess, note = IC.build_case("slack_origin")
    G = R.grid_of(tgt)
    e = G["edge"]
    assert G["origin"][0] == -1000.0 and tgt[:, 0].max() == 1000.0
    q = src[note["src"]]
    d = d2_all(q, tgt)
    rank = np.argsort(d, kind="stable")
    sh = shells(G, q, tgt[[note["P"], note["X"]]])
    lim = F(F(e * e) * F(0.99999))                            # the exit's left side at r = 2 when the slack is 0: lb = (r - 1) e
    print(f"slack_origin: e {e!r}, x cell {note['c']}, boundary gap {note['gap']!r} = {note['gap'] / float(e):.7f} e; d2 P {d[note['P']]!r} (shell {sh[0]}), "
          f"d2 X {d[note['X']]!r} (shell {sh[1]}), e^2 * 0.99999f = {lim!r}; third nearest d2 {d[rank[2]]!r}")
    assert list(rank[:2]) == [note["P"], note["X"]] and R.nn_brute(q[None, :], tgt)[0][0] == note["P"]
    assert (sh[0], sh[1]) == (note["r"], 0)
    assert d[note["P"]] < d[note["X"]] <= lim                 # the bound (r - 1) e alone, even times 0.99999, would stop the walk at X
    assert np.sqrt(np.float64(d[note["P"]])) < float(e) * np.sqrt(0.99999)
    slack = F(1.0e-3) * e + F(1.0e-5) * F(q[0] - G["origin"][0])
    lb = F(e - slack)
    assert F(F(lb * lb) * F(0.99999)) < d[note["P"]]          # with the slack the walk goes on into shell 2


@pytest.mark.parametrize("name", ["gate_edge_half", "gate_edge_odd"])
def test_gate_edge(name):
    src, tgt, over, guess, note = IC.build_case(name)
    g2 = np.float64(over["max_corr_dist"]) ** 2
    idx, d2 = R.nn_brute(src, tgt)
    corr, _, n = R.correspondences(src, tgt, cfg_of(over))
    G = R.grid_of(tgt)
    for p in note["probes"]:
        i = p["src"]
        print(f"{name}: side {p['side']:+d} d2 {d2[i]!r} = {float(d2[i]).hex()} against gate^2 {g2!r} = {float(g2).hex()}, shell {shells(G, src[i], tgt[[idx[i]]])[0]}")
        assert idx[i] == p["tgt"]
        assert d2[i] == [np.nextafter(F(note["at"]), F(0)), F(note["at"]), np.nextafter(F(note["at"]), F(np.inf))][p["side"] + 1]
        assert (np.float64(d2[i]) <= g2) == (p["side"] <= 0) == (corr[i] >= 0)
    assert len(note["probes"]) == 9 and n == 6 and "reach" in note["beyond_reach"]
    assert (np.float64(F(note["at"])) == g2) == (name == "gate_edge_half")           # 0.25 is a float; 1.3^2 is not


@pytest.mark.parametrize("name", ["outside_wide", "outside_tight"])
def test_outside(name):
    src, tgt, over, guess, note = IC.build_case(name)
    G = R.grid_of(tgt)
    c = R.grid_cells(G, src[:note["n_out"]])
    out = np.maximum(np.maximum(-c, c - 32), 0).max(1)
    assert sorted(set(out.astype(int))) == [1, 10, 1000] and len(out) == 26 * 3
    dirs = {tuple(np.sign(np.where(cc < 0, -1, np.where(cc > 32, 1, 0))).astype(int)) for cc in c}
    assert len(dirs) == 26                                   # 6 faces, 12 edges, 8 corners
    corr, _, n = R.correspondences(src, tgt, cfg_of(over))
    assert n == (len(src) if note["wide"] else len(src) - note["n_out"])


def test_clamp_flat_far_and_big():
    src, tgt, over, guess, note = IC.build_case("clamp_tiny")
    G = R.grid_of(tgt)
    c = R.grid_cells(G, src)
    assert (np.abs(c[:note["n_far"]]).max(1) > note["min_cell"]).all() and G["edge"] < 1e-5
    assert (np.abs(c[note["n_far"]:]).max(1) < 100).all()
    for name in ("clamp_one_point", "clamp_repeated"):
        src, tgt, over, guess, note = IC.build_case(name)
        G = R.grid_of(tgt)
        assert (G["nx"], G["ny"], G["nz"], G["occupied"], G["edge"]) == (1, 1, 1, -1, F(1.0)) and len(tgt) == note["n_tgt"]
        assert (R.nn_brute(src, tgt)[0] == 0).all()
    dims = {"flat_plane": lambda G: G["nz"] == 1 and G["nx"] > 1 and G["ny"] > 1, "flat_line": lambda G: G["ny"] == G["nz"] == 1 and G["nx"] > 100,
            "flat_tilted": lambda G: min(G["nx"], G["ny"], G["nz"]) > 1}
    for name, ok in dims.items():
        src, tgt, over, guess, note = IC.build_case(name)
        G = R.grid_of(tgt)
        assert ok(G), (name, G)
        idx, _ = R.nn_brute(src, tgt)
        side = np.sign((src - tgt[idx])[:, 2])
        assert (side > 0).sum() > 50 and (side < 0).sum() > 50                         # sources off the surface on both sides
        if name == "flat_tilted":                                                      # one cell thick almost everywhere
            c = R.grid_cells(G, tgt)
            cols = {}
            for x, y, z in c.astype(int):
                cols.setdefault((x, y), set()).add(z)
            assert np.mean([len(v) == 1 for v in cols.values()]) > 0.6
    src, tgt, over, guess, note = IC.build_case("far_long")
    G = R.grid_of(tgt)
    assert tgt[:, 0].max() - tgt[:, 0].min() == 4000.0 and G["nx"] > 200 and src[:, 0].min() > 3000.0
    src, tgt, over, guess, note = IC.build_case("big_coords")
    ok = R.target_ok(tgt)
    assert list(np.nonzero(~ok)[0]) == note["bad_tgt"] and ok[note["in_range_tgt"]]
    assert np.isfinite(tgt).all() and np.isfinite(src).all()
    idx, d2 = R.nn_brute(src, tgt)
    corr, _, n = R.correspondences(src, tgt, cfg_of(over))
    assert not np.isin(idx, note["bad_tgt"]).any() and n == len(src) - note["n_bad_src"]
    # with the plain isfinite rule the out-of-range target points would take part: they are finite
    assert R.target_ok(tgt).sum() == len(tgt) - len(note["bad_tgt"]) < np.isfinite(tgt).all(1).sum()
    d2_bad = d2[-note["n_bad_src"]:]
    assert np.isinf(d2_bad).sum() >= 2 and np.isfinite(d2_bad).sum() >= 2 and (corr[-note["n_bad_src"]:] == -1).all()


def test_workgroup_bounds_guess_and_criteria():
    for n in IC.WG_SIZES:
        src, tgt, over, guess, note = IC.build_case(f"wg_{n}")
        assert len(src) == n
        _, d2 = R.nn_brute(src, tgt)
        m = np.zeros(n, bool)
        m[note["marked"]] = True
        assert note["marked"] and (d2[m].astype(np.float64) <= over["max_corr_dist"] ** 2).all()
        if (~m).any():
            assert d2[m].min() > d2[~m].max(), n               # the marked lanes carry the largest residuals
    assert n - 1 in note["marked"] and 256 in note["marked"] and 512 in note["marked"]
    for name in ("guess_skew", "guess_answer"):
        src, tgt, over, guess, note = IC.build_case(name)
        r = R.icp(src, tgt, cfg_of(over), guess)
        r0 = R.icp(src, tgt, cfg_of(over))
        assert not np.array_equal(guess, np.eye(4)) and r["converged"] == 1 and r["fitness"] < 1e-3 < r0["fitness"], name
        assert r["iters"] == (1 if name == "guess_answer" else r["iters"]) and (name == "guess_answer" or r["iters"] >= 3)
    for name in IC.NAMES:
        src, tgt, over, guess, note = IC.build_case(name)
        if note.get("what") != "criteria":
            continue
        r = R.icp(src, tgt, cfg_of(over), guess)
        print(f"{name}: state {r['state']} iters {r['iters']} n_corr {r['n_corr']} mse {r['mse']}")
        if "state" in note:
            assert r["state"] == note["state"], name
        if "iters" in note:
            assert r["iters"] == note["iters"], name
        if note["kind"] in ("similar1", "similar3", "reset"):
            plain = R.icp(src, tgt, dict(cfg_of(over), max_similar=0), guess)
            assert plain["iters"] < r["iters"]                 # the counter delayed the end
        if note["kind"] == "zero_mse":
            assert r["mse"][:2] == [0.0, 0.0] and over["max_similar"] == 2
        if note["kind"] == "drop":
            assert r["n_corr"] == note["n_corr"] and (r["state"], r["converged"], r["iters"]) == (R.NO_CORRESPONDENCES, 0, note["drop_at"])
            assert r["n_corr"][note["drop_at"]] < over["min_corr"] <= min(r["n_corr"][:note["drop_at"]])


def test_degenerate_ranks():
    for name in IC.NAMES:
        src, tgt, over, guess, note = IC.build_case(name)
        if "rank" not in note and note.get("what") != "reflection":
            continue
        corr, _, n = R.correspondences(src, tgt, cfg_of(over))
        s, t = src[corr >= 0].astype(np.float64), tgt[corr[corr >= 0]].astype(np.float64)
        cov = (t - t.mean(0)).T @ (s - s.mean(0)) / len(s)
        sv = np.linalg.svd(cov, compute_uv=False)
        ratios = sv / sv[0] if sv[0] > 0 else sv
        print(f"{name}: {n} pairs, singular values {sv}, ratios {ratios}")
        if note.get("what") == "reflection":
            assert ratios[2] > 1e-6 and np.linalg.det(cov) < 0 and R.umeyama_step(s, t)[1]
            continue
        rank = note["rank"]
        assert int((ratios > 1e-12).sum()) == rank and (rank == 0 or ratios[rank - 1] > 1e-4), (name, ratios)
        if rank == 2:                                        # mirrored in the plane: the in-plane block of the covariance has a negative determinant
            assert cov[0, 0] * cov[1, 1] - cov[0, 1] * cov[1, 0] < 0
