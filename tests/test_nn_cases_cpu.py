"""The case builders of tests/nn_cases.py checked on the CPU: `grid_of` gives the constants lio_gridplan.h documents and, field
for field and bit for bit, the plan the library itself lays out (lio_plan_grid and lio_plan_tables through the host-only hook
lio_debug_grid_plan: every case under every handle setting of the GPU test, the size caps, the long-map thresholds, the
caller's-box path, the environment overrides), every
built case really has the ties and edges it claims (under the oracle's brute-force and kd-tree searches, which must agree),
and the emulation of lio_cell_coord pins the long-map rule: two-cell misses exist without it on a strip of 8200 m, none
with it at any extent from 100 m to 70 km.  The miss counts come from that emulation, not from hardware.  "Half of the slack" is
an empirical margin, not a bound: the four roundings of a cell difference (two subtractions, two products) can add up to about
2.8 spacings of the extent in the worst case, 1.4 times the slack where slack / 2 lies just above a power of two -- the sweep
includes such a gate (0.55: the 0.15 table's threshold falls at 1016 m with spacing / slack = 0.499) and finds nothing there
either."""
import importlib
import os

import numpy as np
import pytest

import nn_cases as nc
from test_gpu_nn_margins import MODES, _iters              # the handle settings every case runs under on the device

F = np.float32
CASES = list(nc.all_cases())


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------ grid_of
@pytest.mark.parametrize("gate", [0.49, 1.0, 4.0])
@pytest.mark.parametrize("kdiv", [1, 2, 3])
def test_grid_constants(gate, kdiv):
    rng = np.random.default_rng(0)
    m = rng.uniform(-20, 20, (500, 3)).astype(F)
    root = F(np.sqrt(F(gate)))
    g = nc.grid_of(m, dict(max_sq_dist=gate, cell_div=kdiv, tight_rows=3))
    assert g["cell"] == root * F(1.001) / F(kdiv) and g["grow_steps"] == 0 and g["xs"] == 1
    assert g["nx"] == int(np.floor((float(m[:, 0].max()) - float(g["origin"][0])) * float(g["inv_cell"]))) + 2
    assert g["n_tb"] == 3
    for t, frac in zip(g["tables"], (0.6, 0.3, 0.15)):
        assert t["reach"] == root * F(frac) and t["cell"] == t["reach"] * F(1.001)
        r = t["reach"] / F(1.0002)
        assert t["try_b2"] == r * r * F(0.999999)
        assert float(t["try_b2"]) < (float(t["reach"]) / 1.0002) ** 2 < float(t["cell"]) ** 2
    # the handle decides the defaults: a node's handle has plain rows, a batch handle x buckets four times finer and >= 1 table
    assert nc.grid_of(m, dict(max_sq_dist=gate))["n_tb"] == 0
    b = nc.grid_of(m, dict(max_sq_dist=gate, max_batch=64))
    assert b["xs"] == 4 and b["n_tb"] >= 1 and b["nxf"] == 4 * b["nx"]


@pytest.mark.parametrize("which", ["grow1", "grow3", "below64", "above64", "third192"])
def test_size_caps(which):
    m, _, _, cfg, note = nc.build_case("size_" + which)
    g = nc.grid_of(m, cfg)
    assert (g["grow_steps"], g["n_tb"]) == (note["expect"]["grow_steps"], note["expect"]["n_tb"])
    p = nc.grid_of(m, cfg, long_map_rule=False)
    assert (p["grow_steps"], p["n_tb"], p["n_cells"]) == (g["grow_steps"], g["n_tb"], g["n_cells"])   # sides under a kilometre
    cells = float(g["n_cells"]) * g["xs"]
    assert cells <= 256 * nc.MI
    if which.startswith("grow"):
        k = note["expect"]["grow_steps"]
        small = nc.grid_of(m, dict(cfg, cell_size=float(g["cell"] / F(1.5)) * g["k"]))      # one step less would not fit
        cell = F(1.001) / F(2)
        for _ in range(k):
            cell = cell * F(1.5)
        assert small["grow_steps"] >= 1 and g["cell"] == cell
    if which == "below64":
        assert cells <= 64 * nc.MI < cells + g["nx"] * g["ny"]                                 # one more layer of cells trips it
    if which == "above64":
        assert cells - g["nx"] * g["ny"] <= 64 * nc.MI < cells
    if which == "third192":
        full = nc.grid_of(m, dict(cfg, tight_rows=2))
        assert full["n_tb"] == 2 and full["buckets"] == g["buckets"] <= 192 * nc.MI and cells <= 64 * nc.MI
        t = g["tables"][1]                 # (not the 64 Mi rule, not the long-map rule -- `p` above --: the third table's buckets)
        assert g["buckets"] + 3.9 * t["ny"] * t["nz"] * g["nxf"] > 192 * nc.MI       # half the cell: four times the rows, less rounding


def test_short_maps_keep_their_tables(small_case):
    """Below a kilometre of extent the long-map rule changes nothing: the same cell, the same tables, the same first try."""
    rng = np.random.default_rng(5)
    dense = nc._dense_patch(rng, size=6.0)
    for m in (small_case["map"][:, :3], dense):
        for cfg in (dict(), dict(max_batch=64), dict(tight_rows=3), dict(tight_rows=3, cell_div=3, x_sub=8), dict(max_batch=64, cell_div=1)):
            a, b = nc.grid_of(m, cfg), nc.grid_of(m, cfg, long_map_rule=False)
            for key in ("cell", "n_cells", "nx", "ny", "nz", "n_tb", "tb_try", "buckets", "grow_steps"):
                assert a[key] == b[key], (cfg, key)
    assert nc.grid_of(dense, dict(max_batch=64))["n_tb"] == 3 and nc.grid_of(dense, dict(max_batch=64))["tb_try"] == 2


def test_long_map_rule_thresholds():
    """With a 1 m gate the 0.15 table goes at 1024 m of y or z extent, the 0.3 table at 2048 m, the 0.6 table at 4096 m, and the
    main grid takes cells 1.5 times larger from 4096 m; the x extent is free."""
    def n_tb(extent, axis=1):
        hi = [4.0, 4.0, 4.0]; hi[axis] = extent
        g = nc.grid_of(np.array([[0, 0, 0], hi], F), dict(tight_rows=3))
        return g["n_tb"], g["grow_steps"]
    for axis in (1, 2):
        assert [n_tb(e, axis) for e in (1000.0, 1030.0, 2040.0, 2050.0, 4090.0, 4100.0)] == \
               [(3, 0), (2, 0), (2, 0), (1, 0), (1, 0), (0, 1)]
    assert n_tb(17000.0, 0) == (3, 0)


# ------------------------------------------------------------------------------------------------ grid_of against the library
# (host only: lio_debug_grid_plan runs the parser and the two steps lio_s2m_set_map runs, on grid_of's box and cell count)
no_overrides = pytest.mark.skipif(any(os.environ.get(v) for v in ("LIO_TIGHT", "LIO_X_SUB", "LIO_TRY")),
                                  reason="the row tables are overridden from the environment")
SETTINGS = dict(MODES, plain_tables=None)


@pytest.fixture(scope="module")
def plan_of():
    api = importlib.import_module("lio-slam_amd.api")

    def run(m, cfg, caller_box=False):
        g = nc.grid_of(m, cfg)
        return g, api.debug_grid_plan(g["mn"], g["mx"], len(m), g["occupied"], caller_box, **cfg)
    return run


def _same_plan(g, p):
    """grid_of's dict against lio_grid_plan_info: floats as uint32 words, counts as integers"""
    want = dict(cell=_bits(g["cell"]), inv_cell=_bits(g["inv_cell"]), inv_cell_x=_bits(g["inv_cell_x"]), origin=_bits(g["origin"]).tolist(),
                pts_per_cell=_bits(g["pts_per_cell"]),
                counts=(g["nx"], g["ny"], g["nz"], g["n_cells"], g["k"], g["xs"], g["nxf"], g["n_tb"], g["tb_try"], g["grow_steps"], g["buckets"]),
                tables=[(_bits(t["reach"]), _bits(t["inv_cell"]), _bits(t["oy"]), _bits(t["oz"]), _bits(t["try_b2"]), t["ny"], t["nz"], t["row0"])
                        for t in g["tables"]] + [(_bits(-1.0), _bits(0.0), _bits(0.0), _bits(0.0), _bits(0.0), 0, 0, 0)] * (3 - g["n_tb"]))
    seen = dict(cell=_bits(p.cell), inv_cell=_bits(p.inv_cell), inv_cell_x=_bits(p.inv_cell_x), origin=_bits(list(p.origin)).tolist(),
                pts_per_cell=_bits(p.pts_per_cell),
                counts=(p.nx, p.ny, p.nz, p.n_cells, p.k, p.xs, p.nxf, p.n_tb, p.tb_try, p.grow_steps, p.buckets),
                tables=[(_bits(p.tb_reach[l]), _bits(p.tb_inv_cell[l]), _bits(p.tb_oy[l]), _bits(p.tb_oz[l]), _bits(p.tb_try_b2[l]),
                         p.tb_ny[l], p.tb_nz[l], p.tb_row0[l]) for l in range(3)])
    assert len(g["tables"]) == g["n_tb"]
    assert seen == want


@no_overrides
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", CASES)
def test_grid_of_is_the_librarys_plan(plan_of, name, setting):
    m, _, _, cfg, _ = nc.build_case(name)
    if setting == "plain_tables":
        full = dict(cfg, tight_rows=3, x_sub=1)
    else:                                                   # (as tests/test_gpu_nn_margins.py sets its handles up)
        full = dict(cfg, **MODES[setting])
        if setting != "batch":
            full.update(_iters(name)[2])
    _same_plan(*plan_of(m, full))


@no_overrides
@pytest.mark.parametrize("which", ["grow1", "grow3", "below64", "above64", "third192"])
def test_size_caps_in_the_library(plan_of, which):
    m, _, _, cfg, note = nc.build_case("size_" + which)
    g, p = plan_of(m, cfg)
    assert (p.grow_steps, p.n_tb) == (note["expect"]["grow_steps"], note["expect"]["n_tb"])
    cells = float(p.n_cells) * p.xs
    assert cells <= 256 * nc.MI
    if which.startswith("grow"):
        cell = F(1.001) / F(2)
        for _ in range(note["expect"]["grow_steps"]):
            cell = cell * F(1.5)
        assert _bits(p.cell) == _bits(cell)
        assert plan_of(m, dict(cfg, cell_size=float(F(p.cell) / F(1.5)) * p.k))[1].grow_steps >= 1      # one step less would not fit
    if which == "below64":
        assert cells <= 64 * nc.MI < cells + p.nx * p.ny
    if which == "above64":
        assert cells - p.nx * p.ny <= 64 * nc.MI < cells
    if which == "third192":
        full = plan_of(m, dict(cfg, tight_rows=2))[1]
        assert full.n_tb == 2 and full.buckets == p.buckets <= 192 * nc.MI and cells <= 64 * nc.MI
        assert p.buckets + 3.9 * p.tb_ny[1] * p.tb_nz[1] * p.nxf > 192 * nc.MI


@no_overrides
def test_long_map_rule_thresholds_in_the_library(plan_of):
    def n_tb(extent, axis=1):
        hi = [4.0, 4.0, 4.0]; hi[axis] = extent
        p = plan_of(np.array([[0, 0, 0], hi], F), dict(tight_rows=3))[1]
        return p.n_tb, p.grow_steps
    for axis in (1, 2):
        assert [n_tb(e, axis) for e in (1000.0, 1030.0, 2040.0, 2050.0, 4090.0, 4100.0)] == \
               [(3, 0), (2, 0), (2, 0), (1, 0), (1, 0), (0, 1)]
    assert n_tb(17000.0, 0) == (3, 0)


@no_overrides
def test_a_callers_box_counts_no_cells(plan_of):
    """A map whose box the caller supplies (assembled on the device, installed without a read-back) gets the one table of an
    automatic batch handle; the same map through lio_s2m_set_map gets what its density is worth."""
    dense = nc._dense_patch(np.random.default_rng(5), size=6.0)
    g, p = plan_of(dense, dict(max_batch=64), caller_box=True)
    assert g["occupied"] > 0 and not p.want_occupancy
    assert (p.n_tb, p.tb_try, p.pts_per_cell) == (1, -1, 0.0)
    g, p = plan_of(dense, dict(max_batch=64))
    assert p.want_occupancy and (p.n_tb, p.tb_try) == (3, 2) and p.pts_per_cell > 50
    _same_plan(g, p)


def test_environment_overrides(plan_of, monkeypatch):
    """LIO_TIGHT, LIO_X_SUB and LIO_TRY as the library parses them at every map set (A/B runs)."""
    for v in ("LIO_TIGHT", "LIO_X_SUB", "LIO_TRY"):
        monkeypatch.delenv(v, raising=False)
    m = nc._dense_patch(np.random.default_rng(5), size=6.0)
    root = F(1.0)

    def reaches(p):
        return [_bits(p.tb_reach[l]) for l in range(p.n_tb)]
    monkeypatch.setenv("LIO_TIGHT", "0.5,0.25")
    p = plan_of(m, dict())[1]
    assert p.n_tb == 2 and reaches(p) == [_bits(root * F(0.5)), _bits(root * F(0.25))]
    assert plan_of(m, dict(tight_rows=3))[1].n_tb == 2                       # (whatever the handle asked for)
    monkeypatch.setenv("LIO_TIGHT", "0")
    assert plan_of(m, dict(tight_rows=3))[1].n_tb == 0 and plan_of(m, dict(max_batch=64))[1].n_tb == 0
    monkeypatch.setenv("LIO_TIGHT", "0.3,0.6")                               # not descending: the list ends at the first entry
    p = plan_of(m, dict())[1]
    assert p.n_tb == 1 and reaches(p) == [_bits(root * F(0.3))]
    monkeypatch.setenv("LIO_TIGHT", "0.5,0.25")
    monkeypatch.setenv("LIO_TRY", "5")                                       # clamped to the tightest table there is
    assert plan_of(m, dict())[1].tb_try == 1
    monkeypatch.setenv("LIO_TRY", "0")
    assert plan_of(m, dict())[1].tb_try == 0
    monkeypatch.delenv("LIO_TIGHT"); monkeypatch.delenv("LIO_TRY")
    monkeypatch.setenv("LIO_X_SUB", "8")
    p = plan_of(m, dict())[1]
    assert p.xs == 8 and p.nxf == 8 * p.nx
    monkeypatch.setenv("LIO_X_SUB", "3")                                     # not 1, 2, 4 or 8: ignored
    assert plan_of(m, dict())[1].xs == 1 and plan_of(m, dict(max_batch=64))[1].xs == 4


# ------------------------------------------------------------------------------------------------ the emulation
def test_two_cell_misses_without_the_rule_none_with_it():
    exists, misses = nc.margin_emulation(8200.0, 1.0, 2, long_map_rule=False)
    assert exists and misses >= 1, "the grid before the long-map rule: the 0.15 table at 8200 m misses neighbours (CPU emulation)"
    extents = sorted(set([100.0 * 2 ** (j / 2) for j in range(19)] + [1000.0, 1023.0, 2047.0, 4095.0, 8200.0, 17000.0, 60000.0, 70000.0] +
                         [2.0 ** j - 8.0 for j in range(9, 15)]))                        # (just under where the spacing doubles)
    assert extents[0] == 100.0 and extents[-1] == 70000.0
    t = nc.grid_of(np.array([[0, -1016.0, 0], [4, 4, 4]], F), dict(max_sq_dist=0.55, tight_rows=3))["tables"]
    assert len(t) == 3 and 0.49 < float(np.spacing(F(1016.0))) / float(t[2]["cell"] - t[2]["reach"] / F(1.0001)) <= 0.5   # the adversarial gate
    for gate in (1.0, 0.49, 4.0, 0.55):
        for extent in extents:
            for which in (0, 1, 2, "main"):
                _, misses = nc.margin_emulation(extent, gate, which, long_map_rule=True, n_samples=1 << 18, seed=int(extent))
                assert misses == 0, (gate, extent, which, misses)


# ------------------------------------------------------------------------------------------------ every case under the oracle
def _oracle_runs(oracle, name):
    m, s, pose, cfg, note = nc.build_case(name)
    out = []
    for mode in (0, 1):
        ocfg = oracle.default_config(knn_mode=mode, n_threads=8, max_iters=1, max_sq_dist=cfg.get("max_sq_dist", 1.0))
        _, res, _, corr = oracle.scan2map(ocfg, s, m, pose, corr_iter=0)
        out.append((res, corr))
    return m, s, cfg, note, out


@pytest.mark.parametrize("name", CASES)
def test_case_holds_under_the_oracle(oracle, name):
    m, s, cfg, note, ((res0, c0), (res1, c1)) = _oracle_runs(oracle, name)
    assert len(m) <= 62000 and len(s) <= 3100
    np.testing.assert_array_equal(c0[0], c1[0])
    np.testing.assert_array_equal(np.sort(c0[2], 1), np.sort(c1[2], 1))
    np.testing.assert_array_equal(c0[2], c1[2])                         # and in the same (d2, index) order
    flag, nn = c1[0], c1[2]
    gate = F(cfg.get("max_sq_dist", 1.0))
    kind = note["kind"]
    if kind == "lattice":
        # the five of every query are the first five of the (d2, index) order, and most queries have a tie at the fifth place
        # (every coordinate is a multiple of 1/16: d2 is a multiple of 1/256, exact in fp32, and (d2, index) packs into one integer)
        d2 = ((s[:, None, 0] - m[None, :, 0]) ** 2 + (s[:, None, 1] - m[None, :, 1]) ** 2) + (s[:, None, 2] - m[None, :, 2]) ** 2
        key = (d2 * F(256)).astype(np.int64) * 8192 + np.arange(len(m))
        order = np.sort(np.partition(key, 5, axis=1)[:, :6], axis=1) % 8192
        d6 = np.take_along_axis(d2, order, 1)
        ok = d6[:, 4] < gate
        np.testing.assert_array_equal(nn[ok], order[ok, :5])
        assert (nn[~ok] == -1).all()
        assert (_bits(d6[ok, 4]) == _bits(d6[ok, 5])).sum() > 1500
    elif kind == "gate":
        q, fifth = s[note["probes"]], m[note["fifth"]]
        for e in (-1, 0, 1):
            sel = note["rel"] == e
            assert (_bits(nc.d2_f32(q[sel], fifth[sel])) == _bits(nc._next(gate, e))).all()
            if e < 0:
                np.testing.assert_array_equal(nn[note["probes"]][sel][:, 4], note["fifth"][sel])
            else:
                assert (nn[note["probes"]][sel] == -1).all()                   # `d2_5 < max_sq_dist` is strict
        assert (note["cell_off"] == cfg["cell_div"]).sum() >= 20 and (note["cell_off"] <= cfg["cell_div"]).all()
    elif kind == "table":
        g = nc.grid_of(m, dict(tight_rows=3))
        q, fifth = s[note["probes"]], m[note["fifth"]]
        np.testing.assert_array_equal(nn[note["probes"]][:, 4], note["fifth"])
        for i, (e, l) in enumerate(zip(note["rel"], note["level"])):
            t = g["tables"][l]
            d2 = nc.d2_f32(q[i], fifth[i])
            if e <= 1:
                assert _bits(d2) == _bits(nc._next(t["try_b2"], e))
            else:
                gy, gz = nc.cell_gap(nc.axis_grid(g, 1, l), q[i, 1], fifth[i, 1]), nc.cell_gap(nc.axis_grid(g, 2, l), q[i, 2], fifth[i, 2])
                assert max(gy, gz) == 2 and d2 > t["try_b2"] and d2 < gate
        assert nc.grid_of(m, dict(max_batch=64))["n_tb"] == 3 and nc.grid_of(m, dict(max_batch=64))["tb_try"] == 2
    elif kind == "bounded":
        tables = nc.grid_of(m, dict(tight_rows=3))["tables"]
        want = {0.0: 3, 1000.0: 3, 2040.0: 2, 4090.0: 1}[note["extent"]]                # the long-map rule: 1024 / 2048 / 4096 m
        assert len(tables) == want == nc.grid_of(m, dict(max_batch=64))["n_tb"] and len(nc.grid_of(m, dict(tight_rows=3), False)["tables"]) == 3
        d5 = np.sqrt(nc.d2_f32(s[nn[:, 4] >= 0], m[nn[nn[:, 4] >= 0, 4]]))
        for t in tables:                                                       # fifth neighbours on both sides of every reach
            assert ((d5 > 0.9 * t["reach"]) & (d5 < t["reach"])).sum() > 20 and ((d5 > t["reach"]) & (d5 < 1.1 * t["reach"])).sum() > 20
    elif kind == "outside":
        g = nc.grid_of(m, cfg)
        if len(m) > 5:
            c = np.stack([nc.cell_coord_f32(s[:, a], *nc.axis_grid(g, a)[:3]) for a in range(3)], 1)
            dims = np.array([g["nx"], g["ny"], g["nz"]])
            assert (c == -4).any(0).all() and (c == dims + 3).any(0).all()       # clamped, below and above, on every axis
            assert ((c < 0) | (c >= dims)).any(1).sum() > 400 and (nn[((c < 0) | (c >= dims)).any(1), 4] >= 0).sum() > 50
        else:
            assert ((nn[:, 4] >= 0).sum() > 20) == (len(m) == 5) and (len(m) == 5 or (nn == -1).all())   # fewer than five points: no query passes
    elif kind == "strip":
        q = s[note["probes"]]
        rows = nn[note["probes"]]
        assert ((rows == note["hinge"][:, None]).sum(1) == 1).all() and not (rows == note["decoy"][:, None]).any()
        d_h, d_d = nc.d2_f32(q, m[note["hinge"]]), nc.d2_f32(q, m[note["decoy"]])
        p = nc.grid_of(m, dict(cfg, max_batch=64), long_map_rule=False)
        b2 = np.array([gate if t < 0 else p["tables"][t]["try_b2"] for t in note["table"]], F)
        assert (d_h < d_d).all() and (d_d <= b2).all() and (d_d[note["table"] < 0] < gate).all()
        assert (d_h > b2 * F(0.999)).all()
        assert p["n_tb"] >= 2 and p["tb_try"] == p["n_tb"] - 1
        if note["extent"] == 8200.0 and note["axis"] in (1, 2) and gate == 1.0:
            assert ((note["gap"] > note["k"]) & (note["table"] == 2)).any()    # (emulated: what the device does is the GPU test's matter)
        if note["extent"] <= 900.0:
            assert not (note["gap"] > note["k"]).any()
        if note["axis"] == 0:                                                   # the run of fine x cells loses nothing; cx - k .. cx + k does
            assert not (note["gap"] > note["k"])[note["table"] >= 0].any()
            if note["compact"] and note["extent"] == 17000.0 and gate < 1.0:
                assert (note["gap"] > note["k"]).any()
    elif kind == "size":
        assert flag.sum() >= 50
    if kind in ("gate", "table", "strip", "bounded", "lattice"):
        assert res1.n_corr_last >= 50 or kind == "lattice" or note.get("compact")
