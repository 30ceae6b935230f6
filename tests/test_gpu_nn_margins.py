"""The 5-NN grid search on the cases of tests/nn_cases.py -- exact lattices (ties), fifth neighbours exactly at the gate and at a
tight table's acceptance bound, queries outside the grid, maps kilometres long, the size caps of lio_plan_grid / lio_plan_tables (lio_gridplan.h) -- against the
oracle's kd-tree search, the way tests/test_gpu_fuzz.py::_check compares: flags, 5-NN indices and the coefficients of accepted
points bit for bit at the recorded iteration, the correspondence counts of every iteration, the pose within 1e-5.  Every case
runs through the launch-per-iteration loop, the one-launch loop and a batch handle with its automatic row tables; the lattices
the gate edges and the x strips also through the LDS-staged search; the bounded search (iteration 2) on a dense patch, alone
and at the far end of grids just under the extents at which the long-map rule drops a table.  The grid the device reports (cells, tight tables, first try) must be
the one tests/nn_cases.py::grid_of restates from that plan (held against it field for field in tests/test_nn_cases_cpu.py)."""
import os

import numpy as np
import pytest

import nn_cases as nc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(os.environ.get(v) for v in ("LIO_TIGHT", "LIO_X_SUB", "LIO_TRY")),
                                 reason="the row tables are overridden from the environment")]

MODES = {"launches": dict(pipeline=1), "one_launch": dict(pipeline=4), "batch": dict(max_batch=64),
         "lds": dict(use_lds=1, sort_scan=2)}
_REF = {}


def _iters(name):
    """(recorded iteration, max_iters, settings the case adds to the plain handles)"""
    if name.startswith(("table_bounded", "strip_bounded")):
        return 2, 3, dict(tight_rows=3, x_sub=1)
    return 0, 1, dict()


def _reference(oracle, name):
    if name not in _REF:
        m, s, pose, cfg, _ = nc.build_case(name)
        it, max_iters, _ = _iters(name)
        ocfg = oracle.default_config(knn_mode=1, n_threads=8, max_iters=max_iters, max_sq_dist=cfg.get("max_sq_dist", 1.0))
        _REF[name] = oracle.scan2map(ocfg, s, m, pose, corr_iter=it)
    return _REF[name]


def _params():
    out = []
    for name in nc.all_cases():
        for mode in MODES:
            if mode == "lds" and not name.startswith(("lattice", "gate", "strip_x")):
                continue
            out.append(pytest.param(name, mode, id=f"{name}-{mode}"))
    return out


@pytest.mark.parametrize("name,mode", _params())
def test_nn_margins(pkg, oracle, name, mode):
    m, s, pose, cfg, note = nc.build_case(name)
    it, max_iters, plain = _iters(name)
    full = dict(cfg, **MODES[mode])
    if mode != "batch":
        full.update(plain)
    po, ro, _, corr = _reference(oracle, name)
    s2m = pkg.ScanToMap(record_corr_iter=it, max_iters=max_iters, **full)
    try:
        s2m.set_map(m)
        p, res, rc = s2m.scan2MapOptimization(s, pose)
        flag, coeff, nn = s2m.get_correspondences(0)
        prof = s2m.profile()
    finally:
        s2m.close()
    g = nc.grid_of(m, full)
    bad = np.nonzero((nn != corr[2]).any(1))[0]
    probes = set(np.asarray(note.get("probes", ()), np.int64).tolist())
    seen = (f"n_cells {prof.n_cells} ({g['n_cells']}) tables {prof.map_tight_tables} ({g['n_tb']}) first try {prof.map_first_try} "
            f"({g['tb_try']}); 5-NN rows that differ {len(bad)}, probes among them {sorted(probes & set(bad.tolist()))}")
    assert rc == ro.status and res.iters == ro.iters, seen
    np.testing.assert_array_equal(flag, corr[0], err_msg=seen)
    np.testing.assert_array_equal(nn, corr[2], err_msg=seen)
    np.testing.assert_array_equal(coeff.view(np.uint32)[flag == 1], corr[1].view(np.uint32)[flag == 1])
    assert list(res.n_corr_iter)[:ro.iters] == list(ro.n_corr_iter)[:ro.iters] and res.n_corr_last == ro.n_corr_last
    if ro.n_corr_last >= 50:
        a, b = np.array(res.AtA, np.float32), np.array(ro.AtA, np.float32)
        assert it > 0 or (a.view(np.uint32) != b.view(np.uint32)).sum() <= 2       # (one iteration: the same sums, rounded once)
        np.testing.assert_allclose(p, po, rtol=0, atol=1e-5)
    else:
        np.testing.assert_array_equal(p, po)
    if it == 2:
        assert ro.iters == 3 and int(flag.sum()) > 1000
    # the grid: what the plan laid out (lio_gridplan.h, through lio_map_finish) is what grid_of restates (cells after the size and long-map rules, tables, first try)
    assert (prof.n_cells, prof.map_x_sub, prof.map_tight_tables, prof.map_first_try) == (g["n_cells"], g["xs"], g["n_tb"], g["tb_try"]), seen
    if note["kind"] == "size" and mode != "batch":
        assert (g["grow_steps"], g["n_tb"]) == (note["expect"]["grow_steps"], note["expect"]["n_tb"])
