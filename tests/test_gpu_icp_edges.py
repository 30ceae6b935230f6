"""Loop-closure ICP on the device at the edges of its search, step, criteria and hand-off: the designed cases of
tests/icp_cases.py (tests/test_icp_cases_cpu.py proves what each one hits), step by step against tests/icp_restate.py with
stepwise() of tests/test_gpu_icp.py, and the grid hook lio_icp_debug_grid against icp_restate.grid_of, bit for bit.

The step.  An entry of a step is held to 2 fp32 ulp of the restatement's wherever an ulp measures something: the entry is
at least 2^-10 in magnitude and the covariance is well conditioned.  Both are read from the reference alone: the restated
step is computed in fp64 by two routes (np.linalg.svd of the covariance, and of its transpose) and `dis` is their largest
entrywise disagreement over rotation and translation.  dis <= 2^-40 is "well conditioned".  Every other entry is compared
absolutely: |device - restated| <= 4 max(dis, 2^-40) + half an fp32 ulp of max(1, |entry|) -- the factor 4 lets a third
route (the device's Jacobi SVD) differ from each of the two by as much as they differ from each other, the last term is the
final rounding to fp32.  That term departs from "half an fp32 ulp of 1": for a rotation entry it is the same; for a
translation entry above 1 (3e5 in the far cases) half an ulp of 1 lies below half the spacing of the fp32 result, which no
rounded value can meet, so the entry's own spacing is taken.  DESIGN.md (section 2, loop-closure ICP) has the measured dis per case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_cases as IC                                     # noqa: E402
import icp_restate as R                                    # noqa: E402
from test_gpu_icp import stepwise, ulps, EPS52             # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -40
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = IC.build_case(name)
    return _CASES[name]


def check_grid(pkg, tgt):
    """hook == restatement, field for field, the floats by their bits"""
    G, H = R.grid_of(tgt), pkg.icp_debug_grid(tgt)
    if G is None:
        assert H.any == 0 and (H.nx, H.ny, H.nz, H.n_cells, H.edge) == (0, 0, 0, 0, 0.0)
        return G
    assert H.any == 1
    got = np.array(list(H.origin) + [H.edge, H.inv_cell], np.float32)
    ref = np.array(list(G["origin"]) + [G["edge"], G["inv_cell"]], np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got.tolist(), ref.tolist())
    assert (H.nx, H.ny, H.nz, H.n_cells, H.occupied) == (G["nx"], G["ny"], G["nz"], G["n_cells"], G["occupied"])
    return G


def two_routes(s, t):
    """The restated step in fp64 by two routes -> (step 3x4 of route 1, dis)."""
    s = np.asarray(s, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    n = len(s)
    ms, mt = s.sum(0) / n, t.sum(0) / n
    cov = (t[:, :, None] * s[:, None, :]).sum(0) / n - np.outer(mt, ms)
    R1 = R.umeyama_rotation(cov)[0]
    R2 = R.umeyama_rotation(cov.T)[0].T
    A = np.concatenate([R1, (mt - R1 @ ms)[:, None]], 1)
    B = np.concatenate([R2, (mt - R2 @ ms)[:, None]], 1)
    return A, float(np.abs(A - B).max())


def residual(step, s, t):
    s = np.asarray(s, np.float64)
    t = np.asarray(t, np.float64)
    M = np.asarray(step, np.float64)
    return (s @ M[:3, :3].T + M[:3, 3]) - t


class Judge:
    def __init__(self, name, note):
        self.name, self.note, self.dis = name, note, 0.0

    def __call__(self, k, dev, ref, s, t):
        dev64 = np.asarray(dev, np.float64)
        Rm = dev64[:3, :3]
        assert abs(np.linalg.det(Rm) - 1.0) <= 1e-6 and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-6, (k, Rm)
        assert np.array_equal(dev[3], [0, 0, 0, 1])
        _, dis = two_routes(s, t)
        self.dis = max(self.dis, dis)
        bound = 4.0 * max(dis, FLOOR)
        if "rank" in self.note:
            # the null-space columns of an SVD are arbitrary: no comparison with np.linalg.svd's step at all
            rank = self.note["rank"]
            if rank == 0:
                assert np.array_equal(dev[:3, :3], np.eye(3, dtype=np.float32)), dev
            # the pairs' summed squared residual: an entry error b moves a residual by at most sqrt(3) b (|s|_1 + 1)
            r_dev, r_ref = residual(dev, s, t), residual(ref, s, t)
            b = bound + 2.0 ** -24
            w = np.sqrt(3.0) * b * (np.abs(np.asarray(s, np.float64)).sum(1) + 1.0)
            allowed = float((2.0 * np.linalg.norm(r_ref, axis=1) * w + w * w).sum())
            e_dev, e_ref = float((r_dev ** 2).sum()), float((r_ref ** 2).sum())
            print(f"  {self.name} iteration {k}: rank {rank}, residual {e_dev:.6e} (restated {e_ref:.6e}, allowed + {allowed:.3e}), dis {dis:.3e}")
            assert e_dev <= e_ref + allowed, (e_dev, e_ref, allowed)
            return
        diff = np.abs(dev64[:3] - np.asarray(ref, np.float64)[:3])
        big = (np.abs(ref[:3]) >= 2.0 ** -10) & (dis <= FLOOR)
        u = ulps(dev[:3], ref[:3])
        lim = bound + 0.5 * np.spacing(np.maximum(np.abs(ref[:3]), np.float32(1.0))).astype(np.float64)
        print(f"  {self.name} iteration {k}: dis {dis:.3e}; {int(big.sum())} entries by ulp (worst {float(u[big].max()) if big.any() else 0.0:.2f}), "
              f"{int((~big).sum())} absolutely (worst {float(diff[~big].max()) if (~big).any() else 0.0:.3e} of {float(lim.min()):.3e})")
        assert (u[big] <= 2.0).all(), (k, u)
        assert (diff[~big] <= lim[~big]).all(), (k, diff, lim)


def run_case(pkg, name):
    src, tgt, over, guess, note = case(name)
    cfg = pkg.icp_default_config(**over)
    judge = Judge(name, note)
    res, _, k_n = stepwise(pkg, src, tgt, cfg, guess=guess, judge_step=judge)
    print(f"{name}: {k_n} iterations, state {pkg.ICP_STATES[res.state]}, dis {judge.dis:.3e}")
    return res, k_n, judge


def trace0(pkg, name):
    src, tgt, over, guess, note = case(name)
    return pkg.icp_debug_trace(src, tgt, pkg.icp_default_config(**over), guess=guess, rec_iter=0)


@pytest.mark.parametrize("name", IC.NAMES)
def test_case_stepwise_fitness_grid_and_determinism(pkg, name):
    src, tgt, over, guess, note = case(name)
    cfg = pkg.icp_default_config(**over)
    check_grid(pkg, tgt)
    res, k_n, judge = run_case(pkg, name)
    T = np.array(res.T, np.float32).reshape(4, 4)
    fit = R.fitness(T, src, tgt)
    if fit == R.DBL_MAX:
        assert res.fitness == R.DBL_MAX
    else:
        assert abs(res.fitness - fit) <= len(src) * EPS52 * fit, (res.fitness, fit)
    # twice through the plain entry point: the same bytes, and the traced run's answer
    a, rc_a = pkg.icp_align(src, tgt, cfg, guess=guess)
    b, rc_b = pkg.icp_align(src, tgt, cfg, guess=guess)
    assert rc_a == rc_b == 0 and bytes(a) == bytes(b) == bytes(res)
    # what the case is about, where the step-wise parity does not already say it
    what = note.get("what")
    if "state" in note:
        assert res.state == note["state"], pkg.ICP_STATES[res.state]
    if "iters" in note:
        assert res.iters == note["iters"]
    if what == "criteria" and note["kind"] == "drop":
        _, steps, n_corr, _, _ = trace0(pkg, name)
        assert (res.state, res.converged, res.iters, k_n) == (R.NO_CORRESPONDENCES, 0, note["drop_at"], note["drop_at"] + 1)
        assert list(n_corr) == note["n_corr"] and res.n_corr_last == note["n_corr"][-1]
        assert np.array_equal(T, R.compose(steps[1], steps[0]))
    if what == "gate_edge":
        _, _, n_corr, _, corr = trace0(pkg, name)
        for p in note["probes"]:
            assert corr[p["src"]] == (p["tgt"] if p["side"] <= 0 else -1), p
        assert n_corr[0] == sum(p["side"] <= 0 for p in note["probes"])
    if what == "one_point":
        _, _, n_corr, _, corr = trace0(pkg, name)
        assert (corr == 0).all() and n_corr[0] == len(src)
    if what == "big_coords":
        _, _, n_corr, _, corr = trace0(pkg, name)
        assert (corr[-note["n_bad_src"]:] == -1).all() and not np.isin(corr, note["bad_tgt"]).any()
        assert n_corr[0] == len(src) - note["n_bad_src"] and np.isfinite(res.fitness)
    if what == "outside":
        _, _, n_corr, _, _ = trace0(pkg, name)
        assert n_corr[0] == (len(src) if note["wide"] else len(src) - note["n_out"]) and np.isfinite(res.fitness)
    if what == "shell_exit" and note["mirror"]:
        other, _ = pkg.icp_align(*case("shell_exit")[:2], pkg.icp_default_config(**case("shell_exit")[2]))
        assert other.n_launches == res.n_launches


def test_lookahead_changes_nothing_at_any_workgroup_bound(pkg):
    for n in IC.WG_SIZES:
        src, tgt, over, guess, _ = case(f"wg_{n}")
        ref = None
        for la in IC.LOOKAHEADS:
            res, rc = pkg.icp_align(src, tgt, pkg.icp_default_config(**dict(over, lookahead=la)))
            got = (bytes(res.T), res.iters, res.state, res.converged, res.n_corr_last, res.fitness)
            ref = ref or got
            assert rc == 0 and got == ref, (n, la)


def test_guess_refused_when_not_finite_and_returned_for_an_empty_source(pkg):
    src, tgt, over, guess, _ = case("guess_skew")
    cfg = pkg.icp_default_config(**over)
    lib = pkg.load_library()
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 15):
            g = guess.copy().reshape(16)
            g[at] = bad
            r = pkg.IcpResult()
            args = (0, src.ctypes.data, len(src), 12, tgt.ctypes.data, len(tgt), 12, C.byref(cfg), g.ctypes.data_as(C.POINTER(C.c_float)))
            assert lib.lio_icp_align(*args, C.byref(r)) == -1                                              # LIO_ERR_ARG
            assert lib.lio_icp_debug_trace(*args, -1, C.byref(r), None, None, None, None, None) == -1
    for s, t in ((src[:0], tgt), (src, tgt[:0])):
        res, rc = pkg.icp_align(s, t, cfg, guess=guess)
        assert rc == 0 and (res.state, res.converged, res.iters) == (R.NO_CORRESPONDENCES, 0, 0) and res.fitness == R.DBL_MAX
        assert np.array_equal(np.array(res.T, np.float32).reshape(4, 4), guess)


def test_a_target_without_a_point_in_range_has_no_grid_and_no_pairs(pkg):
    src = case("wg_65")[0]
    for tgt in (np.full((10, 3), np.nan, np.float32), np.array([[2.0e15, 0, 0], [0, np.inf, 0]], np.float32),
                np.array([[2.0e15, 0, 0], [0, 3.0e15, 0], [0, 0, -1.0e16]], np.float32)):
        assert check_grid(pkg, tgt) is None or not R.target_ok(tgt).any()
        res, rc = pkg.icp_align(src, tgt, pkg.icp_default_config(max_corr_dist=1.0e6))
        assert rc == 0 and (res.state, res.n_corr_last, res.iters) == (R.NO_CORRESPONDENCES, 0, 0) and res.fitness == R.DBL_MAX
