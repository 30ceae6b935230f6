"""Bit-exactness net of the serial Gauss-Newton step and of the corner line fit, through the library's test hooks
lio_debug_gn_step (lio_gn_step: lio_solve6_qr_reg, lio_eigen6_sym_lanes, the degeneracy rule, lio_inv6_lu_wave, lio_gemm6_wave,
the projection, the pose update, the convergence test, the loop control) and lio_debug_corner_fit (lio_corner_assoc with
lio_eigen3_sym), on the designed classes of tests/gn_math_cases.py: 2^16 6x6 systems and 2^20 five-point sets per class.

Every output word of both hooks is compared with the oracle's batch result (oracle/lio_oracle.c lo_lm_step_batch /
lo_corner_fit_batch).  No tolerance and no exclusions; in the corner fit a float word that is NaN in the oracle only has to be NaN
on the device (the 6x6 classes hold finite cases only, tests/test_gn_math_cases_cpu.py).  What the oracle's step does not return
is restated here: the float32 normal equations the step stores, the loop control of MO:1848-1859 with the fast-forward of a scan
with too few correspondences (expected_records), and T / trig of the new pose (gn_math_cases.transform_of, pinned against
Oracle.get_transformation on the CPU) wherever the registration goes on.

hold_if_done, from the source: a held step returns 2 and leaves pose, iter, done, status, converged, T and trig as they were;
AtA, AtB and n_corr_last are written before the decision, and so are matP / is_degenerate of a plain iteration 0 (the one-launch
loop holds only with skip_eigen there, and so does the `speculation` class).

The hooks run the source functions as compiled into the hooks' own kernels, not as inlined into k_s2m_iterate / k_s2m_persist;
the whole-registration tests remain that net."""
import importlib

import numpy as np
import pytest

import gn_math_cases as G

N_GN = 1 << 16
N_CORNER = 1 << 20
api = importlib.import_module("lio-slam_amd.api")
WORDS = api.DEBUG_GN_RECORD_DTYPE.itemsize // 4


def expected_records(oracle, b):
    """The record lio_debug_gn_step must return for every case of a batch."""
    n = len(b)
    o = G.oracle_step(oracle, b)
    solve, conv = o["solve"], o["conv"] == 1
    force, max_iters = bool(b.const("force_all_iters")), b.const("max_iters")
    it = b.it.astype(np.int64)
    ends = (conv & (not force)) | (it + 1 >= max_iters) | ~solve          # what hold_if_done asks
    held = ends if b.hold_if_done else np.zeros(n, bool)
    rec = np.zeros(n, api.DEBUG_GN_RECORD_DTYPE)
    rec["pose"] = np.where(held[:, None], b.pose, o["pose"])
    rec["matP"], rec["is_degenerate"] = o["matP"], o["deg"]
    rec["AtA"] = np.where(solve[:, None], b.AtA32().reshape(n, 36), 0)
    rec["AtB"] = np.where(solve[:, None], b.AtB32(), 0)
    rec["n_corr_last"] = b.nc()
    # MO:1848-1859: `for (iterCount < 30)`, `if (LMOptimization(iterCount)) break`; a scan below min_corr returns false without
    # touching the pose (MO:1721-1724), so its remaining iterations are identical and the device fast-forwards them
    iters = it + 1
    done = (conv & (not force)) | (iters >= max_iters)
    ff = ~solve & ~done
    iters = np.where(ff, max_iters, iters)
    done = done | ff
    rec["iter"] = np.where(held, it, iters)
    rec["done"] = np.where(held, 0, done)
    rec["status"] = np.where(held, 0, np.where(solve, 0, 2))
    rec["converged"] = np.where(held, 0, conv)
    rec["ret"] = np.where(held, 2, 0)
    goes_on = ~held & ~done
    T, trig = G.transform_of(rec["pose"][goes_on])
    rec["T"][goes_on], rec["trig"][goes_on] = T, trig
    return rec


def _words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(len(rec), WORDS)


def _run(b):
    return api.debug_gn_step(b.sums, b.pose, b.it, b.deg, b.matP, deg_override=b.deg_override, skip_eigen=b.skip_eigen,
                             hold_if_done=b.hold_if_done, **b.cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.GN_CLASSES))
def test_device_gn_step_bit_identical(pkg, oracle, name):
    total = 0
    for b in G.gn_class(name, N_GN, oracle):
        got, want = _run(b), expected_records(oracle, b)
        bad = np.flatnonzero((_words(got) != _words(want)).any(1))
        print(f"{name} / {b.tag}: {len(b)} cases, {len(bad)} mismatching; done {int(want['done'].sum())}, converged "
              f"{int(want['converged'].sum())}, degenerate {int(want['is_degenerate'].sum())}, held {int((want['ret'] == 2).sum())}")
        if len(bad):
            i = bad[0]
            fields = [f for f in got.dtype.names if not np.array_equal(np.ascontiguousarray(got[f][i]).view(np.uint32),
                                                                      np.ascontiguousarray(want[f][i]).view(np.uint32))]
            raise AssertionError(
                f"{name} / {b.tag}: {len(bad)} of {len(b)} cases differ, first {bad[:5].tolist()}; case {i} differs in {fields}\n"
                f"sums {b.sums[i].tolist()}\npose {b.pose[i].tolist()} iter {int(b.it[i])} is_degenerate {int(b.deg[i])} "
                f"deg_override {b.deg_override} skip_eigen {b.skip_eigen} hold_if_done {b.hold_if_done} cfg {b.cfg}\n"
                f"matP {b.matP[i].tolist()}\ndevice {got[i].tolist()}\noracle {want[i].tolist()}")
        total += len(b)
    assert total == N_GN


def _corner_mismatches(got, want):
    """Rows whose words differ; a float word that is NaN in `want` only has to be NaN in `got`."""
    diff = got != want
    wf, gf = want[:, :4].view(np.float32), got[:, :4].view(np.float32)
    diff[:, :4] &= ~(np.isnan(wf) & np.isnan(gf))
    return np.flatnonzero(diff.any(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CORNER_CLASSES))
def test_device_corner_fit_bit_identical(pkg, oracle, name):
    sets, pts, _ = G.corner_class(name, N_CORNER)
    got = api.debug_corner_fit(sets, pts, G.WEIGHT, G.MIN_S)
    flag, coeff = oracle.corner_fit_batch(oracle.default_config(), sets, pts)
    want = np.concatenate([coeff.view(np.uint32), flag.astype(np.uint32)[:, None]], 1)
    bad = _corner_mismatches(got, want)
    print(f"{name}: {len(sets)} cases, {len(bad)} mismatching; accepted {int(flag.sum())}, NaN coefficients {int(np.isnan(coeff).any(1).sum())}")
    assert len(bad) == 0, (f"{name}: {len(bad)} of {len(sets)} cases differ, first {bad[:5].tolist()}: set {sets[bad[0]].tolist()} point "
                           f"{pts[bad[0]].tolist()} device {got[bad[0]].tolist()} oracle {want[bad[0]].tolist()}")


@pytest.mark.gpu
def test_corner_fit_takes_other_weights(pkg, oracle):
    """weight and min_s are arguments of the hook: a second setting, on the class that sits on the accept test."""
    sets, pts, _ = G.corner_class("on_the_line", 1 << 12)
    got = api.debug_corner_fit(sets, pts, 0.5, 0.5)
    flag, coeff = oracle.corner_fit_batch(oracle.default_config(weight=0.5, min_s=0.5), sets, pts)
    want = np.concatenate([coeff.view(np.uint32), flag.astype(np.uint32)[:, None]], 1)
    assert len(_corner_mismatches(got, want)) == 0
    assert 0 < flag.sum() < len(flag)


# ------------------------------------------------------------------------------------------------ refusals: decided on the host before any
# launch, so these three run without a GPU as well
def _one():
    sums = np.zeros((3, 28))
    sums[:, [0, 6, 11, 15, 18, 20]] = 200.0
    sums[:, 27] = 100
    return sums, np.zeros((3, 6), np.float32), np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros((3, 36), np.float32)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e300])
def test_gn_step_refuses_non_finite_sums(pkg, bad):
    for col in (0, 5, 20, 21, 26, 27):
        if col == 27 and bad == 1e300:
            continue
        sums, pose, it, deg, matP = _one()
        sums[1, col] = bad                                     # (1e300: finite in fp64, infinite as the fp32 the step takes)
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            api.debug_gn_step(sums, pose, it, deg, matP)


def test_gn_step_refuses_bad_poses_counts_and_iterations(pkg):
    for k, bad in ((0, np.nan), (3, np.inf), (5, -np.inf)):
        sums, pose, it, deg, matP = _one()
        pose[2, k] = bad
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            api.debug_gn_step(sums, pose, it, deg, matP)
    for col, bad in ((27, -1.0), (27, 2.0 ** 31)):
        sums, pose, it, deg, matP = _one()
        sums[0, col] = bad
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            api.debug_gn_step(sums, pose, it, deg, matP)
    for bad in (-1, 32):
        sums, pose, it, deg, matP = _one()
        it[1] = bad
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            api.debug_gn_step(sums, pose, it, deg, matP)
    sums, pose, it, deg, matP = _one()
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        api.debug_gn_step(sums, pose, it, deg, matP, max_iters=33)


def test_empty_calls_succeed(pkg):
    out = api.debug_gn_step(np.zeros((0, 28)), np.zeros((0, 6), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                            np.zeros((0, 36), np.float32))
    assert out.shape == (0,) and out.dtype == api.DEBUG_GN_RECORD_DTYPE
    assert api.debug_corner_fit(np.zeros((0, 5, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0, 5)


@pytest.mark.gpu
def test_one_case_matches_and_a_finite_call_is_accepted(pkg, oracle):
    """The smallest launch: three cases, a partly filled workgroup."""
    sums, pose, it, deg, matP = _one()
    b = G.GnBatch(sums, pose, it, deg, matP)
    got, want = _run(b), expected_records(oracle, b)
    assert np.array_equal(_words(got), _words(want))
    assert (got["is_degenerate"] == 0).all() and np.array_equal(got["matP"][0].reshape(6, 6), np.eye(6, dtype=np.float32))
