"""The outlier filter on the device (lio_sor_filter) on the designed inputs of tests/sor_cases.py, which
tests/test_sor_cases_cpu.py proves to hit the edges they name: the grid of the hook lio_sor_debug_grid against
localmap_restate.sor_grid bit for bit, then mean_dist, the return value, the statistics and the kept records against the
restatement through tests/test_gpu_localmap.py's check_filter, and two runs byte for byte."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_restate as L                              # noqa: E402
import sor_cases as S                                     # noqa: E402
from test_gpu_localmap import bits, check_filter, stat_difference          # noqa: E402

pytestmark = pytest.mark.gpu


def check_grid(pkg, cloud, mean_k):
    """hook == restatement, field for field, the floats by their bits"""
    G, H = L.sor_grid(cloud, mean_k), pkg.sor_debug_grid(cloud, mean_k)
    got = np.array(list(H.origin) + [H.edge, H.inv_cell], np.float32)
    ref = np.array(list(G["origin"]) + [G["edge"], G["inv_cell"]], np.float32)
    assert np.array_equal(bits(got), bits(ref)), (got.tolist(), ref.tolist())
    assert (H.nx, H.ny, H.nz, H.n_cells, H.occupied) == (G["nx"], G["ny"], G["nz"], G["n_cells"], G["occupied"])
    assert H.any == 1
    return G


@pytest.mark.parametrize("name", S.NAMES)
def test_case_grid_filter_and_determinism(pkg, name):
    cloud, k, mul, note = S.build_case(name)
    ref = S.reference(name)
    G = check_grid(pkg, cloud, k)
    t0 = time.perf_counter()
    got = pkg.sor_filter(cloud, k, mul)
    dt = time.perf_counter() - t0
    print(f"  {name}: grid {G['nx']} x {G['ny']} x {G['nz']} edge {G['edge']}, the filter's call {dt * 1e3:.1f} ms")
    check_filter(got, ref, cloud, name, bracket=note.get("bracket") != "sign")
    assert len(got[0]) == int(ref["keep"].sum())
    if "bad" in note:
        assert np.isnan(got[1][note["bad"]]).all() and np.isfinite(np.delete(got[1], note["bad"])).all()
    again = pkg.sor_filter(cloud, k, mul)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    assert np.array_equal(np.array(got[2]).view(np.uint64), np.array(again[2]).view(np.uint64)) and got[3] == again[3]


def test_nan_threshold_empties_the_output_and_zero_variance_keeps_everything(pkg):
    """a variance that rounding makes negative gives a NaN threshold and an empty output; a variance of
    exactly 0 gives threshold = every dist_i and keeps everything (dist_i <= thr)."""
    cloud, k, mul, _ = S.build_case("equal_spacing_nan")
    inl, dist, stats, rc = pkg.sor_filter(cloud, k, mul)
    d = np.float32(1.0 + 3.0 * 2.0 ** -12)
    assert rc == 0 and len(inl) == 0 and (bits(dist) == bits(d)).all()
    assert stats[0] == float(d) and np.isnan(stats[1]) and np.isnan(stats[2])
    for name, d in (("equal_spacing_zero", 0.3125), ("one_cell_copies", 0.0)):
        cloud, k, mul, _ = S.build_case(name)
        inl, dist, stats, rc = pkg.sor_filter(cloud, k, mul)
        assert rc == 0 and stats == (d, 0.0, d) and (dist == np.float32(d)).all()
        assert np.array_equal(bits(inl), bits(cloud))


@pytest.mark.parametrize("name", ["big_coords", "big_coords_edge"])
def test_records_beyond_the_bound_change_nothing_for_the_others(pkg, name):
    cloud, k, mul, note = S.build_case(name)
    bad, clean = pkg.sor_filter(cloud, k, mul), pkg.sor_filter(note["clean"], k, mul)
    out = np.zeros(len(cloud), bool)
    out[note["bad"]] = True
    assert np.array_equal(bits(bad[0]), bits(clean[0])) and np.array_equal(bits(bad[1][~out]), bits(clean[1]))
    assert np.isnan(bad[1][out]).all() and (bad[3], clean[3]) == (0, 0)
    # the records shift the others' places in the fixed summation tree: the statistics agree to the tree's bound, not bit for bit
    assert max(stat_difference(a, b) for a, b in zip(bad[2], clean[2])) <= 64 * len(note["clean"]) * 2.0 ** -52
    assert 0 < len(bad[0]) < len(note["clean"])


def test_a_cloud_without_a_participant_has_one_empty_cell(pkg):
    cloud = np.zeros((5, 4), np.float32)
    cloud[:, 0] = [np.nan, np.inf, 2.0e15, -np.inf, 3.0e38]
    H = pkg.sor_debug_grid(cloud, 10)
    assert (H.any, H.nx, H.ny, H.nz, H.n_cells, H.occupied, H.edge) == (0, 1, 1, 1, 1, -1, 1.0) and list(H.origin) == [0.0, 0.0, 0.0]
    inl, dist, stats, rc = pkg.sor_filter(cloud, 10, 1.0)
    ref = L.sor(cloud, 10, 1.0)
    assert rc == ref["rc"] == 1 and len(inl) == 0 and np.isnan(dist).all() and stats == (0.0, 0.0, np.inf)
    H = pkg.sor_debug_grid(cloud[:0], 10)
    assert (H.any, H.n_cells, H.occupied) == (0, 0, -1)
