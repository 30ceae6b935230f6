"""GPU parity of markOccludedPoints + extractFeatures on sweeps no lidar produces (tests/feature_cases.py): long, uneven and
adversarial rings through lio_extract_features against oracle/lio_oracle.c lo_extract_features -- cloudCurvature,
cloudNeighborPicked, cloudLabel, cornerCloud and surfaceCloud all BIT-EXACT, no tolerance anywhere.
tests/test_feature_cases_cpu.py shows that each named case reaches the edge it is named for.

Before each ring's load and write-back were cut to the window it owns ([start-5, end+4]) a ring also wrote back its stale
copy of cell end+5; test_shared_cell_is_not_lost is the test of that cell.  Its shared_cell_long sweeps put 3000- to
4086-point rings in front of 30-point rings, the order in which the stale copy lands last."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_cases as F                                 # noqa: E402

pytestmark = pytest.mark.gpu

NAMED = [c for name in F.CASES if name != "shared_cell" for c in F.cases(name)]
SHARED = F.cases("shared_cell")


@pytest.mark.parametrize("case", NAMED, ids=[c["id"] for c in NAMED])
def test_named_case_bit_exact(pkg, oracle, case):
    F.compare(pkg, F.reference(oracle, case), case["sweep"], case["id"], **case["cfg"])


@pytest.mark.parametrize("case", SHARED, ids=[c["id"] for c in SHARED])
def test_shared_cell_is_not_lost(pkg, oracle, case):
    """The last point of ring A (index end_A + 5) is the first cell of ring B's window: ring B's first pick marks it, and
    ring A, which never changes it, must not write its stale copy back.  Three calls per seed, each against the oracle and
    all three byte for byte: a value that depends on which workgroup finishes last must not pass on a lucky order."""
    sw, ref = case["sweep"], F.reference(oracle, case)
    outs = [pkg.extract_features(sw["cloud"], sw["start_ring"], sw["end_ring"], sw["col"], sw["range"]) for _ in range(3)]
    reports = [F.diff_report(o, ref, sw) for o in outs]
    for k, rep in enumerate(reports):
        if rep:
            print(f"{case['id']} call {k}:\n{rep}")
    assert not any(reports), f"{case['id']}:\n" + "\n".join(f"call {k}: {r}" for k, r in enumerate(reports) if r)
    for o in outs[1:]:
        for k in ("curvature", "picked", "label", "corner", "surface"):
            assert o[k].tobytes() == outs[0][k].tobytes(), (case["id"], k)


def test_too_long_ring_is_refused_and_the_next_call_is_exact(pkg, oracle):
    too = F.too_long_sweep()
    with pytest.raises(pkg.LioError, match="ERR_CAPACITY"):
        pkg.extract_features(too["cloud"], too["start_ring"], too["end_ring"], too["col"], too["range"])
    case = F.cases("longest_ring")[3]                          # one point fewer, between the same 12-point rings
    assert case["sweep"]["lengths"] == [12, F.MAX_RING, 12]
    F.compare(pkg, F.reference(oracle, case), case["sweep"], case["id"], **case["cfg"])


def _abi_call(pkg, sw, in_stride, out_stride, **cfg):
    """lio_extract_features through the C ABI with records of in_stride / out_stride bytes.  Unused input bytes hold noise;
    the output buffers are pre-filled with 0xA5.  -> (outputs as pkg.extract_features gives them, corner / surface
    records as uint32 words, n_corner, n_surface)."""
    L = pkg.load_library()
    c = pkg.FeatureConfig()
    L.lio_feature_default_config(C.byref(c))
    c.N_SCAN = len(sw["start_ring"])
    for k, v in cfg.items():
        setattr(c, k, v)
    n, wi, wo = len(sw["cloud"]), in_stride // 4, out_stride // 4
    rec = np.random.default_rng(7).integers(0, 2 ** 32, (n, wi), dtype=np.uint32).view(np.float32)
    rec[:, :3] = sw["cloud"][:, :3]
    rec[:, 4] = sw["cloud"][:, 3]
    corner = np.full((120 * c.N_SCAN, wo), 0xA5A5A5A5, np.uint32)
    surf = np.full((n, wo), 0xA5A5A5A5, np.uint32)
    curv = np.zeros(n, np.float32); picked = np.zeros(n, np.int32); label = np.zeros(n, np.int32)
    nc, ns = C.c_size_t(0), C.c_size_t(0)
    rc = L.lio_extract_features(C.byref(c), rec.ctypes.data, n, in_stride, sw["start_ring"].ctypes.data, sw["end_ring"].ctypes.data,
                                sw["col"].ctypes.data, sw["range"].ctypes.data, corner.ctypes.data, C.byref(nc),
                                surf.ctypes.data, C.byref(ns), out_stride, curv.ctypes.data, picked.ctypes.data, label.ctypes.data)
    assert rc == 0, L.lio_last_error()
    pts = lambda r, m: np.ascontiguousarray(r[:m, [0, 1, 2, 4]]).view(np.float32)            # noqa: E731
    return ({"corner": pts(corner, nc.value), "surface": pts(surf, ns.value), "curvature": curv, "picked": picked, "label": label},
            corner, surf, nc.value, ns.value)


@pytest.mark.parametrize("in_stride,out_stride", [(20, 32), (32, 20), (48, 32), (32, 48), (20, 24)])
def test_strides(pkg, oracle, in_stride, out_stride):
    sw = F.strides_sweep()
    ref = F.run_oracle(oracle, sw)
    out, corner, surf, nc, ns = _abi_call(pkg, sw, in_stride, out_stride)
    rep = F.diff_report(out, ref, sw)
    assert not rep, f"strides {in_stride} -> {out_stride}\n{rep}"
    assert nc > 20 and ns > 200
    pad = [w for w in range(out_stride // 4) if w not in (0, 1, 2, 4)]
    for name, r, m in (("corner", corner, nc), ("surface", surf, ns)):     # bytes of a record outside its four fields: as they
        words = r[:m, pad]                                                  # were, or zero (include/liogpu.h)
        assert np.isin(words, [0, 0xA5A5A5A5]).all(), name


@pytest.mark.parametrize("t", range(20))
def test_fuzz(pkg, oracle, t):
    sw, cfg, what = F.fuzz_trial(t)
    F.compare(pkg, F.run_oracle(oracle, sw, **cfg), sw, what, **cfg)
