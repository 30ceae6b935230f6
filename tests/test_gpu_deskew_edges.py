"""GPU parity of projectPointCloud + deskewPoint and of the range-image build on inputs no lidar produces
(tests/deskew_cases.py): table, filter and column edges through lio_deskew, lio_deskew_pc2 and lio_range_image against
oracle/lio_oracle.c lo_project_point_cloud / lo_range_image -- the survivor count and the cloud, and for the range image
col, range, start_ring and end_ring as well, all BIT-EXACT: equality of the uint32 views, no tolerance anywhere.  Only the
nan_* cases may hold NaN: there NaN must sit in the same elements on both sides and every other element is bit-equal.
tests/test_deskew_cases_cpu.py shows that each named case reaches the edge it is named for.

Known exposure: both sides form (float)sin((double)x) with different fp64 libraries; a last-bit fp64 difference flips the
float rounding in about one evaluation in 10^8.  No case here has met it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deskew_cases as D                                  # noqa: E402

pytestmark = pytest.mark.gpu

NAMED = D.all_cases()
FIRST = D.cases("first")


@pytest.mark.parametrize("case", NAMED, ids=[c["id"] for c in NAMED])
def test_named_case_bit_exact(pkg, oracle, case):
    """'deskew' cases through lio_deskew, 'pc2' cases through lio_deskew_pc2 on the raw blob, 'ri' cases through lio_range_image."""
    ref = D.reference(oracle, case)
    out = D.compare(pkg, ref, case)
    assert len(out["cloud"]) == len(ref["cloud"])
    if case["kind"] == "pc2":                              # the same sweep as converted records through the record entry point
        D.compare(pkg, ref, case, case["id"] + " (records)", kind="deskew")


@pytest.mark.parametrize("case", FIRST, ids=[c["id"] for c in FIRST])
def test_first_survivor_does_not_depend_on_the_order_of_the_waves(pkg, oracle, case):
    """transStartInverse comes from the lowest surviving index, whichever wave's atomicMin lands first (or is skipped
    because the value it saw was already lower): three calls, each against the oracle, all three byte for byte; then the
    same sweep through the range image, whose first accepted point is found the same way."""
    ref = D.reference(oracle, case)
    outs = [D.compare(pkg, ref, case, f"{case['id']} call {k}") for k in range(3)]
    for o in outs[1:]:
        assert o["cloud"].tobytes() == outs[0]["cloud"].tobytes(), case["id"]
    ri = dict(case, H=1800, minRange=1.0)
    D.compare(pkg, D.run_oracle(oracle, ri, "ri"), ri, case["id"] + " (range image)", kind="ri")


def _abi_deskew(pkg, case, out_stride):
    """lio_deskew through the C ABI with output records of out_stride bytes, the output buffer pre-filled with 0xA5.
    -> (records as uint32 words [n, out_stride / 4], n_out)."""
    L = pkg.load_library()
    dcfg = pkg.deskew_default_config(**case["cfg"])
    rec = D.records(pkg, case)
    n, wo = len(rec), out_stride // 4
    out = np.full((n, wo), 0xA5A5A5A5, np.uint32)
    n_out = C.c_size_t(0)
    cur, T, RX, RY, RZ = case["imu"]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))            # noqa: E731
    rc = L.lio_deskew(C.byref(dcfg), rec.ctypes.data, n, rec.dtype.itemsize, case["t0"], dp(T), dp(RX), dp(RY), dp(RZ), cur,
                      out.ctypes.data, out_stride, C.byref(n_out))
    assert rc == 0, L.lio_last_error()
    return out, n_out.value


@pytest.mark.parametrize("out_stride", [20, 32, 48])
def test_output_strides(pkg, oracle, out_stride):
    case = D.cases("first")[3]                                         # first_1023: 3000 points in, 990 out
    ref = D.reference(oracle, case)
    out, n_out = _abi_deskew(pkg, case, out_stride)
    assert n_out == len(ref["cloud"]) > 500
    got = np.ascontiguousarray(out[:n_out, [0, 1, 2, 4]]).view(np.float32)
    rep = D.diff_report({"cloud": got}, ref)
    assert not rep, f"out_stride {out_stride}\n{rep}"
    assert (out[:n_out, 3] == np.float32(1.0).view(np.uint32)).all()   # PCL_ADD_POINT4D's padding word
    assert (out[:n_out, 5:] == 0).all()                                # bytes past the 20-byte record
    assert (out[n_out:] == 0xA5A5A5A5).all()                           # and nothing behind the last survivor


@pytest.mark.parametrize("t", range(20))
def test_fuzz(pkg, oracle, t):
    case, what = D.fuzz_trial(t)
    D.compare(pkg, D.run_oracle(oracle, case), case, what)
    D.compare(pkg, D.run_oracle(oracle, case, "ri"), case, what + " (range image)", kind="ri")


def test_refusals(pkg, oracle):
    """Every refusal happens on the host before any launch; the call after it is exact."""
    big = D.cases("time")[5]                                           # time_table2000: imuPointerCur 1999, the largest accepted
    assert big["imu"][0] == 1999
    pad = lambda a: np.concatenate([a, a[-1:] + 1.0])                  # noqa: E731
    too = dict(big, imu=(2000,) + tuple(pad(a) for a in big["imu"][1:]))
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        D.run_device(pkg, too)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        D.run_device(pkg, dict(too, H=1800, minRange=1.0), "ri")
    D.compare(pkg, D.reference(oracle, big), big)
    ri = dict(big, H=1800, minRange=1.0)
    D.compare(pkg, D.run_oracle(oracle, ri, "ri"), ri, kind="ri")
    small = D.cases("keep")[1]
    for kind in ("deskew", "ri"):
        with pytest.raises(pkg.LioError, match="ERR_ARG"):
            D.run_device(pkg, dict(small, cfg=dict(small["cfg"], downsampleRate=0), H=1800, minRange=1.0), kind)
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        D.run_device(pkg, dict(small, cfg=dict(small["cfg"], point_filter_num=0)))
    with pytest.raises(pkg.LioError, match="ERR_ARG"):
        D.run_device(pkg, dict(small, cfg=dict(small["cfg"], N_SCAN=1), H=32768, minRange=1.0), "ri")
    ok = dict(small, cfg=dict(small["cfg"], N_SCAN=1), H=32767, minRange=1.0)
    D.compare(pkg, D.run_oracle(oracle, ok, "ri"), ok, kind="ri")
    D.compare(pkg, D.reference(oracle, small), small)
