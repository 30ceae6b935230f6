"""The association's fast fp32 operations (lio-slam_amd/csrc/lio_device_math.h: lio_sqrt_fast / lio_sqrt, lio_div_fast against the
constant 5 / lio_div5) against the plain operators of the device, over ALL 2^32 bit patterns, through the library's test hook
lio_debug_fast_f32_ops: the hook evaluates both on the device and returns the number of words that differ and the first few
differing patterns (a NaN only has to be a NaN).

  raw sequence    0 differences on its guarded range: the root on [2^-96, +inf] (the guard `x >= 2^-96` lets +inf through, and the
                  sequence returns +inf there), the quotient on 2^-40 <= |x| < 2^40 (lio_div_mid)
  entry point     guard included: 0 differences on every pattern, i.e. also outside the guarded range

  fourth root     sqrtf(sqrtf(r2)) of the weight (MO:1671) has no guard of its own: r2 >= 2^-96 is one more term of the plane fit's
                  flag, and the fit's repeat supplies the plain value.  Hook op 2 runs lio_plane_fit5 on a fixed neighbour set with
                  the scan point (x, 0, 0) and takes the root as lio_assoc_point does: 0 differences from sqrtf(sqrtf(x * x)) on every
                  pattern, i.e. for zero, tiny (|x| < 2^-48), infinite and NaN points as well

and, as the independent reference, numpy's float32 sqrt and / (correctly rounded, as IEEE 754 requires of both) on 2^20
patterns: every special value and guard boundary with its neighbours, and random patterns."""
import importlib

import numpy as np
import pytest

CHUNK = 1 << 28
SQRT, DIV5, ROOT4 = 0, 1, 2


def _bits(x):
    return int(np.float32(x).view(np.uint32))


SQRT_LO, INF = _bits(2.0 ** -96), _bits(np.inf)                   # the root's guarded range [SQRT_LO, INF] (sign bit clear)
MID_LO, MID_HI = _bits(2.0 ** -40), _bits(2.0 ** 40)              # lio_div_mid: [MID_LO, MID_HI) and the same with the sign bit
SIGN = 1 << 31


@pytest.fixture(scope="module")
def api():
    return importlib.import_module("lio-slam_amd.api")


def _count(api, op, raw, first, count):
    """Differences over [first, first + count) in chunks; returns (total, first differing patterns)."""
    total, firsts = 0, []
    while count > 0:
        n = min(count, CHUNK)
        d, pats, _ = api.debug_fast_f32_ops(op, raw=raw, first=first, count=n)
        total += d
        firsts += [hex(int(p)) for p in pats]
        first += n
        count -= n
    return total, firsts[:8]


@pytest.mark.gpu
def test_fast_sqrt_equals_sqrtf_on_every_pattern(api):
    d, pats = _count(api, SQRT, True, SQRT_LO, INF - SQRT_LO + 1)
    print(f"raw root, [2^-96, +inf]: {INF - SQRT_LO + 1} patterns, {d} differ {pats}")
    assert d == 0, (d, pats)
    d, pats = _count(api, SQRT, False, 0, 1 << 32)
    print(f"guarded root, all 2^32 patterns: {d} differ {pats}")
    assert d == 0, (d, pats)


@pytest.mark.gpu
def test_fast_div5_equals_the_division_on_every_pattern(api):
    for sign in (0, SIGN):
        d, pats = _count(api, DIV5, True, sign + MID_LO, MID_HI - MID_LO)
        print(f"raw x / 5, sign {sign >> 31}, 2^-40 <= |x| < 2^40: {MID_HI - MID_LO} patterns, {d} differ {pats}")
        assert d == 0, (d, pats)
    d, pats = _count(api, DIV5, False, 0, 1 << 32)
    print(f"guarded x / 5, all 2^32 patterns: {d} differ {pats}")
    assert d == 0, (d, pats)


@pytest.mark.gpu
def test_fourth_root_of_the_range_on_every_pattern(api):
    d, pats = _count(api, ROOT4, False, 0, 1 << 32)
    print(f"fourth root through the plane fit's flag, all 2^32 scan points (x, 0, 0): {d} differ {pats}")
    assert d == 0, (d, pats)


def _patterns():
    """2^20 patterns: the special values and every guard boundary, each with its neighbours and with either sign, then random ones."""
    special = [0.0, np.finfo(np.float32).smallest_subnormal, 2.0 ** -140, np.finfo(np.float32).tiny, 2.0 ** -96, 2.0 ** -48,   # (2^-48: r2 = 2^-96)
               2.0 ** -40, 1.0, 5.0, 2.0 ** 40, 2.0 ** 96, np.finfo(np.float32).max, np.inf, np.nan]
    pats = []
    for v in special:
        b = _bits(v)
        pats += [b + k for k in (-2, -1, 0, 1, 2) if 0 <= b + k < SIGN]
    pats += [_bits(np.finfo(np.float32).tiny) - 1, 0x7f800001, 0x7fc00000, 0x7fffffff]     # largest denormal, signalling / quiet NaNs
    pats = np.array(sorted(set(pats)), np.uint32)
    pats = np.concatenate([pats, pats | np.uint32(SIGN)])
    rng = np.random.default_rng(20)
    rest = (1 << 20) - len(pats)
    # half uniform over all patterns, half uniform over the exponents around the guards' bounds
    uni = rng.integers(0, 1 << 32, rest // 2, dtype=np.uint64).astype(np.uint32)
    near = (rng.choice(np.array([SQRT_LO, MID_LO, MID_HI, 0, INF - (1 << 23)], np.uint32), rest - rest // 2)
            + rng.integers(-(1 << 23), 1 << 24, rest - rest // 2)).astype(np.int64) % (1 << 31)
    near = near.astype(np.uint32) | (rng.integers(0, 2, len(near)).astype(np.uint32) << np.uint32(31))
    return np.concatenate([pats, uni, near])


def _differs(got_bits, want):
    got = got_bits.view(np.float32)
    return np.flatnonzero((got_bits != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))


@pytest.mark.gpu
@pytest.mark.parametrize("op", [SQRT, DIV5], ids=["sqrt", "div5"])
def test_against_numpy_float32(api, op):
    pats = _patterns()
    assert len(pats) == 1 << 20
    x = pats.view(np.float32)
    with np.errstate(all="ignore"):
        want = np.sqrt(x) if op == SQRT else x / np.float32(5)
    assert want.dtype == np.float32
    # the guarded entry point on every pattern
    d, _, vals = api.debug_fast_f32_ops(op, raw=False, patterns=pats, want_values=True)
    bad = _differs(vals, want)
    print(f"op {op}: guarded entry, {len(pats)} patterns, {len(bad)} differ from numpy, {d} from the device's plain operator")
    assert len(bad) == 0 and d == 0, [(hex(int(pats[i])), hex(int(vals[i])), hex(int(want[i].view(np.uint32)))) for i in bad[:5]]
    # the raw sequence on the patterns of its guarded range
    if op == SQRT:
        inside = (pats >= SQRT_LO) & (pats <= INF)
    else:
        mag = pats & np.uint32(SIGN - 1)
        inside = (mag >= MID_LO) & (mag < MID_HI)
    assert inside.sum() > 1 << 17
    d, _, vals = api.debug_fast_f32_ops(op, raw=True, patterns=pats[inside], want_values=True)
    bad = _differs(vals, want[inside])
    print(f"op {op}: raw sequence, {int(inside.sum())} patterns of the guarded range, {len(bad)} differ from numpy")
    assert len(bad) == 0 and d == 0, [(hex(int(pats[inside][i])), hex(int(vals[i]))) for i in bad[:5]]


@pytest.mark.gpu
def test_fourth_root_against_numpy_float32(api):
    pats = _patterns()
    x = pats.view(np.float32)
    with np.errstate(all="ignore"):
        want = np.sqrt(np.sqrt(x * x))
    assert want.dtype == np.float32
    below = np.abs(x) < np.float32(2.0 ** -48)                       # r2 < 2^-96: the fit's repeat supplies the root
    assert below.sum() > 1 << 12 and (~below & np.isfinite(x)).sum() > 1 << 17
    d, _, vals = api.debug_fast_f32_ops(ROOT4, patterns=pats, want_values=True)
    bad = _differs(vals, want)
    print(f"fourth root: {len(pats)} patterns ({int(below.sum())} with r2 < 2^-96), {len(bad)} differ from numpy, {d} from the device")
    assert len(bad) == 0 and d == 0, [(hex(int(pats[i])), hex(int(vals[i])), hex(int(want[i].view(np.uint32)))) for i in bad[:5]]
