"""The inputs tests/test_gpu_grid_convert.py (the library) and tests/test_grid_convert_cpu.py (lio_gridconvert.h on the host)
share: the smallest shapes at which the tile walk, the dword runs and the compactions can still go wrong, with the values that
sit on a rounding or a comparison."""
import numpy as np

import grid_convert_restate as R

f32, u32 = np.float32, np.uint32
# one short of, exactly, and one past a 64 x 64 tile in each direction; a single cell, a single row, a single column
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (67, 45)]
FORMATS_OUT = [(ch, depth) for depth in (R.IMAGE_8U, R.IMAGE_16U, R.IMAGE_32F) for ch in (1, 3, 4)]
FORMATS_IN = [(ch, depth) for ch, depth in FORMATS_OUT if depth != R.IMAGE_32F or ch == 1]
LOWER, UPPER = f32(-0.75), f32(1.25)


def _below_integer(lo, hi, depth, k):
    """a value whose scaled value is the float just below the integer k (searched a few floats down from the exact one)"""
    mx = R.image_max(depth)
    x = f32(lo + f32(hi - lo) * f32(f32(k) / mx))
    for _ in range(16):
        s = f32(f32(f32(x - lo) / f32(hi - lo)) * mx)
        if s == np.nextafter(f32(k), f32(0.0)):
            return x
        x = np.nextafter(x, f32(-np.inf)) if s >= f32(k) else np.nextafter(x, f32(np.inf))
    return x


def image_layer(rows, cols, depth, lo=LOWER, hi=UPPER, seed=0):
    """[rows, cols] float32: random values a fifth beyond the bounds on either side, then by hand (from the front, as many as
    fit): the bounds themselves, one float inside and outside each, +-inf, NaN, +-0, values scaled to just below an integer"""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    span = float(hi - lo)
    v = rng.uniform(float(lo) - 0.2 * span, float(hi) + 0.2 * span, rows * cols).astype(f32)
    up, down = f32(np.inf), f32(-np.inf)
    special = [lo, hi, np.nextafter(lo, up), np.nextafter(lo, down), np.nextafter(hi, up), np.nextafter(hi, down), up, down, f32(np.nan), f32(0.0), f32(-0.0)]
    special += [_below_integer(lo, hi, depth, k) for k in (1, 2, 3, 100, 127, 128, 254)] if depth != R.IMAGE_32F else []
    at = rng.permutation(rows * cols)[:len(special)]
    v[at] = np.array(special, f32)[:len(at)]
    return v.reshape((rows, cols), order="F")


def ingest_image(rows, cols, channels, depth, seed=0, color=False):
    """an image to take in: grey values over the whole range; colour channels equal (what toImage writes, and what every grey
    weighting that sums to the full scale returns exactly) unless `color`; alpha on either side of the default threshold"""
    rng = np.random.default_rng(7000 * rows + 13 * cols + 5 * channels + depth + seed)
    if depth == R.IMAGE_32F:
        return rng.uniform(-0.5, 1.5, (rows, cols, 1)).astype(f32)
    dt, top = R.DTYPES[depth], int(R.image_max(depth))
    img = np.zeros((rows, cols, channels), dt)
    grey = rng.integers(0, top + 1, (rows, cols))
    grey.ravel()[:3] = [0, top, top // 2][:grey.size]
    for ch in range(min(channels, 3)):
        img[:, :, ch] = rng.integers(0, top + 1, (rows, cols)) if color else grey
    if channels == 4:
        mid = top // 2                                         # (Type)(0.5 * max) = 127 / 32767
        img[:, :, 3] = rng.choice([0, mid - 1, mid, mid + 1, top], (rows, cols))
    return img


def cloud_layers(rows, cols, seed=0):
    """{0: heights with holes, 1: a layer with NaNs and a payload NaN of its own, 2: colours (any bits), 3: finite everywhere}"""
    rng = np.random.default_rng(31 * rows + cols + seed)
    h = rng.uniform(-1, 1, (rows, cols)).astype(f32)
    h[rng.random((rows, cols)) < 0.3] = np.nan
    h[rng.random((rows, cols)) < 0.05] = np.inf
    o = rng.uniform(-1, 1, (rows, cols)).astype(f32)
    o.view(u32)[rng.random((rows, cols)) < 0.2] = 0x7fc12345
    c = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(u32).view(f32)
    return {0: h, 1: o, 2: c, 3: rng.uniform(0, 1, (rows, cols)).astype(f32)}


def survivors_layer(rows, cols, which):
    """a height layer with exactly the survivors the compaction's corners need"""
    n = rows * cols
    v = np.full(n, np.nan, f32)
    if which == "all":
        v[:] = np.arange(n, dtype=f32)
    elif which == "one":
        v[n // 2] = 1.0
    elif which == "last workgroup":                            # nothing before the last 256 cells' workgroup
        v[(n - 1) // 256 * 256 + (n - 1) % 256 // 2:] = 2.0
    elif isinstance(which, int):                               # exactly that many, spread over the workgroups
        at = np.linspace(0, n - 1, which).round().astype(int)
        assert len(set(at.tolist())) == which
        v[at] = at.astype(f32)
    return v.reshape((rows, cols), order="F")
