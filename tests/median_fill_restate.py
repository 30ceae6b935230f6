"""grid_map_filters/src/MedianFillFilter.cpp restated in numpy, literally: iterated 3 x 3 erosions and dilations on windows
clipped to the image (OpenCV's default border: cells outside take no part), and a sorted window per cell.  Slow and plain on
purpose; the device (lio_median_fill) is held to it bit for bit.  Grids are [rows, cols] float32."""
import numpy as np

f32, u32 = np.float32, np.uint32
QNAN_BITS = 0x7fc00000


def radius_cells(radius, resolution):
    """static_cast<size_t>(radius / resolution), :127-128: a double division, truncated"""
    return int(float(radius) / float(resolution))


def morph3(mask, erode):
    """cv::erode / cv::dilate with the 3 x 3 rectangle anchored at its centre, default border"""
    rows, cols = mask.shape
    out = np.empty_like(mask)
    for r in range(rows):
        for c in range(cols):
            w = mask[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2]
            out[r, c] = w.min() if erode else w.max()
    return out


def cleaned_mask(valid):
    """cleanedMask, :212-224, every call as written: the third overwrites what the first two left"""
    m = morph3(valid, False)
    m = morph3(m, True)
    m = morph3(valid, True)
    m = morph3(m, False)
    return m


def fill_holes(mask, n):
    """fillHoles, :226-239: one dilation, the loop from 1, then n erosions"""
    m = morph3(mask, False)
    for _ in range(1, n):
        m = morph3(m, False)
    for _ in range(n):
        m = morph3(m, True)
    return m


def box(mask, k, erode):
    """k iterations as one (2k + 1)^2 box clipped to the image"""
    rows, cols = mask.shape
    out = np.empty_like(mask)
    for r in range(rows):
        for c in range(cols):
            w = mask[max(r - k, 0):r + k + 1, max(c - k, 0):c + k + 1]
            out[r, c] = w.min() if erode else w.max()
    return out


def masks_box_form(valid, n):
    """the form the kernel uses -> (cleaned, fill)"""
    cleaned = box(box(valid, 1, True), 1, False)
    m = box(cleaned, max(n, 1), False)
    return cleaned, (box(m, n, True) if n > 0 else m)


def ordered_key(values):
    """the order-preserving float -> uint32 mapping of lio_wg.h: -0 sorts below +0"""
    u = np.ascontiguousarray(values, f32).view(u32)
    return np.where(u & u32(0x80000000), ~u, u | u32(0x80000000)).astype(u32)


def median_bits(grid, r, c, R):
    """getMedian, :153-186 -> the uint32 bits of the result"""
    rows, cols = grid.shape
    r0, r1 = max(r - R, 0), min(r + R, rows - 1)               # boundIndexToRange on both corners
    c0, c1 = max(c - R, 0), min(c + R, cols - 1)
    w = grid[r0:r1 + 1, c0:c1 + 1].ravel()
    w = w[np.isfinite(w)]
    if w.size == 0:
        return QNAN_BITS
    order = np.argsort(ordered_key(w), kind="stable")          # std::nth_element's position n / 2, -0 below +0
    return int(w[order[w.size // 2]].view(u32))


def median_fill(grid, resolution, fill_hole_radius=0.05, existing_value_radius=0.0, filter_existing_values=0,
                num_erode_dilation_iterations=4, mask_in=None):
    """update(), :106-151 -> dict(filled, fill_mask, cleaned_mask (None with mask_in), and the counts of lio_median_fill_info)"""
    g = np.ascontiguousarray(grid, f32)
    rows, cols = g.shape
    valid = np.isfinite(g)
    if mask_in is None:
        cleaned = cleaned_mask(valid.astype(np.uint8))
        mask = fill_holes(cleaned, num_erode_dilation_iterations).astype(f32)
        cleaned = cleaned.astype(f32)
    else:
        cleaned, mask = None, np.ascontiguousarray(mask_in, f32)
    R_fill, R_ex = radius_cells(fill_hole_radius, resolution), radius_cells(existing_value_radius, resolution)
    out = g.view(u32).copy()
    n_filtered = 0
    for r in range(rows):
        for c in range(cols):
            m = bool(mask[r, c] != 0.0)
            if not valid[r, c] and m:
                out[r, c] = median_bits(g, r, c, R_fill)
            elif filter_existing_values and m:
                out[r, c] = median_bits(g, r, c, R_ex)
                n_filtered += 1
    filled = out.view(f32)
    fin_out = np.isfinite(filled)
    return dict(filled=filled, fill_mask=mask, cleaned_mask=cleaned, fill_radius_cells=R_fill, existing_radius_cells=R_ex,
                n_nan_in=int((~valid).sum()), n_mask=int((mask != 0).sum()), n_filled=int((~valid & fin_out).sum()),
                n_filtered=n_filtered, n_nan_out=int((~fin_out).sum()))


# ---- the shapes the device and the host check are run on -----------------------------------------------------------------------
def make_grid(rows, cols, seed, holes=0.3):
    """distinct values from a seeded generator with 30 % random holes, a 4 x 5 and a 9 x 9 hole, holes in all four corners, a
    valid strip two cells wide along one edge, isolated valid specks inside a large hole, repeated values, -0 / +0, +-inf and
    a NaN with a payload -- whatever of it fits rows x cols"""
    rng = np.random.default_rng(seed)
    g = rng.permutation(rows * cols).astype(f32).reshape(rows, cols) * f32(0.01) - f32(1.0)
    g[rng.uniform(size=g.shape) < holes] = np.nan
    if rows >= 8 and cols >= 8:
        g[3:7, 2:7] = np.nan                                   # 4 x 5
    if rows >= 16 and cols >= 12:
        g[rows - 14:rows - 5, 1:10] = np.nan                   # 9 x 9
        g[rows - 10, 5] = f32(7.5)                             # specks: the opening takes them out of the mask
        g[rows - 8, 3] = f32(-7.5)
        g.view(u32)[rows - 10, 6] = 0xffc54321                 # a NaN with a payload where the mask stays 0 (N <= 4)
    if rows >= 4 and cols >= 4:
        for r in (0, rows - 1):
            for c in (0, cols - 1):
                g[r, c] = np.nan
        g[1:rows - 1, cols - 2:] = np.abs(g[1:rows - 1, cols - 2:])
        g[1:rows - 1, cols - 2:][~np.isfinite(g[1:rows - 1, cols - 2:])] = f32(0.25)     # the strip, with repeated values
    if rows >= 8 and cols >= 8:
        g[2, 1], g[2, 2], g[1, 1] = f32(-0.0), f32(0.0), f32(-0.0)
        g[5, 5], g[6, 6] = np.inf, -np.inf
        g.view(u32)[4, 6] = 0x7fc12345                         # a NaN with a payload
        g[7, 2] = g[7, 3] = g[2, 3] = f32(0.125)               # repeated values around the 4 x 5 hole
    return g


def checksum(res):
    """what tools/median_fill_host_check.cpp prints for a case: FNV-1a over the filled grid's words, then the fill mask's,
    column-major"""
    h = 0xcbf29ce484222325
    for a in (res["filled"], res["fill_mask"]):
        for w in np.asfortranarray(a).view(u32).ravel(order="F").tolist():
            for k in range(4):
                h = ((h ^ ((w >> (8 * k)) & 0xff)) * 0x100000001b3) & 0xffffffffffffffff
    return h
