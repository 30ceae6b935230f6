"""The occupancy grid chain of the fork's draft ogmGeneration.cpp (OG), restated in numpy: what "identical" means for
lio_radius_filter, lio_occupancy_grid and lio_kf_store_occupancy_grid.  Brute force throughout.

  slice          pcl::PassThrough<PointXYZ> on z, OG:74-93
  radius_counts  pcl::RadiusOutlierRemoval's neighbour counts, OG:96-112: FLANN L2_Simple in fp32, strict d2 < r2
  raster         SetMapTopicMsg, OG:115-188, as written and with the labelled extension whole_box
"""
import numpy as np

MAX_COORD = np.float32(1.0e15)                 # the cell sort's bound: a point beyond it takes no part
f32 = np.float32


def takes_part(xyz):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(xyz) <= MAX_COORD).all(axis=1)              # (NaN compares false)


def slice_z(xyz, z_min, z_max, negative=0):
    """-> the indices PassThrough keeps, in order: finite points with z_min <= z <= z_max (limits as floats, inclusive), or the
    finite points outside when negative"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    fin = np.isfinite(xyz).all(axis=1)
    with np.errstate(invalid="ignore"):
        inside = (xyz[:, 2] >= f32(z_min)) & (xyz[:, 2] <= f32(z_max))
    return np.nonzero(fin & (~inside if negative else inside))[0]


def radius_counts(xyz, radius, block=512):
    """-> k_i [n] int32: the participating points j, i itself and duplicates included, with
    d2 = ((dx dx) + dy dy) + dz dz < r2 in fp32, r2 = (float)((double)radius * radius); -1 where i takes no part"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    part = takes_part(xyz)
    p = xyz[part]
    r2 = f32(np.float64(f32(radius)) * np.float64(f32(radius)))
    k = np.zeros(len(p), np.int32)
    for a in range(0, len(p), block):
        q = p[a:a + block]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz                      # float32 arrays: every operation rounds to fp32, no FMA
        assert d2.dtype == np.float32
        k[a:a + block] = (d2 < r2).sum(axis=1)
    out = np.full(len(xyz), -1, np.int32)
    out[part] = k
    return out


def radius_keep(xyz, radius, min_neighbors):
    """-> (indices kept, in order; k_i): a point stays iff k_i > min_neighbors"""
    k = radius_counts(xyz, radius)
    return np.nonzero(k > int(min_neighbors))[0], k


def raster(xyz, resolution, whole_box=0):
    """-> (grid [height, width] int8, width, height, (x_min, y_min), n_binned).  The box in fp64 over the points 0 .. n - 2
    (OG:139; all of them for whole_box, and for a single point); width = (int)((x_max - x_min) / resolution);
    i = (int)((x - x_min) / resolution) toward zero; skipped iff i < 0 || i >= width || j < 0 || j >= height - 1 (height for
    whole_box); grid[j, i] = 100."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return np.zeros((0, 0), np.int8), 0, 0, (0.0, 0.0), 0
    res = float(resolution)
    m = n if (whole_box or n == 1) else n - 1
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    x_min, x_max, y_min, y_max = x[:m].min(), x[:m].max(), y[:m].min(), y[:m].max()
    width, height = int(np.trunc((x_max - x_min) / res)), int(np.trunc((y_max - y_min) / res))
    grid = np.zeros((height, width), np.int8)
    i = np.trunc((x - x_min) / res).astype(np.int64)
    j = np.trunc((y - y_min) / res).astype(np.int64)
    j_end = height if whole_box else height - 1
    ok = ~((i < 0) | (i >= width) | (j < 0) | (j >= j_end))
    if width and height:
        grid[j[ok], i[ok]] = 100
    return grid, width, height, (float(x_min), float(y_min)), (int(ok.sum()) if width and height else 0)


def occupancy_grid(xyz, z_min=0.2, z_max=2.0, z_negative=0, remove_outliers=1, radius=0.5, min_neighbors=10, resolution=0.05,
                   whole_box=0):
    """the whole chain -> (grid, info dict with the fields of lio_ogm_info)"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    sl = xyz[slice_z(xyz, z_min, z_max, z_negative)]
    inl = sl[radius_keep(sl, radius, min_neighbors)[0]] if remove_outliers else sl
    grid, w, h, origin, n_binned = raster(inl, resolution, whole_box)
    return grid, dict(width=w, height=h, origin=origin, n_in=len(xyz), n_slice=len(sl), n_inliers=len(inl), n_binned=n_binned,
                      n_occupied=int((grid == 100).sum()))
