"""Cost of the terrain layers on the device (lio_terrain_layers) on a 550 x 400 grid at 0.2 m -- the default crop of the local
map at the loader's resolution -- with the yaml's three lengths scaled by 10 (normal_radius 0.5, smooth_radius 0.6,
edge_window_length 0.5): a tilted plane with noise, boxes and 8 % holes.

GPU time: HIP events on the null stream around each call (everything of this entry point runs there), medians of --reps runs,
the forms alternating.  The whole call (grid up, two kernels, eight layers down) for the area and the raster normals; the same
without the layers' copy (layers == NULL) and with one layer; the two kernels by difference between forms that make one of
them trivial (raster normals with a smooth radius of 0: k_terr_main reads five cells; a window of one cell: k_terr_edges reads
one), both without the copy; the copy of the layers' bytes to the host and of the grid's bytes to the device, timed beside
the calls as stand-ins.  Host stand-in: scipy.ndimage convolutions and numpy gradients for the same eight layers, wall clock.
It is NOT grid_map (no circle iterators, no eigen decomposition per cell, no EigenLab) and is reported, not judged.

    python tools/terrain_cost.py [--reps 20] [--out profiles/terrain_cost.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS, RES = 550, 400, 0.2
SCALED = dict(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)


def scene(seed=3):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(ROWS) * RES, np.arange(COLS) * RES, indexing="ij")
    z = 0.05 * x - 0.03 * y + rng.normal(0, 0.02, x.shape)
    for _ in range(40):
        r, c = rng.integers(0, ROWS - 12), rng.integers(0, COLS - 12)
        z[r:r + rng.integers(3, 12), c:c + rng.integers(3, 12)] += rng.uniform(0.3, 2.0)
    z[rng.uniform(size=z.shape) < 0.08] = np.nan
    return np.asfortranarray(z.astype(np.float32))


def host_stand_in(grid):
    """disc means, gradient normals, slope, roughness, windowed standard deviation, traversability (not grid_map) -> seconds"""
    from scipy import ndimage
    t0 = time.perf_counter()
    z = grid.astype(np.float64)
    ok = np.isfinite(z)
    k = int(SCALED["smooth_radius"] / RES)
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    disc = (xx * xx + yy * yy <= (SCALED["smooth_radius"] / RES) ** 2).astype(np.float64)
    num = ndimage.convolve(np.where(ok, z, 0.0), disc, mode="constant")
    den = ndimage.convolve(ok.astype(np.float64), disc, mode="constant")
    smooth = num / np.where(den > 0, den, np.nan)
    gx, gy = np.gradient(np.where(ok, z, smooth), RES)
    nz = 1.0 / np.sqrt(gx * gx + gy * gy + 1.0)
    slope = np.arccos(nz)
    rough = np.abs(z - smooth)
    m1 = ndimage.uniform_filter(np.nan_to_num(slope), 3, mode="nearest")
    m2 = ndimage.uniform_filter(np.nan_to_num(slope) ** 2, 3, mode="nearest")
    edges = np.sqrt(np.maximum(m2 - m1 * m1, 0.0))
    trav = np.clip(np.nan_to_num(0.5 * (1 - slope / 0.6) + 0.5 * (1 - rough / 0.1)), 0.0, 1.0)
    return time.perf_counter() - t0, float(np.nansum(edges) + trav.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("terrain_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    grid = scene()
    n_cells = ROWS * COLS
    ln, ps = (C.c_double * 2)(ROWS * RES, COLS * RES), (C.c_double * 2)(12.5, -3.0)
    out = np.zeros(8 * n_cells, np.float32)
    info = pkg.TerrainInfo()

    def call(with_layers=True, **kw):
        cfg = pkg.terrain_default_config(**dict(SCALED, **kw))
        rc = lib.lio_terrain_layers(0, grid.ctypes.data, ROWS, COLS, RES, ln, ps, C.byref(cfg), out.ctypes.data if with_layers else None, out.size,
                                    C.byref(info))
        assert rc == 0, rc

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(torch.cuda.default_stream()); fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        return a.elapsed_time(b)

    d_layers = torch.zeros(8 * n_cells, dtype=torch.float32, device="cuda")
    h_layers, h_grid = torch.from_numpy(out), torch.from_numpy(np.ascontiguousarray(grid.ravel(order="F")))
    forms = {
        "terrain_layers_area_ms": lambda: call(),
        "terrain_layers_raster_ms": lambda: call(normal_method=1),
        "one_layer_ms": lambda: call(layers=1 << 7),
        "no_copy_ms": lambda: call(with_layers=False),
        "no_copy_raster_ms": lambda: call(with_layers=False, normal_method=1),
        "no_copy_trivial_main_ms": lambda: call(with_layers=False, normal_method=1, smooth_radius=0.0),
        "no_copy_trivial_edges_ms": lambda: call(with_layers=False, edge_window_size=1),
        "d2h_copy_of_layer_bytes_ms": lambda: h_layers.copy_(d_layers),
        "h2d_copy_of_grid_bytes_ms": lambda: d_layers[:n_cells].copy_(h_grid),
    }
    samples = {name: [] for name in forms}
    for fn in forms.values():
        fn()                                                    # warm-up: the pool, the code objects
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            samples[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in samples.items()}
    call()
    s_host, _ = host_stand_in(grid)
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": ROWS, "cols": COLS, "resolution": RES, "config": SCALED,
        "layer_bytes": 4 * 8 * n_cells, "n_valid_cells": info.n_valid_cells, "n_normal_cells": info.n_normal_cells,
        "n_few_points": info.n_few_points, "n_degenerate": info.n_degenerate, "edge_window_size": info.edge_window_size, **med,
        "kernels_by_difference_ms": {
            "k_terr_main_area_against_trivial": med["no_copy_ms"] - med["no_copy_trivial_main_ms"],
            "k_terr_main_raster_against_trivial": med["no_copy_raster_ms"] - med["no_copy_trivial_main_ms"],
            "k_terr_edges_against_one_cell_window": med["no_copy_ms"] - med["no_copy_trivial_edges_ms"],
            "layers_copy_inside_the_call": med["terrain_layers_area_ms"] - med["no_copy_ms"],
        },
        "host_stand_in_not_grid_map": {"what": "scipy.ndimage disc mean, numpy gradient normals, uniform-filter standard deviation", "ms": 1000.0 * s_host},
        "unmeasured": ["the kernels one by one (differences of whole calls against a trivial form of the same kernel; no rocprofv3 pass)",
                       "lio_kf_store_terrain_map against lio_kf_store_height_map followed by lio_terrain_layers from the host",
                       "grid_map, EigenLab and Eigen themselves"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
