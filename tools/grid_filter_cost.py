"""Cost of filtering a resident planning layer on the device (lio_grid_filter_radius, lio_grid_filter_window,
lio_grid_filter_curvature, lio_grid_filter_threshold, lio_grid_duplicate_layer) on a 550 x 400 grid at 0.2 m (220 000 cells)
with the lengths of grid_map_demos' filters_demo_filter_chain.yaml times ten (the yaml's map is 0.02 m): a radius of 0.6 m
(3 cells), a window length of 0.5 m (3 cells), the box blur's window of 5, the 3 x 3 kernels; beside them the largest reach the
calls accept (32 cells, a window of 65).  Each call whole and its kernel alone, and three comparisons in the same run:
  - a device-to-device copy of one layer's bytes (one layer read, one written): the floor of a call that derives a layer;
  - lio_terrain_layers on the same grid, whose two kernels do the arithmetic of MEAN in a radius and of STDDEV over CROP among
    their other layers: the whole call with all eight layers copied to the host and with none (upload, both kernels, counters);
  - the host route the calls replace: lio_grid_get_layer, a numpy / scipy stand-in for the filter (NOT grid_map: a vectorised
    footprint mean that treats NaN differently and sums in another order), lio_grid_set_layers of the result.

GPU time: HIP events, medians of --reps runs with their quartiles, the forms alternating.  The whole call is timed on the null
stream around the entry point (everything of the call runs there and it ends complete); the kernel is the call's own pair of marks
(lio_grid_filter_debug_kernel_ms); beside them the wall time of the call on the host.  The host route is wall time, piece by
piece.  No figure is a pass bar and none is a comparison with grid_map, which is not built.

    python tools/grid_filter_cost.py [--reps 20] [--out profiles/grid_filter_cost.json]
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
f32 = np.float32
EDGE = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], f32)


def scene(rng):
    x, y = np.arange(ROWS)[:, None] * RES, np.arange(COLS)[None, :] * RES
    z = 0.08 * x - 0.05 * y + 0.3 * np.sin(0.7 * x) * np.cos(0.4 * y) + rng.normal(0, 0.01, (ROWS, COLS))
    z[rng.random((ROWS, COLS)) < 0.08] = np.nan
    return z.astype(f32)


def spread(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median": float(q[1]), "q25": float(q[0]), "q75": float(q[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_filter_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_filter_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    length, position = (ROWS * RES, COLS * RES), (12.0, -7.0)
    z = scene(rng)
    g, up = pkg.Grid(), pkg.Grid()
    g.set_layers([z, z], RES, length, position)

    forms = {
        "radius_mean_0p6m_3_cells": lambda: g.filter_radius(0, 2, pkg.GF_MEAN, 0.6),
        "radius_min_0p6m_3_cells": lambda: g.filter_radius(0, 2, pkg.GF_MIN, 0.6),
        "radius_mean_6p4m_32_cells": lambda: g.filter_radius(0, 2, pkg.GF_MEAN, 6.4),
        "window_stddev_crop_length_0p5m_size_3": lambda: g.filter_window(0, 2, pkg.GW_STDDEV, pkg.GW_CROP, 0, 0.5),
        "window_mean_of_finites_crop_size_5": lambda: g.filter_window(0, 2, pkg.GW_MEAN_OF_FINITES, pkg.GW_CROP, 5),
        "window_weighted_sum_edge_mean_3x3": lambda: g.filter_window(0, 2, pkg.GW_WEIGHTED_SUM, pkg.GW_EDGE_MEAN, 3, 0.0, EDGE),
        "window_sum_inside_size_5": lambda: g.filter_window(0, 2, pkg.GW_SUM, pkg.GW_INSIDE, 5),
        "window_min_of_finites_empty_size_5": lambda: g.filter_window(0, 2, pkg.GW_MIN_OF_FINITES, pkg.GW_EMPTY, 5),
        "window_stddev_crop_size_65": lambda: g.filter_window(0, 2, pkg.GW_STDDEV, pkg.GW_CROP, 65),
        "window_mean_of_finites_in_place_size_5": lambda: g.filter_window(1, 1, pkg.GW_MEAN_OF_FINITES, pkg.GW_CROP, 5),
        "curvature": lambda: g.filter_curvature(0, 2),
        "threshold_upper": lambda: g.filter_threshold(0, 1, True, 5.0, float("nan")),
        "duplicate_layer": lambda: g.duplicate_layer(0, 2),
    }
    ms = C.c_float()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); info = fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_filter_debug_kernel_ms(1, C.byref(ms))
        return a.elapsed_time(b), wall, ms.value, info

    n_bytes = ROWS * COLS * 4
    src_t, dst_t = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

    def copy_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); dst_t.copy_(src_t); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # lio_terrain_layers on the same grid with the same radius and window; normals by the raster method, so that the main
    # kernel's other work is small beside its MeanInRadius loop
    cfg_all = pkg.terrain_default_config(normal_method=1, smooth_radius=0.6, edge_window_length=0.5)
    cfg_none = pkg.terrain_default_config(normal_method=1, smooth_radius=0.6, edge_window_length=0.5, layers=0)
    zf = np.asfortranarray(z)
    ln, ps = (C.c_double * 2)(*length), (C.c_double * 2)(*position)
    buf = np.empty(8 * ROWS * COLS, f32)
    tinfo = pkg.TerrainInfo()

    def terrain(cfg, out):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(torch.cuda.default_stream())
        rc = lib.lio_terrain_layers(0, zf.ctypes.data, ROWS, COLS, RES, ln, ps, C.byref(cfg), out.ctypes.data if out is not None else None,
                                    out.size if out is not None else 0, C.byref(tinfo))
        b.record(torch.cuda.default_stream())
        b.synchronize()
        assert rc == 0, lib.lio_last_error()
        return a.elapsed_time(b)

    lib.lio_grid_filter_debug_kernel_ms(1, None)
    for fn in forms.values():                                   # warm-up: the pool's blocks, the layers, the code objects
        fn()
    copy_ms(); terrain(cfg_all, buf); terrain(cfg_none, None)
    samples, copies, t_all, t_none, infos = {name: [] for name in forms}, [], [], [], {}
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            ev, wall, kernel, info = timed(fn)
            samples[name].append((ev, wall, kernel))
            if info is not None:
                infos[name] = {k: int(info[k]) for k in info.dtype.names if k != "pad"}
        copies.append(copy_ms())
        t_all.append(terrain(cfg_all, buf))
        t_none.append(terrain(cfg_none, None))
    lib.lio_grid_filter_debug_kernel_ms(0, None)
    copy = spread(copies)
    calls = {}
    for name, v in samples.items():
        v = np.array(v)
        calls[name] = {"whole_call_ms": spread(v[:, 0]), "host_wall_ms": spread(v[:, 1]), "kernel_ms": spread(v[:, 2]),
                       "kernel_over_copy_of_one_layer": float(np.median(v[:, 2]) / copy["median"]) if copy["median"] > 0 else None, "info": infos.get(name)}

    # the same words as lio_terrain_layers, at the size that is timed
    d, _ = pkg.terrain_layers(z, RES, length, position, cfg_all)
    g.set_layers([z, d["slope"]], RES, length, position)
    g.filter_radius(0, 2, pkg.GF_MEAN, 0.6)
    same_smooth = bool(np.array_equal(g.layer(2).view(np.uint32), np.ascontiguousarray(d["smooth"]).view(np.uint32)))
    g.filter_window(1, 3, pkg.GW_STDDEV, pkg.GW_CROP, 0, 0.5)
    e, w = g.layer(3), d["edges"]
    same_edges = bool(np.array_equal(np.isnan(e), np.isnan(w)) and np.array_equal(e[~np.isnan(e)].view(np.uint32), w[~np.isnan(w)].view(np.uint32)))

    # the host route for the mean in a radius of 3 cells: down, a stand-in on the host, up
    from scipy import ndimage
    yy, xx = np.mgrid[-3:4, -3:4]
    disc = (xx * xx + yy * yy <= 9).astype(np.float64)
    t = []
    g.set_layers([z, z], RES, length, position)
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        down = g.layer(0)
        t1 = time.perf_counter()
        fin = np.isfinite(down)
        s = ndimage.convolve(np.where(fin, down, 0.0).astype(np.float64), disc, mode="constant")
        n = ndimage.convolve(fin.astype(np.float64), disc, mode="constant")
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (s / n).astype(f32)
        t2 = time.perf_counter()
        up.set_layers([mean], RES, length, position)
        t3 = time.perf_counter()
        t.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
    t = np.array(t)
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "grid": [ROWS, COLS, RES], "cells": ROWS * COLS,
        "clock": "HIP events: around the call on the null stream (whole call), around the call's kernel; medians with quartiles over the "
                 "alternating runs.  Host route: perf_counter",
        "device_to_device_copy_of_one_layer_0p88_MB_ms": copy, "calls": calls,
        "lio_terrain_layers_same_grid": {"raster_normals_smooth_0p6m_window_3": True, "whole_call_eight_layers_to_host_ms": spread(t_all),
                                         "whole_call_no_layer_to_host_ms": spread(t_none),
                                         "what_it_includes": "the grid's upload, k_terr_main (smooth, raster normals, slope, roughness, traversability), k_terr_edges, "
                                                             "the counters; with eight layers also their copy to pageable host memory",
                                         "filter_radius_mean_same_words_as_smooth": same_smooth, "filter_window_stddev_crop_same_words_as_edges": same_edges},
        "host_route_mean_in_radius_3_cells": {"get_layer_ms": spread(t[:, 0]), "scipy_stand_in_not_grid_map_ms": spread(t[:, 1]),
                                              "set_layers_ms": spread(t[:, 2]), "total_ms": spread(t[:, 3])},
        "unmeasured": ["grid_map_filters itself (not built): no speed-up over its loops is claimed; the host stand-in is scipy's convolution, not grid_map",
                       "k_terr_main and k_terr_edges alone (lio_terrain_layers has no kernel clock): its whole call is given instead",
                       "the kernels under a profiler (event pairs only; no rocprofv3 pass, no counters, no LDS bank-conflict count)",
                       "grids beyond 220 k cells; more than one resident object filtered at a time; pinned host buffers for the host route"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    for o in (g, up):
        o.close()


if __name__ == "__main__":
    main()
