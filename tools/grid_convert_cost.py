"""Cost of handing resident planning layers out as images, clouds and grid cells and of taking images and occupancy grids in
(lio_grid_to_image, lio_grid_add_layer_from_image, lio_grid_from_occupancy, lio_grid_to_point_cloud, lio_grid_to_grid_cells,
lio_sdf_to_point_cloud) on the loader's grid (80 m x 90 m at 0.2 m: 400 x 450 cells) and on 64 x 64: each call whole and by its
stages, the image kernels in their direct form (what the entries run) and in their LDS-tiled form, and beside each call the
host route it replaces: lio_grid_get_layer (or lio_sdf_nodes) plus the numpy restatement of the loop (tests/grid_convert_restate.py's arithmetic,
written out here so that the tool needs nothing but the library).

GPU time: HIP events, medians of --reps runs, the forms alternating.  The whole call is timed on the null stream around the
entry point (everything of the call runs there and it ends complete); with --stage (the default) the call's own marks
(lio_grid_convert_debug_stage_ms) split it into first stage (extremes / count and scan / image up), second stage (image kernel /
emit / ingest kernel) and the result down.  The host route is wall time.  No figure is a pass bar and none is a comparison with
grid_map, which is not built.

    python tools/grid_convert_cost.py [--reps 10] [--no-stage] [--out profiles/grid_convert_cost.json]
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

GRIDS = {"loader_400x450": (400, 450, 0.2), "small_64x64": (64, 64, 0.2)}
f32 = np.float32


def host_to_image_8uc1(layer, lo, hi):
    v = np.where(layer < lo, lo, np.where(layer > hi, hi, layer)).astype(f32)
    ok = np.isfinite(v)
    img = np.zeros(layer.shape, np.uint8)
    with np.errstate(all="ignore"):
        img[ok] = np.trunc(((v[ok] - lo) / f32(hi - lo)) * f32(255.0)).astype(np.uint8)
    return img


def host_cloud(layers, res, length, position):
    rows, cols = layers[0].shape
    x = position[0] + (0.5 * length[0] - 0.5 * res) + res * -np.arange(rows, dtype=np.float64)
    y = position[1] + (0.5 * length[1] - 0.5 * res) + res * -np.arange(cols, dtype=np.float64)
    flat = [l.ravel(order="F") for l in layers]
    keep = np.isfinite(flat[0])
    return np.stack([np.tile(x, cols).astype(f32), np.repeat(y, rows).astype(f32)] + flat, axis=1)[keep]


def host_field_cloud(nodes, origin, res, lo, hi):
    layers, cols, rows = nodes.shape[:3]
    d = nodes[..., 0]
    keep = (d >= lo) & (d <= hi)
    z, y, x = np.nonzero(keep)
    return np.stack([(origin[0] - x * res).astype(f32), (origin[1] - y * res).astype(f32), (origin[2] + z * res).astype(f32), d[keep]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stage", action=argparse.BooleanOptionalAction, default=True, help="split each call by the library's own stage marks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_convert_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_convert_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    ms = (C.c_float * 3)()
    tiled = [0]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_convert_debug_stage_ms(1 if args.stage else 0, tiled[0], ms)
        return [a.elapsed_time(b), wall] + list(ms)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "stage_marks": bool(args.stage), "grids": {},
           "clock": "HIP events around the call on the null stream (whole call) and the call's own marks (stages); medians.  Host route: perf_counter, medians",
           "columns": ["whole_call_ms", "host_wall_ms", "stage1_ms", "stage2_ms", "down_ms"]}
    rng = np.random.default_rng(1)
    for name, (rows, cols, cell) in GRIDS.items():
        length, position = (rows * cell, cols * cell), (12.0, -7.0)
        height = rng.uniform(-1.0, 1.0, (rows, cols)).astype(f32)
        height[rng.random((rows, cols)) < 0.1] = np.nan
        layers = np.stack([height, rng.uniform(0, 1, (rows, cols)).astype(f32), rng.uniform(0, 1, (rows, cols)).astype(f32)])
        g, back = pkg.Grid(), pkg.Grid()
        g.set_layers(layers, cell, length, position)
        img8 = g.to_image(0, 1, pkg.IMAGE_8U, -1.0, 1.0)[0]
        img4 = g.to_image(0, 4, pkg.IMAGE_8U, -1.0, 1.0)[0]
        occ = g.to_occupancy(1, 0.0, 1.0)[0]
        sdf = pkg.Sdf()
        info = sdf.build(np.nan_to_num(height, nan=0.0), cell, length, position, pkg.sdf_default_config(min_height=-1.0, max_height=1.0))
        origin = tuple(info.origin)
        n_cloud, n_cells, n_field = len(g.to_point_cloud(0, [0, 1, 2])), len(g.to_grid_cells(0, -0.1, 0.1)), len(sdf.to_point_cloud(1, -0.1, 0.1))
        forms = {
            "to_image_8UC1": lambda: g.to_image(0, 1, pkg.IMAGE_8U, -1.0, 1.0),
            "to_image_8UC1_automatic_bounds": lambda: g.to_image(0, 1, pkg.IMAGE_8U),
            "to_image_8UC4": lambda: g.to_image(0, 4, pkg.IMAGE_8U, -1.0, 1.0),
            "to_image_16UC1": lambda: g.to_image(0, 1, pkg.IMAGE_16U, -1.0, 1.0),
            "to_image_32FC1": lambda: g.to_image(0, 1, pkg.IMAGE_32F, -1.0, 1.0),
            "add_layer_from_image_8UC1": lambda: g.add_layer_from_image(5, img8, -1.0, 1.0),
            "add_layer_from_image_8UC4": lambda: g.add_layer_from_image(5, img4, -1.0, 1.0),
            "from_occupancy": lambda: back.from_occupancy(0, occ, rows, cols, cell, (0.0, 0.0)),
            "to_point_cloud_5_fields": lambda: g.to_point_cloud(0, [0, 1, 2], cap_points=n_cloud),
            "to_grid_cells": lambda: g.to_grid_cells(0, -0.1, 0.1, cap_cells=n_cells),
            "sdf_to_point_cloud_near_surface": lambda: sdf.to_point_cloud(1, -0.1, 0.1, cap_points=n_field),
        }
        image_forms = [k for k in forms if "image" in k]
        lib.lio_grid_convert_debug_stage_ms(1 if args.stage else 0, 0, None)
        for fn in forms.values():                              # warm-up: the pool's blocks, the code objects
            fn()
        samples = {(k, d): [] for k in forms for d in ((0, 1) if k in image_forms else (0,))}
        for _ in range(args.reps):
            for (k, d) in samples:                             # alternating, the direct form (the path) and the tiled one side by side
                tiled[0] = d
                lib.lio_grid_convert_debug_stage_ms(1 if args.stage else 0, d, None)
                samples[(k, d)].append(timed(forms[k]))
        tiled[0] = 0
        lib.lio_grid_convert_debug_stage_ms(0, 0, None)
        calls = {}
        for (k, d), v in samples.items():
            a = np.array(v)
            calls[k + ("_tiled_form" if d else "")] = {"median": np.median(a, axis=0).round(4).tolist(), "min": a.min(axis=0).round(4).tolist(),
                                                        "max": a.max(axis=0).round(4).tolist()}
        lo, hi = f32(-1.0), f32(1.0)
        n = max(3, args.reps // 2)
        host = {
            "image_8UC1: get_layer + numpy": float(np.median([wall_ms(lambda: host_to_image_8uc1(g.layer(0), lo, hi)) for _ in range(n)])),
            "point_cloud: get_layer x3 + numpy": float(np.median([wall_ms(lambda: host_cloud([g.layer(k) for k in range(3)], cell, length, position))
                                                                   for _ in range(n)])),
            "field_cloud: sdf_nodes + numpy": float(np.median([wall_ms(lambda: host_field_cloud(sdf.nodes(), origin, info.resolution, f32(-0.1), f32(0.1)))
                                                                for _ in range(n)])),
        }
        same = bool(np.array_equal(host_to_image_8uc1(g.layer(0), lo, hi), img8[:, :, 0]) and
                    np.array_equal(host_cloud([g.layer(k) for k in range(3)], cell, length, position).view(np.uint32),
                                   g.to_point_cloud(0, [0, 1, 2]).view(np.uint32)) and
                    np.array_equal(host_field_cloud(sdf.nodes(), origin, info.resolution, f32(-0.1), f32(0.1)).view(np.uint32),
                                   sdf.to_point_cloud(1, -0.1, 0.1).view(np.uint32)))
        res["grids"][name] = {"rows": rows, "cols": cols, "field_nodes": int(info.rows * info.cols * info.layers), "survivors": {"point_cloud": n_cloud,
                              "grid_cells": n_cells, "field_cloud": n_field}, "bytes_down": {"image_8UC1": rows * cols, "float_layer": 4 * rows * cols,
                              "field_cloud": 16 * n_field, "sdf_nodes": 16 * int(info.rows * info.cols * info.layers)},
                              "calls": calls, "host_route_wall_ms": host, "host_route_same_words_as_the_device": same}
        for o in (g, back, sdf):
            o.close()
    res["unmeasured"] = ["grid_map itself (not built): no speed-up over its loops is claimed; the host route here is numpy on pageable arrays",
                         "the kernels under a profiler (event pairs only; no rocprofv3 pass, no counters, no LDS bank-conflict count)",
                         "grids beyond 180 k cells; more than five fields; 16U and 32F colour images"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
