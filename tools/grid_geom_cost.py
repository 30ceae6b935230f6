"""Cost of cropping, moving, extending and merging the resident planning layers on the device (lio_grid_submap, lio_grid_move,
lio_grid_extend_to_include, lio_grid_add_data_from) on the loader's grid (80 m x 90 m at 0.2 m: 400 x 450 = 180 000 cells, ten
layers): each entry whole and by its kernel, a device-to-device copy of the same bytes (ten layers read, ten written) in the
same run, and the host route the entries replace: lio_grid_get_layer of every layer, a numpy slice copy, lio_grid_set_layers.

GPU time: HIP events, medians of --reps runs, the forms alternating.  The whole call is timed on the null stream around the
entry point (everything of the call runs there and it ends complete); the kernel is the call's own pair of marks
(lio_grid_geom_debug_kernel_ms); beside them the wall time of the call on the host.  A call that changes its map (move, extend,
add) is given the same map again before each run, outside the timed part.  The host route is wall time, piece by piece.  No
figure is a pass bar and none is a comparison with grid_map, which is not built.

    python tools/grid_geom_cost.py [--reps 10] [--out profiles/grid_geom_cost.json]
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

ROWS, COLS, RES, N_LAYERS = 400, 450, 0.2, 10
f32 = np.float32


def scene(rows, cols, rng):
    a = rng.uniform(-1.0, 1.0, (N_LAYERS, rows, cols)).astype(f32)
    a[0][rng.random((rows, cols)) < 0.1] = np.nan
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_geom_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_geom_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    length, position = (ROWS * RES, COLS * RES), (12.0, -7.0)
    layers = scene(ROWS, COLS, rng)
    g, dst = pkg.Grid(), pkg.Grid()
    inside, corner = pkg.Grid(), pkg.Grid()
    inside.set_layers(scene(200, 225, rng), RES, (200 * RES, 225 * RES), (position[0] + 3.07, position[1] - 1.13))
    corner.set_layers(scene(200, 225, rng), RES, (200 * RES, 225 * RES), (position[0] + 35.07, position[1] - 40.13))

    def restore():
        g.set_layers(layers, RES, length, position)

    forms = {
        "submap_half_200x225": lambda: g.submap(dst, position, (40.0, 45.0)),
        "submap_whole_400x450": lambda: g.submap(dst, position, (1e3, 1e3)),
        "move_7_-3_cells": lambda: g.move((position[0] + 7 * RES, position[1] - 3 * RES)),
        "move_whole_map_away": lambda: g.move((position[0] + 500 * RES, position[1])),
        "extend_to_include_corner": lambda: g.extend_to_include(corner),
        "add_extend_resize_corner": lambda: g.add_data_from(corner, True, True, None, (0,)),
        "add_in_place_inside": lambda: g.add_data_from(inside, False, True, None, (0,)),
        "add_in_place_inside_keep_valid": lambda: g.add_data_from(inside, False, False, None, (0,)),
    }
    ms = C.c_float()

    def timed(fn):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); info = fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_geom_debug_kernel_ms(1, C.byref(ms))
        return a.elapsed_time(b), wall, ms.value, info

    # the plain copy: ten layers read, ten written
    n_bytes = N_LAYERS * ROWS * COLS * 4
    src_t, dst_t = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

    def copy_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); dst_t.copy_(src_t); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    lib.lio_grid_geom_debug_kernel_ms(1, None)
    for fn in forms.values():                                   # warm-up: the pool's blocks, dst's layers, the code objects
        restore()
        fn()
    copy_ms()
    samples, copies, infos = {name: [] for name in forms}, [], {}
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            ev, wall, kernel, info = timed(fn)
            samples[name].append((ev, wall, kernel))
            infos[name] = {k: (info[k].tolist() if hasattr(info[k], "tolist") else info[k]) for k in info.dtype.names if k != "pad"}
        copies.append(copy_ms())
    lib.lio_grid_geom_debug_kernel_ms(0, None)
    copy = float(np.median(copies))
    calls = {}
    for name, v in samples.items():
        med = np.median(np.array(v), axis=0)
        cells = infos[name].get("rows", ROWS) * infos[name].get("cols", COLS) if "rows" in infos[name] else ROWS * COLS
        calls[name] = {"whole_call_ms": float(med[0]), "host_wall_ms": float(med[1]), "kernel_ms": float(med[2]),
                       "kernel_over_copy_of_7p2_MB": float(med[2] / copy) if copy > 0 else None, "cells_written_per_layer": int(cells), "info": infos[name]}
    # the host route, for the move by (7, -3) cells
    t = []
    for _ in range(max(3, args.reps // 2)):
        restore()
        t0 = time.perf_counter()
        down = np.stack([g.layer(k) for k in range(N_LAYERS)])
        t1 = time.perf_counter()
        moved = np.full_like(down, np.nan)
        moved[:, 7:, :COLS - 3] = down[:, :ROWS - 7, 3:]        # new (r, c) = old (r - 7, c + 3): the index shift is (-7, 3)
        t2 = time.perf_counter()
        g.set_layers(moved, RES, length, (position[0] + 7 * RES, position[1] - 3 * RES))
        t3 = time.perf_counter()
        t.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
    med = np.median(np.array(t), axis=0)
    restore()
    g.move((position[0] + 7 * RES, position[1] - 3 * RES))
    same = all(np.array_equal(g.layer(k).view(np.uint32), moved[k].view(np.uint32)) for k in range(N_LAYERS))
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "grid": [ROWS, COLS, RES], "layers": N_LAYERS,
        "clock": "HIP events: around the call on the null stream (whole call), around the call's kernel; medians.  Host route: perf_counter, medians",
        "device_to_device_copy_7p2_MB_ms": copy, "calls": calls,
        "host_route_move": {"get_layer_x10_ms": float(med[0]), "numpy_slice_copy_ms": float(med[1]), "set_layers_ms": float(med[2]),
                            "total_ms": float(med[3]), "same_words_as_the_device": bool(same)},
        "unmeasured": ["grid_map itself (not built): no speed-up over its loops is claimed; the host route here is a numpy slice copy",
                       "the kernels under a profiler (event pairs only; no rocprofv3 pass, no counters)",
                       "more than ten layers; grids beyond 180 k cells; other's resolution different from the map's",
                       "pinned host buffers for the host route (pageable numpy arrays here)"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    for o in (g, dst, inside, corner):
        o.close()


if __name__ == "__main__":
    main()
