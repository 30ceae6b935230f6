"""Cost of lio_grid_filter_expression on the 550 x 400 grid at 0.2 m (220 000 cells) of tools/grid_filter_cost.py: a 1-op
expression (`a`), the demo chain's traversability expression, a 40-op expression, and expressions with one, two and four
map-wide reductions, whose walker runs in one workgroup.  Each call whole and its two stages alone (the reduction passes together,
the storing pass), and three comparisons in the same run:
  - a device-to-device copy of one layer's bytes (one layer read, one written): the floor of a call that derives a layer;
  - lio_terrain_layers on the same grid, whose main kernel hard-wires the traversability expression among its other layers;
  - the host route the call replaces for the traversability expression: two lio_grid_get_layer, numpy float32 arithmetic,
    lio_grid_set_layers of the result; and lio_debug_grid_expression_host, the interpreter on one host thread.

GPU time: HIP events, medians of --reps runs with their quartiles, the forms alternating.  The whole call is timed on the null
stream around the entry point; the stages are the call's own marks (lio_grid_expression_debug_kernel_ms).  The host route is wall
time.  No figure is a pass bar and none is a comparison with grid_map, which is not built.

    python tools/grid_expression_cost.py [--reps 20] [--out profiles/grid_expression_cost.json]
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
TRAVERSABILITY = "0.5 * (1.0 - (slope / 0.6)) + 0.5 * (1.0 - (roughness / 0.1))"
NAMES = {"slope": 0, "roughness": 1}
FORTY = " + ".join(["abs(slope - roughness)"] * 7) + " - slope .* roughness + 1"         # 40 instructions: 7 x 4, 6 sums, 4 and 2 more
EXPRESSIONS = {
    "one_op_copy": "slope",
    "traversability_15_ops": TRAVERSABILITY,
    "forty_ops": FORTY,
    "acos": "acos(roughness)",
    "exp_fp64_route": "exp(roughness)",
    "one_reduction_minus_mean": "slope - meanOfFinites(slope)",
    "two_reductions_normalise": "(slope - minOfFinites(slope)) / maxOfFinites(slope)",
    "four_reductions_standard_score": "(slope - meanOfFinites(slope)) / sqrt(sumOfFinites(square(slope - meanOfFinites(slope))) ./ numberOfFinites(slope))",
}


def spread(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median": float(q[1]), "q25": float(q[0]), "q75": float(q[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_expression_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_expression_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    length, position = (ROWS * RES, COLS * RES), (12.0, -7.0)
    slope = rng.uniform(0.0, 0.9, (ROWS, COLS)).astype(f32)
    rough = rng.uniform(0.0, 0.15, (ROWS, COLS)).astype(f32)
    for z in (slope, rough):
        z[rng.random((ROWS, COLS)) < 0.08] = np.nan
    g, up = pkg.Grid(), pkg.Grid()
    g.set_layers([slope, rough], RES, length, position)
    compiled = {name: pkg.grid_expression_check(e, NAMES) for name, e in EXPRESSIONS.items()}
    assert compiled["forty_ops"]["n_ops"] == 40 and compiled["one_op_copy"]["n_ops"] == 1
    ms = (C.c_float * 2)()

    def timed(e):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); info = g.filter_expression(e, NAMES, 2); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_expression_debug_kernel_ms(1, ms)
        return a.elapsed_time(b), wall, ms[0], ms[1], info

    n_bytes = ROWS * COLS * 4
    src_t, dst_t = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

    def copy_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); dst_t.copy_(src_t); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    x, y = np.arange(ROWS)[:, None] * RES, np.arange(COLS)[None, :] * RES
    z = (0.08 * x - 0.05 * y + 0.3 * np.sin(0.7 * x) * np.cos(0.4 * y) + rng.normal(0, 0.01, (ROWS, COLS))).astype(f32)
    z[rng.random((ROWS, COLS)) < 0.08] = np.nan
    cfg_none = pkg.terrain_default_config(normal_method=1, smooth_radius=0.6, edge_window_length=0.5, layers=0)
    zf = np.asfortranarray(z)
    ln, ps = (C.c_double * 2)(*length), (C.c_double * 2)(*position)
    tinfo = pkg.TerrainInfo()

    def terrain():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(torch.cuda.default_stream())
        rc = lib.lio_terrain_layers(0, zf.ctypes.data, ROWS, COLS, RES, ln, ps, C.byref(cfg_none), None, 0, C.byref(tinfo))
        b.record(torch.cuda.default_stream())
        b.synchronize()
        assert rc == 0, lib.lio_last_error()
        return a.elapsed_time(b)

    lib.lio_grid_expression_debug_kernel_ms(1, None)
    for e in EXPRESSIONS.values():                              # warm-up: the pool's blocks, the layer, the code objects
        g.filter_expression(e, NAMES, 2)
    copy_ms(); terrain()
    samples, copies, t_terrain, infos = {name: [] for name in EXPRESSIONS}, [], [], {}
    for _ in range(args.reps):
        for name, e in EXPRESSIONS.items():                     # alternating
            ev, wall, reduce_ms, store_ms, info = timed(e)
            samples[name].append((ev, wall, reduce_ms, store_ms))
            infos[name] = {k: int(info[k]) for k in info.dtype.names}
        copies.append(copy_ms())
        t_terrain.append(terrain())
    lib.lio_grid_expression_debug_kernel_ms(0, None)
    copy = spread(copies)
    calls = {}
    for name, v in samples.items():
        v = np.array(v)
        n_reduce = infos[name]["n_passes"] - 1
        calls[name] = {"expression": EXPRESSIONS[name], "whole_call_ms": spread(v[:, 0]), "host_wall_ms": spread(v[:, 1]), "reduction_passes_ms": spread(v[:, 2]),
                       "reduction_walker_ms_per_pass": float(np.median(v[:, 2]) / n_reduce) if n_reduce else None, "storing_pass_ms": spread(v[:, 3]),
                       "storing_pass_over_copy_of_one_layer": float(np.median(v[:, 3]) / copy["median"]) if copy["median"] > 0 else None, "info": infos[name]}

    # the host routes for the traversability expression
    t = []
    for _ in range(max(3, args.reps // 2)):
        t0 = time.perf_counter()
        s, r = g.layer(0), g.layer(1)
        t1 = time.perf_counter()
        with np.errstate(all="ignore"):
            out = f32(0.5) * (f32(1.0) - s / f32(0.6)) + f32(0.5) * (f32(1.0) - r / f32(0.1))
        t2 = time.perf_counter()
        up.set_layers([out], RES, length, position)
        t3 = time.perf_counter()
        pkg.grid_expression_host(TRAVERSABILITY, ["slope", "roughness"], np.stack([s, r]))
        t4 = time.perf_counter()
        t.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3, (t4 - t3) * 1e3))
    t = np.array(t)
    g.filter_expression(TRAVERSABILITY, NAMES, 2)
    got = g.layer(2)
    same = bool(np.array_equal(np.isnan(got), np.isnan(out)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), out[~np.isnan(out)].view(np.uint32)))
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "grid": [ROWS, COLS, RES], "cells": ROWS * COLS,
        "clock": "HIP events: around the call on the null stream (whole call), around the call's reduction passes and its storing pass; medians with "
                 "quartiles over the alternating runs.  Host route: perf_counter",
        "device_to_device_copy_of_one_layer_0p88_MB_ms": copy, "calls": calls,
        "lio_terrain_layers_same_grid_no_layer_to_host_ms": spread(t_terrain),
        "host_route_traversability": {"get_two_layers_ms": spread(t[:, 0]), "numpy_float32_ms": spread(t[:, 1]), "set_layers_ms": spread(t[:, 2]),
                                      "total_ms": spread(t[:, 3]), "same_words_as_the_device": same,
                                      "interpreter_on_one_host_thread_with_the_wrapper_copies_ms": spread(t[:, 4])},
        "unmeasured": ["grid_map_filters' MathExpressionFilter itself (not built): no speed-up over EigenLab is claimed",
                       "the kernels under a profiler (event pairs only; no rocprofv3 pass, no counters, no LDS bank-conflict count)",
                       "a register-resident stack or a specialised kernel per expression: the interpreter is the only form",
                       "a reduction walker over more than one workgroup (a segmented scan cannot keep the serial order of the float sums)",
                       "grids beyond 220 k cells; several expressions fused into one launch"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    for o in (g, up):
        o.close()


if __name__ == "__main__":
    main()
