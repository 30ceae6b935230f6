"""Cost of reducing resident layers over regions on the device (lio_grid_region_reduce, lio_grid_region_cells) on the terrain
profile's 550 x 400 grid at 0.2 m: by kind (line, circle, ellipse, polygon), by layer count (1, 4, 10), by region count (10^3,
10^4, 10^5) and by region size (a 1.1 x 0.7 m footprint, 4 x 2 m, 20 x 10 m), regions drawn uniformly with uniform headings;
one region that covers the whole map (a single wave sweeps it: the known limit); and the only alternative a caller had before:
lio_grid_get_layer of the same layers (the host loop that follows it is the header's single-thread time, below).

GPU time: HIP events, medians of --reps runs, the forms alternating.  The whole call is timed on the null stream around the
entry point (everything of the call runs there and it ends complete).  The stages are the call's own marks
(lio_grid_region_debug_stage_ms: regions up, plan kernel, reduce kernel, results down).  Beside them: the wall time of the call
on the host, and the single-thread time per region of the same header on the host (tools/grid_region_host_check.cpp built with
-O2, passed in with --host-ns as line,circle,ellipse,polygon; one layer, plan + cells + reduction; it is not measured here).
No figure is a pass bar and none is a comparison with grid_map, which is not built.

    python tools/grid_region_cost.py [--reps 10] [--host-ns 1686,3354,21072,21050] [--out profiles/grid_region_cost.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS, COLS, RES = 550, 400, 0.2
KINDS = ("line", "circle", "ellipse", "polygon")
SIZES = {"footprint": (1.1, 0.7), "medium": (4.0, 2.0), "large": (20.0, 10.0)}


def regions_of(pkg, kind, n, size, rng):
    """n regions of one kind and size (length x width, m), centres uniform over 90 % of the map, headings uniform"""
    lx, ly = SIZES[size]
    x = rng.uniform(-0.45 * ROWS * RES, 0.45 * ROWS * RES, n)
    y = rng.uniform(-0.45 * COLS * RES, 0.45 * COLS * RES, n)
    yaw = rng.uniform(0, 2 * np.pi, n)
    if kind == "polygon":
        return pkg.footprint_polygons(np.c_[x, y, yaw], lx, ly)
    rec = np.zeros(n, pkg.GRID_REGION_DTYPE)
    if kind == "line":                                         # twice the length: some 40 cells at `medium`
        rec["kind"] = pkg.REGION_LINE
        rec["p"][:, 0], rec["p"][:, 1] = x, y
        rec["p"][:, 2], rec["p"][:, 3] = x + 2 * lx * np.cos(yaw), y + 2 * lx * np.sin(yaw)
    elif kind == "circle":                                     # radius = half the width
        rec["kind"] = pkg.REGION_CIRCLE
        rec["p"][:, 0], rec["p"][:, 1], rec["p"][:, 2] = x, y, 0.5 * ly
    else:
        rec["kind"] = pkg.REGION_ELLIPSE
        rec["p"][:, 0], rec["p"][:, 1], rec["p"][:, 2], rec["p"][:, 3], rec["p"][:, 4] = x, y, lx, ly, yaw
    return rec, np.zeros((0, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-ns", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_region_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_region_cost.py needs a GPU (no CPU fallback)")
    import terrain_cost
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    elev = terrain_cost.scene()
    elev = np.where(np.isfinite(elev), elev, np.float32(0.0)).astype(np.float32)
    rng = np.random.default_rng(1)
    layers = np.stack([elev] + [(elev * np.float32(k) + rng.uniform(0, 1, elev.shape).astype(np.float32)) for k in range(2, 11)])
    grid = pkg.Grid()
    grid.set_layers(layers, RES, (ROWS * RES, COLS * RES), (0.0, 0.0))
    ids = {k: (C.c_int32 * k)(*range(k)) for k in (1, 4, 10)}
    stage = (C.c_float * 4)()
    cases = [(kind, 10 ** 4, 1, "medium") for kind in KINDS]
    cases += [("polygon", n, k, "medium") for n in (10 ** 3, 10 ** 4, 10 ** 5) for k in (1, 4, 10) if (n, k) != (10 ** 4, 1)]
    cases += [("polygon", 10 ** 4, 4, "footprint"), ("polygon", 10 ** 4, 4, "large")]
    forms = {}
    for kind, n, k, size in cases:
        rec, verts = regions_of(pkg, kind, n, size, rng)
        verts = np.ascontiguousarray(verts, np.float64)
        out = (np.zeros((k, n), pkg.GRID_REGION_STAT_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.uint8))

        def call(rec=rec, verts=verts, n=n, k=k, out=out):
            cfg = pkg.grid_region_default_config()
            info = pkg.GridRegionInfo()
            rc = lib.lio_grid_region_reduce(grid.h, ids[k], k, C.byref(cfg), rec.ctypes.data, n, verts.ctypes.data, len(verts), out[0].ctypes.data,
                                            out[1].ctypes.data, out[2].ctypes.data, C.byref(info))
            assert rc == 0, rc
            return info
        forms[f"reduce_{kind}_n{n}_layers{k}_{size}"] = call
    h = 0.5 * ROWS * RES + 1.0
    w = 0.5 * COLS * RES + 1.0
    whole, wverts = pkg.pack_regions([("polygon", ((h, w), (-h, w), (-h, -w), (h, -w)))])
    for k in (1, 10):
        out = (np.zeros((k, 1), pkg.GRID_REGION_STAT_DTYPE), np.zeros(1, np.int32), np.zeros(1, np.uint8))

        def call(k=k, out=out):
            cfg = pkg.grid_region_default_config()
            info = pkg.GridRegionInfo()
            rc = lib.lio_grid_region_reduce(grid.h, ids[k], k, C.byref(cfg), whole.ctypes.data, 1, wverts.ctypes.data, 4, out[0].ctypes.data, out[1].ctypes.data,
                                            out[2].ctypes.data, C.byref(info))
            assert rc == 0 and info.n_cells == ROWS * COLS, (rc, info.n_cells)
            return info
        forms[f"reduce_whole_map_one_region_layers{k}"] = call
    rec, verts = regions_of(pkg, "polygon", 10 ** 4, "medium", rng)
    verts = np.ascontiguousarray(verts, np.float64)
    offsets, cells = np.zeros(10 ** 4 + 1, np.int64), np.zeros(10 ** 4 * 260, np.int32)

    def call_cells():
        info = pkg.GridRegionInfo()
        rc = lib.lio_grid_region_cells(grid.h, rec.ctypes.data, len(rec), verts.ctypes.data, len(verts), offsets.ctypes.data, cells.ctypes.data, cells.size, None,
                                       C.byref(info))
        assert rc == 0, rc
        return info
    forms["cells_polygon_n10000_medium"] = call_cells
    host = np.zeros(ROWS * COLS, np.float32)
    for k in (1, 4, 10):
        def call_get(k=k):
            for layer in range(k):
                assert lib.lio_grid_get_layer(grid.h, layer, host.ctypes.data, host.size) == 0
            return None
        forms[f"get_layer_x{k}"] = call_get

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); info = fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_region_debug_stage_ms(1, stage)
        return a.elapsed_time(b), wall, list(stage), info

    lib.lio_grid_region_debug_stage_ms(1, None)
    samples = {name: [] for name in forms}
    counts = {}
    for fn in forms.values():
        fn()                                                    # warm-up: the workspace, the code objects
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            ev, wall, st, info = timed(fn)
            samples[name].append((ev, wall, *st))
            if info is not None:
                counts[name] = {"n_ok": info.n_ok, "n_empty": info.n_empty, "n_cells": info.n_cells}
    lib.lio_grid_region_debug_stage_ms(0, None)
    rows = {}
    for name, v in samples.items():
        med = np.median(np.array(v), axis=0)
        rows[name] = {"whole_call_ms": float(med[0]), "host_wall_ms": float(med[1])}
        if name.startswith("reduce_"):                          # (the marks are lio_grid_region_reduce's alone)
            rows[name].update({"regions_up_ms": float(med[2]), "plan_kernel_ms": float(med[3]), "reduce_kernel_ms": float(med[4]), "results_down_ms": float(med[5])})
        rows[name].update(counts.get(name, {}))
    host_ns = [float(x) for x in args.host_ns.split(",")] if args.host_ns else None
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": ROWS, "cols": COLS, "resolution": RES, "sizes_m": SIZES,
        "clock": "HIP events: around the call on the null stream (whole call), between the call's own stages (copies, kernels); medians",
        "calls": rows,
        "host_single_thread_ns_per_region_medium_1_layer": dict(zip(KINDS, host_ns)) if host_ns else "not given (--host-ns)",
        "unmeasured": ["grid_map itself (not built): no speed-up over it is claimed",
                       "the kernels under a profiler (event pairs only; no rocprofv3 pass, no counters)",
                       "the plan kernel clear of the upload: the regions are a pageable host array, and its staged copy can still be draining "
                       "when the mark behind it is recorded: an upper bound",
                       "regions that follow a trajectory (uniform centres are the worst case for the gathers' locality)",
                       "lines whose ends lie far outside the map (the walk is up to 4096 serial steps a lane)",
                       "pinned host buffers for regions and results (pageable numpy arrays here)"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    grid.close()


if __name__ == "__main__":
    main()
