"""Cost of moving the resident planning layers into another frame on the device (lio_grid_transform) and of handing one out as
occupancy cells (lio_grid_to_occupancy): on the loader's grid (80 m x 90 m at 0.2 m: 400 x 450 = 180 000 cells, ten layers)
and on one small grid (67 x 45, ten layers), under a yaw alone and under a yaw with a tilt, with five samples a cell (ratio 0.25)
and with one (ratio 0); and the host path the call replaces: lio_grid_get_layer of every layer, a numpy scatter (the same key
folded by np.maximum.at, then a gather: already far from the reference's serial loop), lio_grid_set_layers of the result.

GPU time: HIP events, medians of --reps runs, the forms alternating.  The whole call is timed on the null stream around the
entry point (everything of the call runs there and it ends complete).  The stages are the call's own marks
(lio_grid_transform_debug_stage_ms: keys cleared, scatter kernel, gather kernel with the counters down).  Beside them the wall
time of the call on the host.  The host path is wall time, piece by piece.  No figure is a pass bar and none is a comparison
with grid_map, which is not built.

    python tools/grid_transform_cost.py [--reps 10] [--out profiles/grid_transform_cost.json]
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = {"loader_400x450": (400, 450, 0.2), "small_67x45": (67, 45, 0.2)}
N_LAYERS = 10
f32, u32, u64 = np.float32, np.uint32, np.uint64


def rot(yaw, pitch, t):
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    return np.array([[cy * cp, -sy, cy * sp, t[0]], [sy * cp, cy, sy * sp, t[1]], [-sp, 0.0, cp, t[2]]])


TRANSFORMS = {"yaw": rot(math.radians(30.0), 0.0, (3.0, -1.0, 0.0)), "yaw_tilt": rot(math.radians(30.0), math.radians(4.0), (3.0, -1.0, 0.2))}


def scene(rows, cols, res, rng):
    """rolling ground with a wall, steps and a tenth of the cells empty -> [N_LAYERS, rows, cols] float32"""
    x, y = np.meshgrid(np.arange(rows) * res, np.arange(cols) * res, indexing="ij")
    elev = (0.4 * np.sin(0.21 * x) * np.cos(0.13 * y) + 0.05 * rng.standard_normal((rows, cols))).astype(f32)
    elev[rows // 3, :] += 2.0
    elev[:, cols // 2:] += np.round(y[:, cols // 2:] / 6.0).astype(f32) * f32(0.15)
    elev[rng.random((rows, cols)) < 0.1] = np.nan
    return np.stack([elev] + [(np.nan_to_num(elev) * f32(k) + rng.uniform(0, 1, elev.shape).astype(f32)) for k in range(2, N_LAYERS + 1)])


def numpy_transform(layers, res, length, position, T, ratio, info):
    """the host path's middle: the key of lio_gridtransform.h per sample, np.maximum.at per new cell, the gather.  The new
    geometry is taken from the device call's info (it is a handful of fp64 operations)."""
    n_layers, rows, cols = layers.shape
    nr, nc = int(info["rows"]), int(info["cols"])
    nlen, npos = info["length"], info["position"]
    flat = np.stack([l.ravel(order="F") for l in layers])
    h = flat[0]
    lin = np.nonzero(np.isfinite(h))[0]
    r, c = lin % rows, lin // rows
    cx = position[0] + (0.5 * length[0] - 0.5 * res) + res * (-r).astype(np.float64)
    cy = position[1] + (0.5 * length[1] - 0.5 * res) + res * (-c).astype(np.float64)
    z = h[lin].astype(np.float64)
    sl = res * ratio
    offs = ((0.0, 0.0), (-sl, 0.0), (sl, 0.0), (0.0, -sl), (0.0, sl)) if ratio > 0.0 else ((0.0, 0.0),)
    keys = np.zeros(nr * nc, u64)
    for s, (dx, dy) in enumerate(offs):
        x, y = cx + dx, cy + dy
        tx, ty, tz = (((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3))
        inside = np.ones(len(lin), bool)
        idx = []
        for p, a, n in ((tx, 0, nr), (ty, 1, nc)):
            t = -((p - npos[a]) - 0.5 * nlen[a])
            inside &= (t >= 0.0) & (t < nlen[a])
            with np.errstate(invalid="ignore"):
                i = (-(((p - 0.5 * nlen[a]) - npos[a]) / res)).astype(np.int64)
            inside &= (i >= 0) & (i < n)
            idx.append(i)
        fz = tz.astype(f32)
        fz[fz == 0] = 0.0
        w = fz.view(u32)
        order = np.where(w & u32(0x80000000), ~w, w | u32(0x80000000)).astype(u64)
        visit = (5 * lin + s).astype(u64)
        low = np.where(tz >= fz.astype(np.float64), u64(0x80000000) | visit, u64(0x7fffffff) - visit)
        key = (order << u64(32)) | low
        np.maximum.at(keys, (idx[1] * nr + idx[0])[inside], key[inside])
    out = np.full((n_layers, nr * nc), np.nan, f32)
    hit = np.nonzero(keys)[0]
    low = keys[hit] & u64(0xffffffff)
    visit = np.where(low & u64(0x80000000), low & u64(0x7fffffff), u64(0x7fffffff) - low).astype(np.int64)
    src, s = visit // 5, visit % 5
    out[:, hit] = flat[:, src]
    dx = np.array([o[0] for o in offs])[s]
    dy = np.array([o[1] for o in offs])[s]
    x = position[0] + (0.5 * length[0] - 0.5 * res) + res * (-(src % rows)).astype(np.float64) + dx
    y = position[1] + (0.5 * length[1] - 0.5 * res) + res * (-(src // rows)).astype(np.float64) + dy
    out[0, hit] = (((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * flat[0, src].astype(np.float64)) + T[2, 3]).astype(f32)
    return out.reshape(n_layers, nc, nr).transpose(0, 2, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_transform_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_transform_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    rng = np.random.default_rng(1)
    stage = (C.c_float * 3)()
    grids, forms, host_rows = {}, {}, {}
    for gname, (rows, cols, res) in GRIDS.items():
        layers = scene(rows, cols, res, rng)
        length, position = (rows * res, cols * res), (12.0, -7.0)
        src, dst = pkg.Grid(), pkg.Grid()
        src.set_layers(layers, res, length, position)
        grids[gname] = (src, dst, layers, res, length, position)
        for tname, T in TRANSFORMS.items():
            for ratio in (0.25, 0.0):
                forms[f"transform_{gname}_{tname}_ratio{ratio}"] = (lambda src=src, dst=dst, T=T, ratio=ratio: src.transform(dst, T, 0, ratio))
        forms[f"to_occupancy_{gname}"] = (lambda src=src: src.to_occupancy(1, 0.0, 1.0) and None)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); info = fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_transform_debug_stage_ms(1, stage)
        return a.elapsed_time(b), wall, list(stage), info

    lib.lio_grid_transform_debug_stage_ms(1, None)
    samples, counts = {name: [] for name in forms}, {}
    for fn in forms.values():
        fn()                                                    # warm-up: the layers of dst, the pool, the code objects
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            ev, wall, st, info = timed(fn)
            samples[name].append((ev, wall, *st))
            if info is not None:
                counts[name] = {k: int(info[k]) for k in ("rows", "cols", "n_source_cells", "n_samples_outside", "n_cells_written")}
    lib.lio_grid_transform_debug_stage_ms(0, None)
    rows_out = {}
    for name, v in samples.items():
        med = np.median(np.array(v), axis=0)
        rows_out[name] = {"whole_call_ms": float(med[0]), "host_wall_ms": float(med[1])}
        if name.startswith("transform_"):
            rows_out[name].update({"keys_cleared_ms": float(med[2]), "scatter_kernel_ms": float(med[3]), "gather_kernel_and_counters_ms": float(med[4])})
        rows_out[name].update(counts.get(name, {}))
    # the host path the call replaces, on both grids under yaw_tilt with five samples
    for gname, (src, dst, layers, res, length, position) in grids.items():
        T, ratio = TRANSFORMS["yaw_tilt"], 0.25
        info = src.transform(dst, T, 0, ratio)
        device = np.stack([dst.layer(k) for k in range(N_LAYERS)])
        t = []
        for _ in range(max(3, args.reps // 2)):
            t0 = time.perf_counter()
            down = np.stack([src.layer(k) for k in range(N_LAYERS)])
            t1 = time.perf_counter()
            moved = numpy_transform(down, res, length, position, T, ratio, info)
            t2 = time.perf_counter()
            dst.set_layers(moved, res, tuple(info["length"]), tuple(info["position"]))
            t3 = time.perf_counter()
            t.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        med = np.median(np.array(t), axis=0)
        host_rows[f"host_path_{gname}_yaw_tilt_ratio0.25"] = {
            "get_layer_x10_ms": float(med[0]), "numpy_scatter_ms": float(med[1]), "set_layers_ms": float(med[2]), "total_ms": float(med[3]),
            "same_words_as_the_device": bool(np.array_equal(np.ascontiguousarray(moved).view(u32), np.ascontiguousarray(device).view(u32)))}
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "grids": GRIDS, "layers": N_LAYERS,
        "transforms": {k: v.tolist() for k, v in TRANSFORMS.items()},
        "clock": "HIP events: around the call on the null stream (whole call), between the call's own stages; medians.  Host path: perf_counter, medians",
        "calls": rows_out, "host_path": host_rows,
        "unmeasured": ["grid_map itself (not built): no speed-up over its serial loop is claimed; the host path here is vectorised numpy",
                       "the kernels under a profiler (event pairs only; no rocprofv3 pass, no counters)",
                       "steep pitches (many source cells per new cell: the atomics' worst case) beyond the 4 degree tilt",
                       "more than ten layers; grids beyond 180 k cells",
                       "pinned host buffers for the host path (pageable numpy arrays here)"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    for src, dst, *_ in grids.values():
        src.close(); dst.close()


if __name__ == "__main__":
    main()
