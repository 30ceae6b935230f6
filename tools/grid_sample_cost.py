"""Cost of sampling resident layers on the device (lio_grid_sample) on the terrain profile's 550 x 400 grid at 0.2 m: n = 10^3,
10^5 and 10^6 uniformly drawn positions (2 % of them outside the map), 1 and 4 layers, each of the four methods.

GPU time: HIP events, medians of --reps runs, the forms alternating.  The whole call is timed on the null stream around
lio_grid_sample (everything of the call runs there and it ends complete: positions up, kernel, values, method bytes and counts
down).  The kernel alone and the two copies alone are the call's own stage marks (lio_grid_debug_stage_ms: events recorded
between the stages of the same call).  Beside them: the wall time of the call on the host, and the single-thread time per
query of the same arithmetic on the host (tools/grid_sample_host_check.cpp built with -O2, passed in with --host-ns; it is
not measured here).  No figure is a pass bar and none is a comparison with grid_map, which is not built.

    python tools/grid_sample_cost.py [--reps 20] [--host-ns 27.0,52.4,119.4,179.4] [--out profiles/grid_sample_cost.json]
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
METHODS = ("nearest", "linear", "cubic_convolution", "cubic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-ns", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_sample_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_sample_cost.py needs a GPU (no CPU fallback)")
    import terrain_cost
    pkg = importlib.import_module("lio-slam_amd")
    lib = pkg.load_library()
    elev = terrain_cost.scene()
    elev = np.where(np.isfinite(elev), elev, np.float32(0.0)).astype(np.float32)      # (holes would only shorten the cubic paths)
    rng = np.random.default_rng(1)
    layers = np.stack([elev] + [(elev * np.float32(k) + rng.uniform(0, 1, elev.shape).astype(np.float32)) for k in (2, 3, 4)])
    grid = pkg.Grid()
    grid.set_layers(layers, RES, (ROWS * RES, COLS * RES), (0.0, 0.0))
    ids = {1: (C.c_int32 * 1)(0), 4: (C.c_int32 * 4)(0, 1, 2, 3)}
    stage = (C.c_float * 3)()
    forms, bufs = {}, {}
    for n in (10 ** 3, 10 ** 5, 10 ** 6):
        pos = np.c_[rng.uniform(-0.505 * ROWS * RES, 0.505 * ROWS * RES, n), rng.uniform(-0.505 * COLS * RES, 0.505 * COLS * RES, n)]
        bufs[n] = (np.ascontiguousarray(pos), np.empty(4 * n, np.float32), np.empty(4 * n, np.uint8))
        for n_layers in (1, 4):
            for m, name in enumerate(METHODS):
                def call(n=n, n_layers=n_layers, m=m):
                    cfg = pkg.grid_sample_default_config(method=m)
                    info = pkg.GridSampleInfo()
                    p, v, u = bufs[n]
                    rc = lib.lio_grid_sample(grid.h, ids[n_layers], n_layers, C.byref(cfg), p.ctypes.data, n, v.ctypes.data, u.ctypes.data, C.byref(info))
                    assert rc == 0, rc
                    return info
                forms[f"n{n}_layers{n_layers}_{name}"] = call

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(torch.cuda.default_stream()); info = fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        lib.lio_grid_debug_stage_ms(1, stage)
        return a.elapsed_time(b), wall, list(stage), info

    lib.lio_grid_debug_stage_ms(1, None)
    samples = {name: [] for name in forms}
    counts = {}
    for fn in forms.values():
        fn()                                                    # warm-up: the pool, the code objects
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            ev, wall, st, info = timed(fn)
            samples[name].append((ev, wall, *st))
            counts[name] = {"n_outside": info.n_outside, "n_method": list(info.n_method)}
    lib.lio_grid_debug_stage_ms(0, None)
    rows = {}
    for name, v in samples.items():
        med = np.median(np.array(v), axis=0)
        rows[name] = {"whole_call_ms": float(med[0]), "host_wall_ms": float(med[1]), "positions_up_ms": float(med[2]), "kernel_ms": float(med[3]),
                      "values_down_ms": float(med[4]), **counts[name]}
    host_ns = [float(x) for x in args.host_ns.split(",")] if args.host_ns else None
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": ROWS, "cols": COLS, "resolution": RES,
        "clock": "HIP events: around the call on the null stream (whole call), between the call's own stages (copies, kernel); medians",
        "calls": rows,
        "host_single_thread_ns_per_query": dict(zip(METHODS, host_ns)) if host_ns else "not given (--host-ns)",
        "unmeasured": ["grid_map itself (not built): no speed-up over it is claimed",
                       "the kernel under a profiler (event pairs only; no rocprofv3 pass, no counters)",
                       "the kernel clear of the upload: positions are a pageable host array, its staged copy is still draining when the mark "
                       "behind it is recorded, and at 10^5 and 10^6 positions the kernel's slice carries that tail (it barely differs between "
                       "nearest and cubic there): an upper bound",
                       "positions that follow a trajectory (uniform positions are the worst case for the tap loads' locality)",
                       "border_mode 1 and layers with holes (fall-back chains)",
                       "pinned host buffers for positions and values (pageable numpy arrays here)"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    grid.close()


if __name__ == "__main__":
    main()
