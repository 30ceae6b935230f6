"""Cost of the planner's occupancy grid on the device (lio_kf_store_occupancy_grid) on a synthetic saved map: the bench's 200
keyframes (64x1800 sweeps, voxel 0.4) under their poses, filtered at save_map's resolution 0.2, then the draft's chain at its
defaults (slice 0.2 .. 2.0 m, radius 0.5 m / 10 neighbours, 0.05 m cells).

GPU time: the chain's stages by HIP events the library records on the chain's own stream at the stage boundaries
(lio_ogm_debug_stage_ms): the slice, the filter split into grid build, search and compaction, the raster, the grid's copy to
the host.  The whole call -- which also builds the map: export tables, world-frame sum, voxel filter -- by the host's wall
clock around it (it ends complete: it waits for its stream).  Medians of --reps runs, the forms alternating: the call with
the grid, without it (grid == NULL), without the filter, and lio_occupancy_grid on the same cloud from the host.  Host
stand-in: numpy for the slice and the raster, scipy.spatial.cKDTree.query_ball_point for the counts, wall clock.  It is NOT
PCL and is reported, not judged; no speed-up over PCL is claimed.

    python tools/ogm_cost.py [--reps 20] [--out profiles/ogm_cost.json]
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

STAGES = ("slice_ms", "filter_grid_build_ms", "filter_search_ms", "filter_compaction_ms", "raster_ms", "grid_copy_ms")


def host_stand_in(cloud, cfg):
    """numpy slice, cKDTree counts, numpy raster (as written) -> (seconds per stage, occupied cells)"""
    from scipy.spatial import cKDTree
    t = [time.perf_counter()]
    xyz = cloud[:, :3]
    ok = np.isfinite(xyz).all(axis=1) & (xyz[:, 2] >= cfg.z_min) & (xyz[:, 2] <= cfg.z_max)
    sl = xyz[ok]
    t.append(time.perf_counter())
    tree = cKDTree(sl.astype(np.float64))
    t.append(time.perf_counter())
    k = tree.query_ball_point(sl.astype(np.float64), float(cfg.radius), return_length=True, workers=1)
    inl = sl[k > cfg.min_neighbors]
    t.append(time.perf_counter())
    x, y = inl[:, 0].astype(np.float64), inl[:, 1].astype(np.float64)
    x0, x1, y0, y1 = x[:-1].min(), x[:-1].max(), y[:-1].min(), y[:-1].max()
    w, h = int((x1 - x0) / cfg.resolution), int((y1 - y0) / cfg.resolution)
    i, j = np.trunc((x - x0) / cfg.resolution).astype(np.int64), np.trunc((y - y0) / cfg.resolution).astype(np.int64)
    keep = (i >= 0) & (i < w) & (j >= 0) & (j < h - 1)
    grid = np.zeros((h, w), np.int8)
    grid[j[keep], i[keep]] = 100
    t.append(time.perf_counter())
    d = np.diff(t)
    return {"slice_ms": 1e3 * d[0], "kdtree_build_ms": 1e3 * d[1], "radius_counts_ms": 1e3 * d[2], "raster_ms": 1e3 * d[3],
            "total_ms": 1e3 * (t[-1] - t[0])}, int((grid == 100).sum()), len(sl), len(inl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--sensor", default="hdl64")
    ap.add_argument("--map-resolution", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ogm_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ogm_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    lib = pkg.load_library()
    case = synth.make_case(args.sensor, n_keyframes=args.keyframes, seed=synth.BASE_SEED, device="cuda", with_map=True)
    clouds = [np.concatenate([c, np.full((len(c), 1), float(k % 255), np.float32)], 1).astype(np.float32)
              for k, (c, _) in enumerate(case["keyframes"])]
    poses = np.array([p for _, p in case["keyframes"]], np.float32)
    st = pkg.KeyframeStore()
    for c in clouds:
        st.add(c)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    cfg = pkg.ogm_default_config()
    no_filter = pkg.ogm_default_config(remove_outliers=0)
    _, saved, _ = st.export_map(args.map_resolution, want_full=False)          # the saved map, for the host forms
    xyz = np.ascontiguousarray(saved[:, :3])
    _, info0, n_map = st.occupancy_grid(args.map_resolution, cfg, want_grid=False)
    _, info1, _ = st.occupancy_grid(args.map_resolution, no_filter, want_grid=False)        # (without the filter the box is larger)
    cells = info0.width * info0.height
    grid = np.zeros(max(cells, info1.width * info1.height, 1), np.int8)
    info, n_map_c = pkg.OgmInfo(), C.c_size_t()
    ms = (C.c_float * 6)()

    def store_call(c, with_grid=True):
        rc = lib.lio_kf_store_occupancy_grid(st.h, args.map_resolution, C.byref(c), grid.ctypes.data if with_grid else None, grid.size,
                                             C.byref(n_map_c), C.byref(info))
        assert rc == 0, rc

    def host_call():
        rc = lib.lio_occupancy_grid(0, xyz.ctypes.data, len(xyz), 12, C.byref(cfg), grid.ctypes.data, grid.size, C.byref(info))
        assert rc == 0, rc

    forms = {
        "store_call_ms": lambda: store_call(cfg),
        "store_call_no_grid_ms": lambda: store_call(cfg, with_grid=False),
        "store_call_no_filter_ms": lambda: store_call(no_filter),
        "host_cloud_call_ms": host_call,
    }
    wall = {k: [] for k in forms}
    stages = {k: {s: [] for s in STAGES} for k in forms}
    lib.lio_ogm_debug_stage_ms(1, None)
    for fn in forms.values():
        fn()                                                    # warm-up: the pool, the kept workspaces, the code objects
    for _ in range(args.reps):
        for k, fn in forms.items():                             # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[k].append(1e3 * (time.perf_counter() - t0))
            lib.lio_ogm_debug_stage_ms(1, ms)
            for s, v in zip(STAGES, ms):
                stages[k][s].append(float(v))
    lib.lio_ogm_debug_stage_ms(0, None)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    med_stages = {k: {s: float(np.median(v)) for s, v in d.items()} for k, d in stages.items()}
    store_call(cfg)
    stand_in, occ, n_sl, n_inl = host_stand_in(saved, cfg)
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "sensor": args.sensor, "n_keyframes": len(clouds),
        "n_points_summed": int(sum(len(c) for c in clouds)), "map_resolution": args.map_resolution, "n_map": int(n_map),
        "config": {"z_min": cfg.z_min, "z_max": cfg.z_max, "radius": cfg.radius, "min_neighbors": cfg.min_neighbors, "resolution": cfg.resolution},
        "info": {"width": info.width, "height": info.height, "n_slice": info.n_slice, "n_inliers": info.n_inliers, "n_binned": info.n_binned,
                 "n_occupied": info.n_occupied, "grid_bytes": int(cells)},
        "clock": "whole calls: host wall clock around complete calls; stages: HIP events on the chain's stream",
        **med, "stages_ms": med_stages,
        "map_build_inside_the_store_call_ms": med["store_call_ms"] - sum(med_stages["store_call_ms"].values()),
        "host_stand_in_not_pcl": {"what": "numpy slice and raster, scipy.spatial.cKDTree.query_ball_point(return_length) on one thread",
                                  **stand_in, "n_slice": n_sl, "n_inliers": n_inl, "n_occupied": occ},
        "unmeasured": ["k_ogm_search under a profiler (no rocprofv3 pass; the search stage is that kernel alone between two events)",
                       "lanes in cell-sorted order against lanes in input order", "the gain of the form that stops a lane early",
                       "PCL and FLANN themselves"],
    }
    st.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
