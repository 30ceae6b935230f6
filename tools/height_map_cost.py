"""Cost of the planning height map on the device (lio_kf_store_height_map) at the reference's sizes: the newest 30 and 50
keyframes of 64x1800 sweeps, the default crop and filters of the local map, the defaults of grid_map_pcl's parameters.yaml
(resolution 0.2, second outlier filter on, no clustering).

GPU time: HIP events on the null stream around each call (everything of these entry points runs there), medians of --reps
runs, the forms alternating.  The whole call; the same with use_cluster = 1; the stages by difference between forms that
switch one stage off or make it trivial: the second outlier filter (remove_outliers 0); level and ego filter
(level_and_ego_filter 0, which leaves the compaction of the finite points); the box pass and that compaction (grid == NULL
with both off, against the local map alone); elevation (min_points_per_cell above every cell's count: the kernel runs and
writes NaN without reading a point), for the mean and for the cluster kernel; binning, the NaN layer and the grid copy (that
form against grid == NULL); fill (fill_holes 1 against 0).  The grid copy has no form of its own: a device-to-host copy of
the same bytes into the same kind of host array is timed beside the calls as a stand-in.  For comparison
lio_kf_store_local_map with its output copied to the host followed by lio_height_map from the host, which is what a node
must do today with any consumer of the cloud.  Host stand-in: numpy / scipy binning and per-cell means on the same local map,
wall clock.  It is NOT the reference (no PCL, no grid_map) and is reported, not judged.
--ab DIR adds `value` and `single_scan_node_path_ms` of `python bench.py --full --no-cpu` runs found there as
bench_parent_<n>.json / bench_change_<n>.json (a tree of the parent commit and this one, alternating).

    python tools/height_map_cost.py [--reps 20] [--ab DIR] [--out profiles/height_map_cost.json]
"""
import argparse
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_stand_in(cloud, resolution):
    """cKDTree outlier filter + numpy binning + bincount means (not the reference) -> (valid cells, seconds)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = cloud[:, :3].astype(np.float64)
    d, _ = cKDTree(p).query(p, k=11)
    dist = d[:, 1:].sum(1) / 10
    p = p[dist <= dist.mean() + dist.std(ddof=1)]
    mn, mx = p[:, :2].min(0), p[:, :2].max(0)
    size = np.round((mx - mn) / resolution).astype(int)
    idx = np.trunc((0.5 * size * resolution + 0.5 * (mx + mn) - p[:, :2]) / resolution).astype(int)
    ok = (idx < size).all(1)
    key = idx[ok, 0] + idx[ok, 1] * size[0]
    s = np.bincount(key, p[ok, 2], size.prod())
    c = np.bincount(key, minlength=size.prod())
    return int((c > 0).sum()), time.perf_counter() - t0, (s / np.maximum(c, 1)).sum()


def node_path(ab_dir):
    out = {}
    for label in ("parent", "change"):
        vals = []
        for p in sorted(glob.glob(os.path.join(ab_dir, f"bench_{label}_*.json"))):
            d = json.loads(open(p).read().strip().splitlines()[-1])
            vals.append({"value_reg_per_s": d["value"], "single_scan_node_path_ms": d["single_scan_node_path_ms"]})
        out[label] = vals
    for key in ("total_resident_keyframes", "downsample_and_register_from_raw_cloud"):      # the spread of each side's own runs
        out[key + "_min_max"] = {label: [min(v["single_scan_node_path_ms"][key] for v in out[label]),
                                         max(v["single_scan_node_path_ms"][key] for v in out[label])]
                                 for label in ("parent", "change") if out[label]}
    out["value_min_max"] = {label: [min(v["value_reg_per_s"] for v in out[label]), max(v["value_reg_per_s"] for v in out[label])]
                            for label in ("parent", "change") if out[label]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "height_map_cost.json"))
    ap.add_argument("--sensor", default="hdl64")
    ap.add_argument("--keyframes", type=int, nargs="+", default=[30, 50])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("height_map_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    n_kf = max(args.keyframes)
    case = synth.make_case(args.sensor, n_keyframes=n_kf, seed=21, device="cuda")
    st = pkg.KeyframeStore()
    for cloud, _ in case["keyframes"]:
        st.add(np.concatenate([cloud, np.zeros((len(cloud), 1), np.float32)], 1))
    poses = np.array([p for _, p in case["keyframes"]], np.float32)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    pose = poses[-1]                                        # transformTobeMapped at the newest keyframe

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(torch.cuda.default_stream()); fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        return a.elapsed_time(b)

    rows = {}
    for k in args.keyframes:
        lm = pkg.local_map_default_config(n_keyframes=k)
        hm = lambda **kw: pkg.height_map_default_config(roll=float(pose[0]), pitch=float(pose[1]), **kw)
        cloud, lm_info, _ = st.local_map(pose, lm)
        grid, info, _ = st.height_map(pose, lm, hm())
        _, info_c, _ = st.height_map(pose, lm, hm(use_cluster=1))
        _, info_f, _ = st.height_map(pose, lm, hm(fill_holes=1))
        n_cells = info.rows * info.cols
        buf = np.zeros(max(n_cells, 1), np.float32)
        import ctypes as C
        lib, hi, li = pkg.load_library(), pkg.HeightMapInfo(), pkg.LocalMapInfo()
        pose_p = pose.ctypes.data_as(C.POINTER(C.c_float))

        def store_call(cfg, with_grid=True):
            rc = lib.lio_kf_store_height_map(st.h, C.byref(lm), pose_p, C.byref(cfg), buf.ctypes.data if with_grid else None, buf.size,
                                             C.byref(li), C.byref(hi))
            assert rc == 0, rc

        def through_the_host():
            c, _, _ = st.local_map(pose, lm)
            xyz = np.ascontiguousarray(c[:, :3])
            assert lib.lio_height_map(0, xyz.ctypes.data, len(xyz), 12, C.byref(hm()), buf.ctypes.data, buf.size, C.byref(hi)) == 0

        never = 2000000000                                  # min_points_per_cell no cell reaches: elevation writes NaN, reads no point
        d_grid = torch.zeros(max(n_cells, 1), dtype=torch.float32, device="cuda")
        h_grid = torch.from_numpy(buf)

        forms = {
            "height_map_ms": lambda: store_call(hm()),
            "height_map_cluster_ms": lambda: store_call(hm(use_cluster=1)),
            "height_map_fill_ms": lambda: store_call(hm(fill_holes=1)),
            "no_second_sor_ms": lambda: store_call(hm(remove_outliers=0)),
            "no_level_ego_ms": lambda: store_call(hm(level_and_ego_filter=0)),
            "no_elevation_ms": lambda: store_call(hm(min_points_per_cell=never)),
            "no_elevation_cluster_ms": lambda: store_call(hm(use_cluster=1, min_points_per_cell=never)),
            "geometry_only_ms": lambda: store_call(hm(), with_grid=False),
            "geometry_only_no_sor_no_level_ms": lambda: store_call(hm(remove_outliers=0, level_and_ego_filter=0), with_grid=False),
            "local_map_alone_ms": lambda: st.local_map(pose, lm, want_output=False),
            "local_map_to_host_then_height_map_ms": through_the_host,
            "d2h_copy_of_grid_bytes_ms": lambda: h_grid.copy_(d_grid),
        }
        samples = {name: [] for name in forms}
        for fn in forms.values():
            fn()                                            # warm-up: the pool
        for _ in range(args.reps):
            for name, fn in forms.items():                  # alternating
                samples[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in samples.items()}
        n_host, s_host, _ = host_stand_in(cloud, 0.2)
        rows[str(k)] = {
            "n_local_map": lm_info.n_out, "rows": info.rows, "cols": info.cols, "grid_bytes": 4 * n_cells,
            "n_inliers": info.n_inliers, "n_filtered": info.n_filtered, "n_binned": info.n_binned, "n_valid_cells": info.n_valid_cells,
            "n_valid_cells_cluster": info_c.n_valid_cells, "n_filled_cells_with_fill": info_f.n_filled_cells, **med,
            "stages_by_difference_ms": {
                "second_sor": med["height_map_ms"] - med["no_second_sor_ms"],
                "level_and_ego_filter_against_finite_only": med["height_map_ms"] - med["no_level_ego_ms"],
                "box_and_finite_compaction": med["geometry_only_no_sor_no_level_ms"] - med["local_map_alone_ms"],
                "sor_level_box_together": med["geometry_only_ms"] - med["local_map_alone_ms"],
                "binning_nan_layer_grid_copy": med["no_elevation_ms"] - med["geometry_only_ms"],
                "elevation_mean": med["height_map_ms"] - med["no_elevation_ms"],
                "elevation_cluster": med["height_map_cluster_ms"] - med["no_elevation_cluster_ms"],
                "fill": med["height_map_fill_ms"] - med["height_map_ms"],
                "grid_copy_stand_in": med["d2h_copy_of_grid_bytes_ms"],
            },
            "host_stand_in_not_the_reference": {"what": "scipy cKDTree filter + numpy binning and bincount means on the local map",
                                                "valid_cells": n_host, "ms": 1000.0 * s_host},
        }
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sensor": args.sensor, "resolution": 0.2, "keyframes": rows,
           "node_path_ab": node_path(args.ab) if args.ab else None,
           "unmeasured": ["the kernels one by one (the stages are differences of whole calls; no rocprofv3 pass)",
                          "binning (keys, sort, ranges) apart from the grid copy: one difference holds both",
                          "the grid copy inside the call (grid_copy_stand_in is a separate copy of the same bytes)",
                          "the cluster kernel's workgroup-per-cell cost per cell, and cells past its LDS tile at these sizes",
                          "PCL / grid_map themselves"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
