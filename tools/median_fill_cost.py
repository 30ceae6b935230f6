"""Cost of the median fill on the device (lio_median_fill) on the terrain profile's 550 x 400 grid at 0.2 m -- a tilted plane
with noise, boxes and 8 % holes (tools/terrain_cost.py's scene) plus one 4 x 5 hole -- and of the one-chain call
lio_kf_store_planning_map beside the pair of calls it replaces.

GPU time: HIP events on the null stream around each call (everything of these entry points runs there), medians of --reps
runs, the forms alternating.  The whole call (grid up, two kernels, filled grid down) at radii of 5 and 32 cells with
filter_existing_values off and on; the kernels by difference between forms that make one of them trivial (a radius of 0
cells: k_mf_fill reads one cell 33 times; a mask handed in: k_mf_mask does not run, one more copy to the device, which is
timed beside the calls as a stand-in).  The chain: the local map of tools/sdf_cost.py (the newest 30 keyframes of 64 x 1800
sweeps, the default crop); lio_kf_store_terrain_map followed by lio_kf_store_sdf on the height map with fill_holes = 1 and
nan_policy = 1 -- the pair a node calls today -- against one lio_kf_store_planning_map with fill_holes = 0 and the median fill,
and against the same call without the fill.  --parent-package DIR: the pair is called from the package in DIR (a built
lio-slam_amd directory of the commit before, loaded beside this one with its own library and its own store of the same
keyframes), alternating with the new call in the same process; without it the pair is called from this library, whose entry
points and kernels for it are the ones that commit has.

    python tools/median_fill_cost.py [--reps 20] [--parent-package DIR] [--out profiles/median_fill_cost.json]
"""
import argparse
import ctypes as C
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS, COLS, RES = 550, 400, 0.2
BAND = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--keyframes", type=int, default=30)
    ap.add_argument("--parent-package", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_fill_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("median_fill_cost.py needs a GPU (no CPU fallback)")
    import terrain_cost
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    lib = pkg.load_library()
    grid = terrain_cost.scene()
    grid[100:104, 200:205] = np.nan
    n_cells = ROWS * COLS
    filled = np.zeros(n_cells, np.float32)
    zeros = np.zeros(n_cells, np.float32)
    info = pkg.MedianFillInfo()
    infos = {}

    def call(name, cells, filter_existing=0, mask_in=None, n=4):
        cfg = pkg.median_fill_default_config(fill_hole_radius=(cells + 0.5) * RES, existing_value_radius=(cells + 0.5) * RES,
                                             filter_existing_values=filter_existing, num_erode_dilation_iterations=n)
        rc = lib.lio_median_fill(0, grid.ctypes.data, ROWS, COLS, RES, C.byref(cfg), None if mask_in is None else mask_in.ctypes.data,
                                 filled.ctypes.data, None, None, C.byref(info))
        assert rc == 0, rc
        infos[name] = {k: getattr(info, k) for k, _ in pkg.MedianFillInfo._fields_ if k != "pad"}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(torch.cuda.default_stream()); fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        return a.elapsed_time(b)

    d_buf = torch.zeros(n_cells, dtype=torch.float32, device="cuda")
    h_grid = torch.from_numpy(np.ascontiguousarray(grid.ravel(order="F")))
    forms = {
        "median_fill_r5_ms": lambda: call("r5", 5),
        "median_fill_r32_ms": lambda: call("r32", 32),
        "median_fill_r5_filter_existing_ms": lambda: call("r5_filter", 5, 1),
        "median_fill_r32_filter_existing_ms": lambda: call("r32_filter", 32, 1),
        "median_fill_r0_ms": lambda: call("r0", 0),
        "median_fill_r0_mask_in_zeros_ms": lambda: call("r0_mask_in", 0, 0, zeros),
        "median_fill_r5_n15_ms": lambda: call("r5_n15", 5, 0, None, 15),
        "h2d_copy_of_grid_bytes_ms": lambda: d_buf.copy_(h_grid),
    }
    # the chain
    case = synth.make_case("hdl64", n_keyframes=args.keyframes, seed=21, device="cuda")
    st = pkg.KeyframeStore()
    for cloud, _ in case["keyframes"]:
        st.add(np.concatenate([cloud, np.zeros((len(cloud), 1), np.float32)], 1))
    poses = np.array([p for _, p in case["keyframes"]], np.float32)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    pose = poses[-1]
    lm = pkg.local_map_default_config(n_keyframes=args.keyframes)
    hm_raw = pkg.height_map_default_config(roll=float(pose[0]), pitch=float(pose[1]), fill_holes=0)
    sdf = pkg.Sdf()
    grid_c, hm_info, _ = st.height_map(pose, lm, hm_raw)
    lo_c = float(np.nanmin(grid_c))
    scfg = pkg.sdf_default_config(min_height=lo_c, max_height=lo_c + BAND, nan_policy=1)
    tcfg = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)
    fcfg = pkg.median_fill_default_config(fill_hole_radius=1.0, num_erode_dilation_iterations=4)
    chain_info = {}
    # the pair: from the package of the commit before when one is given, with its own store, object and configurations
    old = pkg
    if args.parent_package:
        d = os.path.abspath(args.parent_package)
        spec = importlib.util.spec_from_file_location("lio_slam_amd_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
        old = importlib.util.module_from_spec(spec)
        sys.modules["lio_slam_amd_parent"] = old
        spec.loader.exec_module(old)
        assert not hasattr(old.load_library(), "lio_median_fill"), "--parent-package holds this commit's library"
    st_old, sdf_old = old.KeyframeStore(), old.Sdf()
    for cloud, _ in case["keyframes"]:
        st_old.add(np.concatenate([cloud, np.zeros((len(cloud), 1), np.float32)], 1))
    st_old.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    lm_old = old.local_map_default_config(n_keyframes=args.keyframes)
    hm_old = old.height_map_default_config(roll=float(pose[0]), pitch=float(pose[1]), fill_holes=1)
    scfg_old = old.sdf_default_config(min_height=lo_c, max_height=lo_c + BAND, nan_policy=1)
    tcfg_old = old.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)

    def pair():
        st_old.terrain_map(pose, lm_old, hm_old, tcfg_old)
        st_old.sdf_map(sdf_old, pose, lm_old, hm_old, scfg_old)

    def one_call(fill):
        out = st.planning_map(pose, lm, hm_raw, fill, tcfg, sdf, scfg)
        if fill is not None:
            chain_info.update({k: getattr(out["fill_info"], k) for k, _ in pkg.MedianFillInfo._fields_ if k != "pad"})

    forms["pair_terrain_map_then_sdf_ms"] = pair
    forms["planning_map_with_fill_ms"] = lambda: one_call(fcfg)
    forms["planning_map_without_fill_ms"] = lambda: one_call(None)
    forms["kf_store_height_map_ms"] = lambda: st.height_map(pose, lm, hm_raw)
    samples = {name: [] for name in forms}
    for fn in forms.values():
        fn()                                                    # warm-up: the pool, the code objects, the buffers
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            samples[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in samples.items()}
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": ROWS, "cols": COLS, "resolution": RES,
        "clock": "HIP events on the null stream around calls that end complete", **med,
        "kernels_by_difference_ms": {
            "k_mf_fill_r5_against_r0": med["median_fill_r5_ms"] - med["median_fill_r0_ms"],
            "k_mf_fill_r32_against_r0": med["median_fill_r32_ms"] - med["median_fill_r0_ms"],
            "k_mf_mask_n4_against_a_mask_handed_in": med["median_fill_r0_ms"] - med["median_fill_r0_mask_in_zeros_ms"] + med["h2d_copy_of_grid_bytes_ms"],
            "k_mf_mask_n15_against_n4": med["median_fill_r5_n15_ms"] - med["median_fill_r5_ms"],
        },
        "counts": infos,
        "chain": {"pair_called_from": "the package of the commit before" if args.parent_package else "this library", "keyframes": args.keyframes, "rows": hm_info.rows, "cols": hm_info.cols, "height_map_points": hm_info.n_in, "fill": chain_info,
                  "saving_with_fill_ms": med["pair_terrain_map_then_sdf_ms"] - med["planning_map_with_fill_ms"],
                  "saving_without_fill_ms": med["pair_terrain_map_then_sdf_ms"] - med["planning_map_without_fill_ms"]},
        "unmeasured": ["the kernels one by one under a profiler (differences of whole calls; no rocprofv3 pass)",
                       *([] if args.parent_package else ["the pair from a build of the commit before (the same entry points of this library stand in for it)"]),
                       "grid_map and OpenCV themselves"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    sdf.close(); st.close(); sdf_old.close(); st_old.close()


if __name__ == "__main__":
    main()
