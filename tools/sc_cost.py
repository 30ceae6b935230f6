"""Cost of Scan Context on the device (lio_sc.hip) at headline size: the descriptor of one 64x1800 sweep (115 200 rays) from
the blob lio_s2m_register_raw has just staged and from a host cloud, and lio_kf_store_sc_detect over 100 / 1000 / 5000
stored descriptors (default constants: 3 candidates, 7 shifts each).

Times are wall clock around the synchronous calls (each ends with its own stream wait), medians of --reps runs, the forms
alternating; Python ctypes caller.  They are absolute figures, recorded and not judged: nothing was measured before.
--ab DIR adds `single_scan_node_path_ms.total_resident_keyframes` of `python bench.py --full [--no-cpu]` runs found there as
bench_parent_<n>.json / bench_change_<n>.json (the parent commit and this tree, alternating).

    python tools/sc_cost.py [--reps 30] [--ab DIR] [--out profiles/sc_cost.json]
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


def node_path(ab_dir):
    out = {}
    for label in ("parent", "change"):
        vals = []
        for p in sorted(glob.glob(os.path.join(ab_dir, f"bench_{label}_*.json"))):
            d = json.loads(open(p).read().strip().splitlines()[-1])
            vals.append({"total_resident_keyframes": d["single_scan_node_path_ms"]["total_resident_keyframes"],
                         "downsample_and_register_from_raw_cloud": d["single_scan_node_path_ms"]["downsample_and_register_from_raw_cloud"],
                         "value_reg_per_s": d["value"]})
        out[label] = vals
    for key in ("total_resident_keyframes", "downsample_and_register_from_raw_cloud"):      # the spread of each side's own runs
        out[key + "_min_max"] = {label: [min(v[key] for v in out[label]), max(v[key] for v in out[label])]
                                 for label in ("parent", "change") if out[label]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ab", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sc_cost.json"))
    ap.add_argument("--sensor", default="hdl64")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sc_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    case = synth.make_case("vlp16", n_keyframes=6, seed=21, device="cuda")
    boxes = synth.make_scene(21, length=120.0)
    pose = synth.keyframe_poses(8, spacing=2.0, seed=21)[3]
    sc = synth.cast_scan(boxes, pose, args.sensor, seed=5, max_range=1e9, device="cuda")      # every ray that hits: the full sweep
    xyz = sc["xyz"]
    rec = np.zeros((len(xyz), 8), np.float32)
    rec[:, :3], rec[:, 3] = xyz, 1.0
    h = pkg.ScanToMap()
    h.set_map(case["map"])
    lay = pkg.PC2Layout(point_step=32, off_x=0, off_intensity=16, off_ring=-1, off_time=-1)
    h.downsampleAndScan2MapOptimization(rec, len(rec), lay, 0.4, pose.astype(np.float32))
    st = pkg.KeyframeStore()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    build = {"build_from_resident_blob_ms": lambda: st.sc_add_from_handle(h), "build_from_host_cloud_ms": lambda: st.sc_add(rec),
             "make_standalone_host_cloud_ms": lambda: pkg.sc_make(rec)}
    samples = {k: [] for k in build}
    for fn in build.values():
        fn()
    for _ in range(args.reps):
        for k, fn in build.items():
            samples[k].append(timed(fn))
    st.close()
    # detection: stores of random descriptors' worth of small clouds (the cost does not depend on what they hold)
    rng = np.random.default_rng(3)
    clouds = []
    for _ in range(64):
        r, a = rng.uniform(1, 75, 2000), rng.uniform(0, 2 * np.pi, 2000)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.5, 8, 2000)], 1).astype(np.float32))
    cfg = pkg.sc_default_config(tree_period=1)                 # every call searches the whole current prefix
    st = pkg.KeyframeStore()
    detect = {}
    for n in (100, 1000, 5000):
        while st.sc_count() < n:
            st.sc_add(clouds[int(rng.integers(0, 64))][int(rng.integers(0, 4))::4])
        st.sc_detect(cfg)
        ts = [timed(lambda: st.sc_detect(cfg)) for _ in range(args.reps)]
        res = st.sc_detect(cfg)
        detect[str(n)] = {"detect_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "n_searched": res.n_searched,
                          "n_candidates": res.n_candidates}
    st.close(); h.close()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sensor": args.sensor, "points": int(len(xyz)),
           **{k: float(np.median(v)) for k, v in samples.items()}, **{k.replace("_ms", "_min_ms"): float(np.min(v)) for k, v in samples.items()},
           "detect": detect, "clock": "wall clock around the synchronous call, Python ctypes caller",
           "node_path_ab": node_path(args.ab) if args.ab else None,
           "unmeasured": ["kernel times alone (no profiler run)", "the reference's serial makeScancontext and nanoflann search (not buildable here)"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
