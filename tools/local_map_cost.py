"""Cost of the planning local map on the device (lio_kf_store_local_map) at the reference's sizes: the newest 30 and 50
keyframes of 64x1800 sweeps (voxel 0.4), the default crop (70 / 40 / 20 / 40 m), mean_k 10, stddev 1.0.

GPU time: HIP events on the null stream around each call (everything of these entry points runs there), medians of --reps
runs, the forms alternating: the whole call at the default leaf (0.01: the voxel filter passes through, as in PCL) and at
leaf 0.4; the sum alone (lio_assemble_map_resident with a leaf that passes through); sum + crop; sum + crop + filter; the
filter alone on the cropped cloud (lio_sor_filter, its upload, download and grid build included).  Host stand-in: a scipy
cKDTree + numpy filter on the same cropped cloud, wall clock.  It is NOT PCL and is reported, not judged.

    python tools/local_map_cost.py [--reps 20] [--out profiles/local_map_cost.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_stand_in(cloud, mean_k, mul):
    """cKDTree k-NN + numpy threshold (not PCL) -> (inliers, seconds)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = cloud[:, :3].astype(np.float64)
    d, _ = cKDTree(p).query(p, k=mean_k + 1)
    dist = d[:, 1:].sum(1) / mean_k
    keep = dist <= dist.mean() + mul * dist.std(ddof=1)
    return int(keep.sum()), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_cost.json"))
    ap.add_argument("--sensor", default="hdl64")
    ap.add_argument("--keyframes", type=int, nargs="+", default=[30, 50])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("local_map_cost.py needs a GPU (no CPU fallback)")
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
        ids = list(range(n_kf - k, n_kf))
        cfg = lambda **kw: pkg.local_map_default_config(n_keyframes=k, **kw)
        cropped, info_c, _ = st.local_map(pose, cfg(remove_outliers=0, downsample=0))
        _, info, _ = st.local_map(pose, cfg())
        _, info4, _ = st.local_map(pose, cfg(leaf=0.4))
        forms = {
            "local_map_ms": lambda: st.local_map(pose, cfg(), want_output=False),
            "local_map_leaf04_ms": lambda: st.local_map(pose, cfg(leaf=0.4), want_output=False),
            "sum_ms": lambda: st.assemble(ids, poses[ids], 1e-3, want_output=False),
            "sum_crop_ms": lambda: st.local_map(pose, cfg(remove_outliers=0, downsample=0), want_output=False),
            "sum_crop_filter_ms": lambda: st.local_map(pose, cfg(downsample=0), want_output=False),
            "sor_filter_host_cloud_ms": lambda: pkg.sor_filter(cropped, 10, 1.0),
        }
        samples = {name: [] for name in forms}
        for fn in forms.values():
            fn()                                            # warm-up: the pool
        for _ in range(args.reps):
            for name, fn in forms.items():                  # alternating
                samples[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in samples.items()}
        n_host, s_host = host_stand_in(cropped, 10, 1.0)
        rows[str(k)] = {
            "n_summed": info.n_summed, "n_cropped": info.n_cropped, "n_inliers": info.n_inliers, "n_out": info.n_out,
            "voxel_passthrough": info.voxel_passthrough, "n_out_leaf04": info4.n_out,
            "sor": [info.sor_mean, info.sor_stddev, info.sor_threshold], **med,
            "filter_by_difference_ms": med["sum_crop_filter_ms"] - med["sum_crop_ms"],
            "crop_by_difference_ms": med["sum_crop_ms"] - med["sum_ms"],
            "host_stand_in_not_pcl": {"what": "scipy cKDTree + numpy on the cropped cloud", "inliers": n_host, "ms": 1000.0 * s_host},
        }
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sensor": args.sensor, "mean_k": 10, "stddev_mul": 1.0,
           "crop": [70.0, 40.0, 20.0, 40.0], "keyframes": rows,
           "unmeasured": ["the search kernel alone (inside filter_by_difference_ms, with the grid build and the compaction)",
                          "the tail of a wave behind an isolated point (the crop bounds the grid: no far point in these clouds)",
                          "PCL itself"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
