"""Cost of selecting the surrounding keyframes on the device (lio_assemble_map_nearby) against the resident assembly given ids
selected on the host (lio_assemble_map_resident), at N_kf = 200, 1 000, 10 000 and 50 000 key poses.

Every selected keyframe carries a cloud of headline size (6 600 points: the 200-keyframe headline map holds 1.32 M); the others
carry 4 points, so that the store stays small at 50 000 keyframes.  Layouts: a straight drive at 1 m (the selection is the last
~50 m plus the 10 s window) and, up to 1 000 keyframes, the lawn-mower path of configs[3] (every keyframe within the radius).

GPU time: HIP events on the null stream around each call, generic path (s2m = None: everything runs on the null stream, so the
events bracket all of it), the two forms alternating.  Host time: wall clock of the node path (a handle), which returns with the
grid build still in flight.  The host selection is timed with scipy's cKDTree as a STAND-IN for PCL's kd-tree (no PCL here):
it is not a measurement of PCL.

    python tools/nearby_cost.py [--reps 20] [--out profiles/nearby_cost.json] [--sizes 200,1000,10000,50000]
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
HEADLINE_PTS = 6600
LEAF = 0.5


def host_selection(P, t, time_cur, R=50.0, density=1.0, window=10.0):
    """extractNearby MO:1519-1551 + MO:1562 on the host with cKDTree (stand-in for PCL's kd-tree) and a numpy VoxelGrid."""
    from scipy.spatial import cKDTree
    tree = cKDTree(P)                                                   # MO:1527: rebuilt every callback
    hit = np.asarray(tree.query_ball_point(P[-1], R), np.int64)         # MO:1528
    q = P[hit]
    inv = np.float32(1.0) / np.float32(density)
    ijk = np.floor(q * inv).astype(np.int64)
    ijk -= ijk.min(0)
    dims = ijk.max(0) + 1
    key = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]
    uk, inv_idx = np.unique(key, return_inverse=True)
    cent = np.zeros((len(uk), 3)); np.add.at(cent, inv_idx, q); cent /= np.bincount(inv_idx)[:, None]
    _, ids = tree.query(cent, k=1)                                      # MO:1537-1541
    ids = list(ids)
    coords = list(cent)
    for i in range(len(P) - 1, -1, -1):                                 # MO:1544-1551
        if not (time_cur - t[i] < window):
            break
        ids.append(i); coords.append(P[i])
    keep = np.linalg.norm(np.asarray(coords) - P[-1], axis=1) <= R      # MO:1562
    return np.asarray(ids, np.int32)[keep]


def layout(kind, n):
    synth = importlib.import_module("lio-slam_amd.synth")
    if kind == "lawnmower":
        poses = synth.keyframe_poses(n, seed=77, lawnmower=True).astype(np.float32)
    else:
        poses = synth.keyframe_poses(n, spacing=1.0, seed=77).astype(np.float32)
    times = 100.0 + 1.0 * np.arange(n)
    return poses, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="200,1000,10000,50000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearby_cost.json"))
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("lio-slam_amd")
    rng = np.random.default_rng(0)
    big = rng.uniform(-1, 1, (HEADLINE_PTS, 3)) * np.array([50.0, 50.0, 5.0])
    big = np.concatenate([big, rng.uniform(0, 255, (HEADLINE_PTS, 1))], 1).astype(np.float32)
    tiny = big[:4].copy()
    rows = []
    for kind in ("straight", "lawnmower"):
        for n in [int(v) for v in args.sizes.split(",")]:
            if kind == "lawnmower" and n > 1000:
                continue
            poses, times = layout(kind, n)
            time_cur = float(times[-1]) + 0.1
            P = poses[:, 3:6].astype(np.float64)
            near = np.linalg.norm(P - P[-1], axis=1) < 51.0
            st = pkg.KeyframeStore()
            for i in range(n):
                st.add(big if near[i] else tiny)
            st.set_poses(0, poses, times)
            _, n_map, ids, _ = st.assemble_nearby(time_cur, LEAF, want_output=False)
            ids_host = host_selection(P, times, time_cur)
            kp = poses[ids]
            # host stand-in
            th = []
            for _ in range(args.reps):
                t0 = time.perf_counter(); host_selection(P, times, time_cur); th.append(time.perf_counter() - t0)
            # GPU time, alternating, generic path on the null stream
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            g_near, g_res = [], []
            for r in range(args.reps + 2):
                ev[0].record(); st.assemble_nearby(time_cur, LEAF, want_ids=False, want_output=False); ev[1].record()
                ev[2].record(); st.assemble(ids, kp, LEAF, want_output=False); ev[3].record()
                torch.cuda.synchronize()
                if r >= 2:
                    g_near.append(ev[0].elapsed_time(ev[1])); g_res.append(ev[2].elapsed_time(ev[3]))
            # host wall time of the node path (the call returns with the grid build in flight)
            s2m = pkg.ScanToMap()
            w_near, w_res = [], []
            for r in range(args.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); st.assemble_nearby(time_cur, LEAF, s2m=s2m, want_ids=False, want_output=False)
                t1 = time.perf_counter(); torch.cuda.synchronize()
                t2 = time.perf_counter(); st.assemble(ids, kp, LEAF, s2m=s2m, want_output=False); t3 = time.perf_counter()
                torch.cuda.synchronize()
                if r >= 2:
                    w_near.append(t1 - t0); w_res.append(t3 - t2)
            s2m.close(); st.close()
            row = {"layout": kind, "n_kf": n, "n_ids": int(len(ids)), "n_unique": int(len(set(ids.tolist()))),
                   "points": int(sum(HEADLINE_PTS if near[i] else 4 for i in ids)), "n_map": int(n_map),
                   "gpu_ms_nearby_median": float(np.median(g_near)), "gpu_ms_resident_median": float(np.median(g_res)),
                   "host_ms_node_nearby_median": 1e3 * float(np.median(w_near)), "host_ms_node_resident_median": 1e3 * float(np.median(w_res)),
                   "host_selection_ckdtree_ms_median_STAND_IN_NOT_PCL": 1e3 * float(np.median(th)),
                   "host_ckdtree_ids_equal_device_ids": bool(np.array_equal(np.sort(ids_host), np.sort(ids)))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "leaf": LEAF, "headline_pts": HEADLINE_PTS,
                   "note": "cKDTree timings are a stand-in for PCL's kd-tree, not a measurement of it", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
