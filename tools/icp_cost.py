"""Cost of the loop-closure registration on the device (lio_kf_store_loop_icp) at headline size: one 64x1800 keyframe
(voxel 0.4) against the 51 keyframes around an earlier visit (historyKeyframeSearchNum = 25), submaps at leaf 0.5.

GPU time: HIP events on the null stream around each call (everything of these entry points runs there), medians of --reps
runs, the forms alternating: the whole call; the two submaps alone (lio_assemble_map_resident with the same ids); the ICP
loop + fitness pass alone (lio_icp_align on the submaps, its two uploads and the grid build included).  The fitness pass alone
is one launch of the same search kernel and is reported as unmeasured.  Host stand-in: a scipy cKDTree + numpy ICP loop on the same clouds (tree built
once, the same criteria), wall clock.  It is NOT PCL and is reported, not judged.

    python tools/icp_cost.py [--reps 20] [--out profiles/icp_cost.json]
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
LEAF = 0.5


def host_stand_in(src, tgt, cfg):
    """cKDTree + numpy ICP with the criteria of tests/icp_restate.py (not PCL) -> (iterations, seconds)."""
    from scipy.spatial import cKDTree
    import icp_restate as R
    t0 = time.perf_counter()
    tree = cKDTree(tgt.astype(np.float64))
    cur = src.astype(np.float32).copy()
    crit = R.Criteria(cfg)
    iters = 0
    while True:
        d, j = tree.query(cur.astype(np.float64), distance_upper_bound=cfg["max_corr_dist"])
        keep = np.isfinite(d)
        if keep.sum() < cfg["min_corr"]:
            break
        mse = float((d[keep] ** 2).mean())
        step, _ = R.umeyama_step(cur[keep], tgt[j[keep]])
        cur = R.transform_points(step, cur)
        iters += 1
        if crit.has_converged(iters, step, mse)[0]:
            break
    tree.query(cur.astype(np.float64))                      # getFitnessScore
    return iters, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_cost.json"))
    ap.add_argument("--sensor", default="hdl64")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("icp_cost.py needs a GPU (no CPU fallback)")
    import icp_restate as R
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    n_kf, key_pre, search = 60, 30, 25
    case = synth.make_case(args.sensor, n_keyframes=n_kf, seed=21, device="cuda")
    # the revisit: the place of keyframe key_pre seen again, its pose off by 0.3 m / 1 degree
    boxes = case["boxes"]
    true = np.array(case["kf_poses"][key_pre], np.float64); true[4] += 0.5
    scan, _ = synth.make_query(boxes, true, args.sensor, seed=991, device="cuda")
    wrong = true.copy(); wrong[3] += 0.25; wrong[4] -= 0.15; wrong[5] += 0.05; wrong[2] += np.radians(1.0)
    st = pkg.KeyframeStore()
    z4 = lambda c: np.concatenate([c, np.zeros((len(c), 1), np.float32)], 1)
    for cloud, _ in case["keyframes"]:
        st.add(z4(cloud))
    key_cur = st.add(z4(scan))
    poses = np.array([p for _, p in case["keyframes"]] + [wrong], np.float32)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    cfg = pkg.icp_default_config()
    ids = list(range(key_pre - search, key_pre + search + 1))
    res, rc, (src, tgt, _) = st.loop_icp(key_cur, key_pre, search, LEAF, cfg, want_clouds=True)
    assert rc == 0, rc

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(torch.cuda.default_stream()); fn(); b.record(torch.cuda.default_stream())
        b.synchronize()
        return a.elapsed_time(b)

    forms = {
        "loop_icp_ms": lambda: st.loop_icp(key_cur, key_pre, search, LEAF, cfg),
        "submaps_ms": lambda: (st.assemble([key_cur], poses[[key_cur]], LEAF, want_output=False),
                               st.assemble(ids, poses[ids], LEAF, want_output=False)),
        "icp_align_ms": lambda: pkg.icp_align(src, tgt, cfg),
    }
    samples = {k: [] for k in forms}
    for fn in forms.values():
        fn()                                                # warm-up: pool, pinned words
    for _ in range(args.reps):
        for k, fn in forms.items():                         # alternating
            samples[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in samples.items()}
    it_host, s_host = host_stand_in(src[:, :3], tgt[:, :3], {k: getattr(cfg, k) for k in R.DEFAULTS})
    dt, dr = np.linalg.norm(np.array(res.pose_corrected[3:]) - true[3:]), np.abs(np.array(res.pose_corrected[:3]) - true[:3]).max()
    out = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "sensor": args.sensor, "leaf": LEAF,
        "n_source": res.n_source, "n_target": res.n_target, "target_keyframes": len(ids),
        "iterations": res.iters, "state": pkg.ICP_STATES[res.state], "converged": res.converged, "fitness": res.fitness,
        "accepted": res.accepted, "launches": res.n_launches, "pose_error_m": float(dt), "pose_error_rad": float(dr),
        **med,
        "us_per_iteration_upper_bound": 1000.0 * med["icp_align_ms"] / max(res.iters, 1),
        "fitness_pass_ms": None,
        "host_stand_in_not_pcl": {"what": "scipy cKDTree + numpy, tree built once", "iterations": it_host, "ms": 1000.0 * s_host},
        "unmeasured": ["fitness pass alone (one launch of the search kernel, inside icp_align_ms)",
                       "ICP loop without its two H2D uploads and the grid build (inside icp_align_ms)", "PCL itself"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))
    st.close()


if __name__ == "__main__":
    main()
