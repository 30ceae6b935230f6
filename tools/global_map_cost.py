"""Cost of the global map (lio_kf_store_global_map) and of the map export (lio_kf_store_export_map) on the device, on the
bench's 200-keyframe synthetic map (64x1800 sweeps, voxel 0.4) and on a longer trajectory: --long keyframes on a lawn-mower
path that reuse the 200 clouds in turn (no further ray casting; the poses, and so the world-frame clouds, all differ).

Wall clock around each call (they end complete: every one waits for its own streams), medians of --reps runs, the forms
alternating: the global map at the yaml defaults (1000 m, 10 m, 1 m), counts only and with the cloud; the export at
resolution 0 (the chunked path alone: its bytes over its time is the achieved device-to-host rate) and at 0.2.  Device
memory: hipMemGetInfo before and after the first resolution-0 export of a fresh store -- what the path allocates -- at both
store sizes.  Host baseline: the restatement of tests/globalmap_restate.py (numpy + the project's C oracle, one thread), run
once in the same process.  It is NOT PCL and is reported, not judged.

    python tools/global_map_cost.py [--reps 5] [--long 2000] [--out profiles/global_map_cost.json]
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


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1000.0 * (time.perf_counter() - t0)


def measure(pkg, torch, oracle, G, name, clouds, poses, reps, restate):
    st = pkg.KeyframeStore()
    for c in clouds:
        st.add(c)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    total = sum(len(c) for c in clouds)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    st.export_map(0.0, want_full=False)                     # count only: allocates the per-keyframe table
    free1 = torch.cuda.mem_get_info()[0]
    L, C = st.lib, __import__("ctypes")
    full = np.zeros((max(total, 1), 8), np.float32)
    ds = np.zeros((max(total, 1), 8), np.float32)
    n_full, n_ds, vpt = C.c_size_t(), C.c_size_t(), C.c_int32()

    def export(res, want_ds=True):
        cfg = pkg.ExportConfig(res, 0)
        rc = L.lio_kf_store_export_map(st.h, C.byref(cfg), full.ctypes.data, 32, len(full), C.byref(n_full),
                                       ds.ctypes.data if want_ds else None, 32, len(ds), C.byref(n_ds), C.byref(vpt))
        assert rc == 0, rc
        return n_full.value, n_ds.value

    export(0.0)
    free2 = torch.cuda.mem_get_info()[0]
    cfg = pkg.global_map_default_config()
    forms = {
        "global_map_counts_ms": lambda: st.global_map(cfg, want_ids=False, want_output=False),
        "global_map_ms": lambda: st.global_map(cfg),
        "export_res0_ms": lambda: export(0.0),
        "export_res02_ms": lambda: export(0.2),
    }
    samples = {k: [] for k in forms}
    for fn in forms.values():
        fn()                                                # warm-up: the kept workspaces
    for _ in range(reps):
        for k, fn in forms.items():                         # alternating
            samples[k].append(wall(fn)[1])
    med = {k: float(np.median(v)) for k, v in samples.items()}
    spread = {k.replace("_ms", "_min_max_ms"): [float(min(v)), float(max(v))] for k, v in samples.items()}
    gm, ids, info = st.global_map(cfg)
    n_f, n_d = export(0.2)
    row = {"n_keyframes": len(clouds), "n_points": total, "bytes_out_res0": total * 32, **med, **spread,
           "export_d2h_GBps": total * 32 / (med["export_res0_ms"] * 1e-3) / 1e9,
           "global_map": {"n_selected": int(info.n_keyframes), "n_summed": int(info.n_summed), "n_out": int(info.n_out)},
           "export_res02_n_ds": int(n_d),
           "device_bytes_allocated_by_export_res0": {"count_only_call": int(free0 - free1), "first_full_call": int(free0 - free2),
                                                     "per_keyframe_bytes_expected": 92},
           "pinned_host_bytes_export_res0": int(2 * min(total, 1 << 22) * 32)}
    if restate:
        (_, r_ids, _), t_gm = wall(lambda: G.global_map(oracle, clouds, poses, 1000.0, 10.0, 1.0))
        (r_full, _, _), t_e0 = wall(lambda: G.export_map(oracle, clouds, poses, 0.0))
        (_, r_ds, _), t_e2 = wall(lambda: G.export_map(oracle, clouds, poses, 0.2))
        got = np.concatenate([full[:n_f, :3], full[:n_f, 4:5]], 1)
        row["restatement_not_pcl"] = {"what": "tests/globalmap_restate.py: numpy + the C oracle, one thread, one run",
                                      "global_map_ms": t_gm, "export_res0_ms": t_e0, "export_res02_ms": t_e2,
                                      "ids_equal": bool(r_ids.tolist() == ids.tolist()),
                                      "full_bit_equal": bool(np.array_equal(got.view(np.uint32), r_full.view(np.uint32))),
                                      "n_ds_equal": bool(len(r_ds) == n_d)}
    st.close()
    print(name, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--sensor", default="hdl64")
    ap.add_argument("--no-restate-long", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_map_cost.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("global_map_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    import globalmap_restate as G
    from oracle.oracle import Oracle
    oracle = Oracle()
    case = synth.make_case(args.sensor, n_keyframes=args.keyframes, seed=synth.BASE_SEED, device="cuda", with_map=True)
    clouds = [np.concatenate([c, np.full((len(c), 1), float(k % 255), np.float32)], 1).astype(np.float32)
              for k, (c, _) in enumerate(case["keyframes"])]
    poses = np.array([p for _, p in case["keyframes"]], np.float32)
    rows = {"bench_map": measure(pkg, torch, oracle, G, "bench_map", clouds, poses, args.reps, True)}
    long_poses = synth.keyframe_poses(args.long, seed=synth.BASE_SEED, lawnmower=True).astype(np.float32)
    long_poses[:, 3] *= 10.0; long_poses[:, 4] *= 10.0      # 700 m rows 2.8 m apart: most of it inside the 1000 m radius
    long_clouds = [clouds[k % len(clouds)] for k in range(args.long)]
    rows["long"] = measure(pkg, torch, oracle, G, "long", long_clouds, long_poses, args.reps, not args.no_restate_long)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sensor": args.sensor, "clock": "host wall clock around complete calls",
           "global_map_config": [1000.0, 10.0, 1.0], "chunk_points": 1 << 22, "out_stride": 32, "stores": rows,
           "unmeasured": ["the export kernel alone (its time is the transfer: it writes pinned host memory)",
                          "the host copy out of the staging buffers alone", "a caller's buffer that is itself pinned", "PCL itself"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
