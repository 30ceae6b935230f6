"""Cost of the signed distance field on the device at the planning size: a 0.2 m grid of 425 x 425 cells (an 85 m square) with
a 3 m band from the terrain's minimum, i.e. 15 layers: rolling ground with noise, 60 boxes and walls.

Times: host wall clock around calls that end complete (every entry point does), medians of --reps runs, the forms
alternating.  lio_sdf_build whole (grid up, statistics, two sweeps, stencil); its stages from lio_sdf_debug_stage_ms (HIP
events on the build's stream: the layer statistics with their host wait, the column sweeps, the row sweeps, the node
stencil); lio_sdf_query per 10^5 positions with and without the derivative; lio_sdf_nodes (the copy of the field);
lio_occupancy_sdf on the occupancy of the same grid at 0.5 m above its median.  Beside them lio_kf_store_sdf and
lio_kf_store_terrain_map on one local map (the newest 30 keyframes of 64 x 1800 sweeps, the default crop, fill_holes 1).
The single-thread host time of the same arithmetic comes from tools/sdf_host_check.cpp on the same grid:

    python tools/sdf_cost.py --write-grid /tmp/sdf_grid.f32                     (no GPU needed)
    hipcc -x hip --offload-arch=gfx950 -O3 -ffp-contract=off tools/sdf_host_check.cpp -o /tmp/sdf_host_check
    /tmp/sdf_host_check time 425 425 0.2 3.0 /tmp/sdf_grid.f32 > /tmp/sdf_host.json
    python tools/sdf_cost.py [--reps 20] [--host-json /tmp/sdf_host.json] [--out profiles/sdf_cost.json]

It is a reported baseline, not a target; no time is fixed in advance.
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

ROWS, COLS, RES, BAND = 425, 425, 0.2, 3.0


def scene(seed=5):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(ROWS) * RES, np.arange(COLS) * RES, indexing="ij")
    z = 0.4 * np.sin(0.08 * x) * np.cos(0.06 * y) + 0.01 * x + rng.normal(0, 0.02, x.shape)
    for _ in range(60):
        r, c = rng.integers(0, ROWS - 40), rng.integers(0, COLS - 40)
        z[r:r + rng.integers(2, 40), c:c + rng.integers(2, 40)] += rng.uniform(0.3, 2.5)
    return np.asfortranarray(z.astype(np.float32))


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1000.0 * (time.perf_counter() - t0))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--write-grid", default="")
    ap.add_argument("--host-json", default="")
    ap.add_argument("--keyframes", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_cost.json"))
    args = ap.parse_args()
    grid = scene()
    if args.write_grid:
        grid.ravel(order="F").tofile(args.write_grid)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("sdf_cost.py needs a GPU (no CPU fallback)")
    pkg = importlib.import_module("lio-slam_amd")
    synth = importlib.import_module("lio-slam_amd.synth")
    lib = pkg.load_library()
    lo = float(grid.min())
    cfg = pkg.sdf_default_config(min_height=lo, max_height=lo + BAND)
    sdf = pkg.Sdf()
    length, position = (ROWS * RES, COLS * RES), (12.5, -3.0)
    info = sdf.build(grid, RES, length, position, cfg)
    n_nodes = info.rows * info.cols * info.layers
    rng = np.random.default_rng(2)
    pos = np.c_[rng.uniform(position[0] - 45, position[0] + 45, 100000), rng.uniform(position[1] - 45, position[1] + 45, 100000),
                rng.uniform(lo - 0.5, lo + BAND + 0.5, 100000)]
    occ = ((grid > np.median(grid) + 0.5) * 100).astype(np.int8).T.copy()                  # [height, width] as the message
    nodes = np.empty(4 * n_nodes, np.float32)
    stage = (C.c_float * 4)()
    stages = []

    def build_staged():
        lib.lio_sdf_debug_stage_ms(1, None)
        sdf.build(grid, RES, length, position, cfg)
        lib.lio_sdf_debug_stage_ms(0, stage)
        stages.append(list(stage))

    forms = {
        "sdf_build_ms": lambda: sdf.build(grid, RES, length, position, cfg),
        "sdf_build_with_stage_events_ms": build_staged,
        "sdf_query_1e5_ms": lambda: sdf.query(pos),
        "sdf_query_1e5_no_derivative_ms": lambda: sdf.query(pos, want_derivative=False),
        "sdf_nodes_copy_ms": lambda: lib.lio_sdf_nodes(sdf.h, nodes.ctypes.data, nodes.size),
        "occupancy_sdf_ms": lambda: pkg.occupancy_sdf(occ, RES),
    }
    # one local map for the chain: lio_kf_store_sdf beside lio_kf_store_terrain_map
    case = synth.make_case("hdl64", n_keyframes=args.keyframes, seed=21, device="cuda")
    st = pkg.KeyframeStore()
    for cloud, _ in case["keyframes"]:
        st.add(np.concatenate([cloud, np.zeros((len(cloud), 1), np.float32)], 1))
    poses = np.array([p for _, p in case["keyframes"]], np.float32)
    st.set_poses(0, poses, times=np.arange(len(poses)) * 1.0)
    pose = poses[-1]
    lm = pkg.local_map_default_config(n_keyframes=args.keyframes)
    hm = pkg.height_map_default_config(roll=float(pose[0]), pitch=float(pose[1]), fill_holes=1)
    chain = pkg.Sdf()
    grid_c, hm_info, _ = st.height_map(pose, lm, hm)
    lo_c = float(np.nanmin(grid_c))
    cfg_c = pkg.sdf_default_config(min_height=lo_c, max_height=lo_c + BAND, nan_policy=1)
    tcfg = pkg.terrain_default_config(normal_radius=0.5, smooth_radius=0.6, edge_window_length=0.5)
    _, info_c, _, _ = st.sdf_map(chain, pose, lm, hm, cfg_c)
    forms["kf_store_sdf_ms"] = lambda: st.sdf_map(chain, pose, lm, hm, cfg_c)
    forms["kf_store_sdf_no_grid_ms"] = lambda: st.sdf_map(chain, pose, lm, hm, cfg_c, want_grid=False)
    forms["kf_store_height_map_ms"] = lambda: st.height_map(pose, lm, hm)
    forms["kf_store_terrain_map_ms"] = lambda: st.terrain_map(pose, lm, hm, tcfg)
    for fn in forms.values():
        fn()                                                    # warm-up: the pool, the code objects, the buffers
    stages.clear()
    samples = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():                          # alternating
            samples[name].append(median_ms(fn, 1))
    med = {name: float(np.median(v)) for name, v in samples.items()}
    st_med = np.median(np.array(stages), axis=0)
    res = {
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": ROWS, "cols": COLS, "resolution": RES, "band": BAND,
        "layers": info.layers, "nodes": n_nodes, "node_bytes": 16 * n_nodes,
        "layer_modes": {"all_obstacle": info.n_all_obstacle, "all_free": info.n_all_free, "mixed": info.n_mixed},
        "lines": {"column_sweep": 2 * info.layers * COLS, "row_sweep": 2 * info.layers * ROWS},
        "clock": "host wall clock around calls that end complete; stages: HIP events on the build's stream", **med,
        "sdf_build_stages_ms": dict(zip(("layer_statistics_and_host_wait", "column_sweeps", "row_sweeps", "node_stencil"), map(float, st_med))),
        "chain": {"keyframes": args.keyframes, "rows": info_c.rows, "cols": info_c.cols, "layers": info_c.layers, "n_nan_cells_filled": info_c.n_nan,
                  "height_map_points": hm_info.n_in},
        "unmeasured": ["the kernels under a profiler (no rocprofv3 pass)", "the lower-bound stack in LDS against the global workspace (only the global form is built)",
                       "grid_map_sdf itself, which needs Eigen"],
    }
    if args.host_json:
        res["host_single_thread_same_arithmetic"] = json.loads(open(args.host_json).read().strip().splitlines()[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))
    chain.close(); sdf.close(); st.close()


if __name__ == "__main__":
    main()
