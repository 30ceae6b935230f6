"""numpy restatement (fp32, no contraction) of publishGlobalMap MO:992-1041 and saveMapService MO:935-957, from the
project's oracle calls `voxel_grid` and `transform_point_cloud`: the checker of tests/test_gpu_globalmap.py, pinned by
tests/test_globalmap_cpu.py against `literal`, a per-line Python loop of the same lines.

Conventions: the radius set is strict (d2 < (float)((double)R * R)) and ordered by (d2, i); the
pose filter sees (x, y, z, intensity = i); a centroid is relabelled to its nearest key pose over all N, ties to the lowest
index; the recheck of MO:1030 drops a centroid whose own distance to the last key pose is > R (strict); a keyframe that
two centroids relabel to is summed twice."""
import numpy as np


def select(oracle, poses, R=1000.0, density=10.0):
    """MO:1011-1031 -> (ids int32 [m] of the keyframes MO:1033 sums, in order, duplicates included;
    info dict: n_hits, n_centroids, pose_passthrough, n_rechecked_out)."""
    P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 6)[:, 3:6])
    n = len(P)
    if n == 0:
        return np.zeros(0, np.int32), dict(n_hits=0, n_centroids=0, pose_passthrough=0, n_rechecked_out=0)
    last = n - 1
    R32 = np.float32(R)
    r2 = np.float32(np.float64(R32) * np.float64(R32))                 # what PCL hands FLANN
    d = P - P[last]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    hit = np.nonzero(d2 < r2)[0]
    hit = hit[np.lexsort((hit, d2[hit]))]
    rec = np.concatenate([P[hit], hit.astype(np.float32)[:, None]], 1)
    cent, rc = oracle.voxel_grid(rec, np.float32(density))
    cent = cent[:, :3]
    ids = np.zeros(len(cent), np.int32)
    for k, c in enumerate(cent):
        e = c[None, :] - P
        ids[k] = int(np.argmin((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]))   # first occurrence: lowest index
    e = cent - P[last]
    dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    keep = ~(dist > R32)
    return ids[keep], dict(n_hits=len(hit), n_centroids=len(cent), pose_passthrough=int(rc == 1), n_rechecked_out=int((~keep).sum()))


def literal(oracle, poses, R=1000.0, density=10.0):
    """MO:1011-1033 line by line: a brute-force radius search (FLANN's sorted result set), scalar fp32."""
    f = np.float32
    key3 = [(f(p[3]), f(p[4]), f(p[5])) for p in np.asarray(poses, np.float32).reshape(-1, 6)]     # cloudKeyPoses3D
    if not key3:                                                       # MO:997
        return np.zeros(0, np.int32)
    back = key3[-1]
    r2 = f(float(f(R)) * float(f(R)))

    def sqdist(a, b):
        dx, dy, dz = f(a[0] - b[0]), f(a[1] - b[1]), f(a[2] - b[2])
        return f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))

    found = [(sqdist(p, back), i) for i, p in enumerate(key3) if sqdist(p, back) < r2]             # radiusSearch MO:1012
    found.sort()
    key_poses = [(key3[i][0], key3[i][1], key3[i][2], f(i)) for _, i in found]                     # MO:1015-1016
    ds, _ = oracle.voxel_grid(np.asarray(key_poses, np.float32).reshape(-1, 4), f(density))        # MO:1018-1021
    out = []
    for pt in ds:
        best = min((sqdist(pt, p), i) for i, p in enumerate(key3))                                 # nearestKSearch(pt, 1) MO:1024
        if f(np.sqrt(sqdist(pt, back))) > f(R):                                                    # MO:1030
            continue
        out.append(best[1])                                                                        # MO:1032
    return np.asarray(out, np.int32)


def summed(oracle, clouds, poses, ids):
    """sum over ids of transformPointCloud(surfCloudKeyFrames[i], cloudKeyPoses6D[i]) -> [n,4]."""
    poses = np.asarray(poses, np.float32).reshape(-1, 6)
    parts = [oracle.transform_point_cloud(clouds[i], poses[i]) for i in ids if len(clouds[i])]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 4), np.float32)


def global_map(oracle, clouds, poses, R=1000.0, density=10.0, leaf=1.0):
    """MO:992-1041 -> (globalMapKeyFramesDS [m,4], ids, info with n_summed and voxel_passthrough added)."""
    ids, info = select(oracle, poses, R, density)
    world = summed(oracle, clouds, poses, ids)
    info["n_summed"] = len(world)
    if len(world) == 0:
        info["voxel_passthrough"] = 0
        return world, ids, info
    ds, rc = oracle.voxel_grid(world, np.float32(leaf))
    info["voxel_passthrough"] = int(rc == 1)
    return ds, ids, info


def export_map(oracle, clouds, poses, resolution=0.0):
    """MO:935-957 -> (globalSurfCloud [n,4], its filtered copy or None when resolution == 0, voxel_passthrough)."""
    full = summed(oracle, clouds, poses, range(len(clouds)))
    if resolution == 0 or len(full) == 0:
        return full, (None if resolution == 0 else np.zeros((0, 4), np.float32)), 0
    ds, rc = oracle.voxel_grid(full, np.float32(resolution))
    return full, ds, int(rc == 1)


# ------------------------------------------------------------------ the fixed cases of the GPU tests
def curved_path(n=300, seed=0):
    """~n key poses on a curved path that comes back on itself (several poses per 4 m voxel, the start far from the end)
    and tiny clouds of 0 to 40 points."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 2.6 * np.pi, n)
    poses = np.zeros((n, 6), np.float32)
    poses[:, 3] = (45.0 + 4.0 * np.sin(3 * a)) * np.sin(a) + rng.normal(0, 0.3, n)
    poses[:, 4] = (45.0 + 4.0 * np.sin(3 * a)) * (1 - np.cos(a)) + rng.normal(0, 0.3, n)
    poses[:, 5] = 1.8 + rng.normal(0, 0.1, n)
    poses[:, 0:2] = rng.normal(0, 0.03, (n, 2))
    poses[:, 2] = a
    clouds = []
    for k in range(n):
        m = int(rng.integers(0, 41))
        xyz = rng.uniform(-1, 1, (m, 3)) * np.array([12.0, 8.0, 2.0])
        clouds.append(np.concatenate([xyz, rng.uniform(0, 255, (m, 1))], 1).astype(np.float32))
    return poses, clouds


CURVED_SEED = 0            # searched in tests/test_globalmap_cpu.py's terms (its docstring); hard-coded here
CURVED_R, CURVED_DENSITY, CURVED_LEAF = 60.0, 4.0, 0.5


def export_case(n_kf=40, seed=5):
    """Keyframes whose sizes cross the 256-point workgroup of the export kernel, under random poses."""
    rng = np.random.default_rng(seed)
    sizes = rng.choice([0, 1, 255, 256, 257, 1000], n_kf)
    sizes[0], sizes[-1] = 0, 0                                          # empty keyframes at both ends, and wherever else
    poses = np.zeros((n_kf, 6), np.float32)
    poses[:, :3] = rng.uniform(-np.pi, np.pi, (n_kf, 3)) * np.array([0.2, 0.2, 1.0])
    poses[:, 3:] = rng.uniform(-30, 30, (n_kf, 3))
    clouds = []
    for m in sizes:
        xyz = rng.uniform(-1, 1, (int(m), 3)) * np.array([12.0, 8.0, 2.0])
        clouds.append(np.concatenate([xyz, rng.uniform(0, 255, (int(m), 1))], 1).astype(np.float32))
    return poses, clouds
