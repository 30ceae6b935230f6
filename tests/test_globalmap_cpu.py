"""The global map and the map export without a GPU: the restatement of tests/globalmap_restate.py against its per-line
form, the two new structs against C, the defaults against the yaml literals, and the fixed cases of
tests/test_gpu_globalmap.py for what they must contain.

The curved path's seed was searched here, on the CPU, under the restatement alone: the first seed from 0 upwards for
which the case at (R, density) = (60, 4) holds a key pose outside the radius, a voxel with two or more poses and a keyframe
that two centroids relabel to, and for which a density of 1e-3 makes the pose filter pass its input through.  Seed 0
meets all four; it is hard-coded as globalmap_restate.CURVED_SEED."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import globalmap_restate as G                                  # noqa: E402

PASS_DENSITY = 1e-3        # 60 m / 1e-3 per axis: the pose filter's voxel index overflows 2^31 (and stays inside int64)


def test_struct_layouts_match_c(pkg):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "liogpu.h"
    int main(void) {
        printf("%zu %zu %zu %zu\n", sizeof(lio_global_map_config), offsetof(lio_global_map_config, search_radius),
               offsetof(lio_global_map_config, pose_density), offsetof(lio_global_map_config, leaf));
        printf("%zu %zu %zu %zu %zu\n", sizeof(lio_global_map_info), offsetof(lio_global_map_info, n_keyframes),
               offsetof(lio_global_map_info, n_summed), offsetof(lio_global_map_info, n_out), offsetof(lio_global_map_info, voxel_passthrough));
        printf("%zu %zu %zu\n", sizeof(lio_export_config), offsetof(lio_export_config, resolution), offsetof(lio_export_config, chunk_points));
        printf("%d %d\n", (int)LIO_STAGED_DS, (int)LIO_STAGED_RAW);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    g, i, e = pkg.GlobalMapConfig, pkg.GlobalMapInfo, pkg.ExportConfig
    assert out[:4] == [C.sizeof(g), g.search_radius.offset, g.pose_density.offset, g.leaf.offset]
    assert out[4:9] == [C.sizeof(i), i.n_keyframes.offset, i.n_summed.offset, i.n_out.offset, i.voxel_passthrough.offset]
    assert out[9:12] == [C.sizeof(e), e.resolution.offset, e.chunk_points.offset]
    assert out[12:] == [pkg.STAGED_DS, pkg.STAGED_RAW]


def test_defaults_are_the_yaml_literals(pkg):
    import importlib
    cfg = pkg.global_map_default_config()
    assert (cfg.search_radius, cfg.pose_density, cfg.leaf) == (1000.0, 10.0, 1.0)     # globalMapVisualization*, all yaml files
    api = importlib.import_module("lio-slam_amd.api")
    assert {"lio_global_map_default_config", "lio_kf_store_global_map", "lio_kf_store_export_map", "lio_kf_store_get_keyframe",
            "lio_s2m_registered_cloud"} <= set(api.EXPORTS)


def test_new_calls_refuse_null_and_bad_arguments_without_a_device(pkg):
    L = pkg.load_library()
    cfg, ecfg = pkg.global_map_default_config(), pkg.ExportConfig(0.0, 0)
    n_ids, n, m, v = C.c_int32(), C.c_size_t(), C.c_size_t(), C.c_int32()
    assert L.lio_kf_store_global_map(None, C.byref(cfg), None, 0, C.byref(n_ids), None, 32, 0, C.byref(n), None) == -1
    assert L.lio_kf_store_export_map(None, C.byref(ecfg), None, 32, 0, C.byref(n), None, 32, 0, C.byref(m), C.byref(v)) == -1
    assert L.lio_kf_store_get_keyframe(None, 0, None, None, 32, 0, C.byref(n)) == -1
    assert L.lio_s2m_registered_cloud(None, 0, None, None, 32, 0, C.byref(n)) == -1


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_agrees_with_the_literal_loop(oracle, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    poses = np.zeros((n, 6), np.float32)
    poses[:, 3:6] = np.cumsum(rng.normal(0, 1.5, (n, 3)), 0).astype(np.float32)
    poses[:, 3:6] = np.round(poses[:, 3:6] * 2) / 2                     # repeated positions: ties in the relabel
    for R, dens in [(1000.0, 10.0), (6.0, 2.0), (3.5, 0.5), (6.0, PASS_DENSITY)]:
        ids, _ = G.select(oracle, poses, R, dens)
        assert ids.tolist() == G.literal(oracle, poses, R, dens).tolist()


def test_restatement_agrees_with_the_literal_loop_on_the_gpu_cases(oracle):
    poses, _ = G.curved_path(seed=G.CURVED_SEED)
    for R, dens in [(G.CURVED_R, G.CURVED_DENSITY), (G.CURVED_R, PASS_DENSITY)]:
        ids, _ = G.select(oracle, poses, R, dens)
        assert ids.tolist() == G.literal(oracle, poses, R, dens).tolist()
    for P in (poses[:1], poses[:0]):
        assert G.select(oracle, P)[0].tolist() == G.literal(oracle, P).tolist() == list(range(len(P)))


def test_radius_boundary_is_strict_and_the_recheck_is_not(oracle):
    # (30, 40, 0) from the origin: d2 == 2500 == r2 exactly -> not in the radius set
    poses = np.zeros((2, 6), np.float32)
    poses[0, 3:6] = (30.0, 40.0, 0.0)
    ids, info = G.select(oracle, poses, 50.0, 1.0)
    assert ids.tolist() == [1] and info["n_hits"] == 1
    # two poses in one voxel whose centroid is nearer to the farther one: relabelled there, and kept (the recheck is on the
    # centroid's own coordinates, not on the relabelled pose's)
    poses = np.zeros((3, 6), np.float32)
    poses[:, 3] = (9.0, 1.0, 0.0)
    ids, info = G.select(oracle, poses, 9.5, 10.0)
    assert info["n_hits"] == 3 and info["n_centroids"] == 1 and ids.tolist() == [1]


def _curved_facts(oracle, seed):
    poses, clouds = G.curved_path(seed=seed)
    ids, info = G.select(oracle, poses, G.CURVED_R, G.CURVED_DENSITY)
    d = np.linalg.norm(poses[:, 3:6].astype(np.float64) - poses[-1, 3:6].astype(np.float64), axis=1)
    _, pinfo = G.select(oracle, poses, G.CURVED_R, PASS_DENSITY)
    return dict(outside=int((d > G.CURVED_R + 1e-3).sum()), shared_voxels=info["n_hits"] - info["n_centroids"],
                duplicates=len(ids) - len(set(ids.tolist())), passthrough=pinfo["pose_passthrough"],
                pass_ids=pinfo["n_centroids"], n_hits=pinfo["n_hits"], sizes={len(c) for c in clouds})


def test_the_curved_path_contains_what_the_gpu_tests_need(oracle):
    f = _curved_facts(oracle, G.CURVED_SEED)
    assert f["outside"] >= 1                       # a key pose outside the radius
    assert f["shared_voxels"] >= 1                 # a voxel with two or more poses
    assert f["duplicates"] >= 1                    # a keyframe selected twice
    assert f["passthrough"] == 1 and f["pass_ids"] == f["n_hits"]     # the pose filter passes its input through
    assert 0 in f["sizes"] and max(f["sizes"]) <= 40
    first = next(s for s in range(64) if all((lambda g: (g["outside"], g["shared_voxels"], g["duplicates"], g["passthrough"]))(
        _curved_facts(oracle, s))))
    assert first == G.CURVED_SEED


def test_the_export_case_crosses_every_boundary(oracle):
    poses, clouds = G.export_case()
    sizes = [len(c) for c in clouds]
    assert set(sizes) == {0, 1, 255, 256, 257, 1000} and sizes[0] == 0 and sizes[-1] == 0
    total = sum(sizes)
    assert total > 3 * 768 and total % 256 != 0 and total % 768 != 0          # several chunks of 256 and 768, a ragged last one
    starts = np.cumsum([0] + sizes[:-1])
    assert any(s % 256 and n for s, n in zip(starts, sizes))                  # a chunk starts in the middle of a keyframe
    full, ds, vpt = G.export_map(oracle, clouds, poses, 0.5)
    assert len(full) == total and 0 < len(ds) < total and vpt == 0
    assert G.export_map(oracle, clouds, poses, 0.0)[1] is None
    # the cloud filter overflows at a millimetre leaf: the sum passes through
    assert G.export_map(oracle, clouds, poses, 1e-3)[2] == 1
