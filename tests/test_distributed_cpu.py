"""world_size-2 gloo test of the map-sharding logic, CPU only.

Each rank holds its slab of the map + a one-cell halo, runs the oracle's
surfOptimization on the shard for the scan points it owns, and the ranks
exchange (a) the correspondence sets and (b) the 28 normal-equation sums.
Claims checked: every scan point has exactly one owner; the union of the
per-rank correspondences equals the unsharded ones BIT-EXACTLY (flags,
coefficients, global neighbour indices); the all-reduced sums equal the
unsharded sums; the pose after the step is identical on every rank.
"""
import importlib
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows(oracle, pose, scan, coeff, flag):
    """Jacobian rows of the accepted correspondences -> 28 sums in fp64."""
    sums = np.zeros(28)
    for i in np.nonzero(flag)[0]:
        row, rhs = oracle.jacobian_row(pose, scan[i], coeff[i])
        r = row.astype(np.float64)
        sums[:21] += np.outer(r, r)[np.triu_indices(6)]
        sums[21:27] += r * float(rhs)
        sums[27] += 1.0
    return sums


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from oracle.oracle import Oracle
    mg = importlib.import_module("lio-slam_amd.multigpu")
    synth = importlib.import_module("lio-slam_amd.synth")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        case = synth.make_case("vlp16", n_keyframes=6, seed=11, device="cpu")
        map_xyz, query = case["map"], case["queries"][0]
        scan, pose = query["scan"], query["pose_init"]
        orc = Oracle()
        cfg = orc.default_config(knn_mode=1)
        plan = mg.plan_shards(map_xyz, world)
        idx = mg.shard_points(map_xyz, plan, rank)
        T = orc.get_transformation(pose[3], pose[4], pose[5], pose[0], pose[1], pose[2])
        own = mg.owner_mask(mg.transform_f32(T.reshape(12), scan), plan, rank)
        # association on the shard, for owned points only
        flag_s, coeff_s, nn_s = orc.surf_optimization(cfg, pose, scan[own], map_xyz[idx])
        flag = np.zeros(len(scan), np.uint8); coeff = np.zeros((len(scan), 4), np.float32)
        nn = np.full((len(scan), 5), -1, np.int64)
        flag[own] = flag_s; coeff[own] = coeff_s
        nn[own] = np.where(nn_s >= 0, idx[np.clip(nn_s, 0, None)], -1)     # shard-local -> global indices
        sums = _rows(orc, pose, scan, coeff, flag)
        # exchange
        t_own = torch.from_numpy(own.astype(np.int64)); dist.all_reduce(t_own)
        t_flag = torch.from_numpy(flag.astype(np.int64)); dist.all_reduce(t_flag)
        t_coeff = torch.from_numpy(coeff.astype(np.float64)); dist.all_reduce(t_coeff)
        t_nn = torch.from_numpy(np.where(own[:, None], nn, 0)); dist.all_reduce(t_nn)
        t_sums = torch.from_numpy(sums.copy()); dist.all_reduce(t_sums)
        # reference: unsharded
        flag_f, coeff_f, nn_f = orc.surf_optimization(cfg, pose, scan, map_xyz)
        sums_f = _rows(orc, pose, scan, coeff_f, flag_f)
        ok = {
            "one_owner": bool((t_own.numpy() == 1).all()),
            "flags": bool(np.array_equal(t_flag.numpy().astype(np.uint8), flag_f)),
            "coeff": bool(np.array_equal(t_coeff.numpy().astype(np.float32)[flag_f == 1], coeff_f[flag_f == 1])),
            "nn": bool(np.array_equal(t_nn.numpy()[flag_f == 1], nn_f[flag_f == 1])),
            "sums": bool(np.allclose(t_sums.numpy(), sums_f, rtol=1e-12, atol=1e-9)),
            "n_corr": int(t_sums.numpy()[27]), "n_own": int(own.sum()), "n_shard": int(len(idx)),
            "n_map": int(len(map_xyz)),
        }
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_association_matches_unsharded_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in (0, 1):
        ok = res[r]
        assert ok["one_owner"] and ok["flags"] and ok["coeff"] and ok["nn"] and ok["sums"], ok
        assert ok["n_corr"] > 1000
        assert 0 < ok["n_own"] and ok["n_shard"] < ok["n_map"]        # a real split with a real halo
    assert res[0]["n_corr"] == res[1]["n_corr"]


def test_plan_shards_properties():
    mg = importlib.import_module("lio-slam_amd.multigpu")
    rng = np.random.default_rng(0)
    pts = (rng.uniform(-1, 1, (20000, 3)) * np.array([120, 15, 4])).astype(np.float32)
    for world in (1, 2, 4, 8):
        plan = mg.plan_shards(pts, world)
        b = plan["bounds"]
        assert b[0] == 0 and b[-1] == plan["dims"][plan["axis"]] and (np.diff(b) >= 0).all()
        assert plan["axis"] == 0
        total = 0
        for r in range(world):
            idx = mg.shard_points(pts, plan, r)
            own = mg.owner_mask(pts, plan, r)
            total += own.sum()
            assert set(np.nonzero(own)[0]) <= set(idx)               # a rank holds what it owns
            # halo: every point within 1 m (< one cell) of an owned point along the axis is present
            lo = pts[own][:, 0].min() - 1.0 if own.any() else 0
            hi = pts[own][:, 0].max() + 1.0 if own.any() else 0
            need = np.nonzero((pts[:, 0] > lo) & (pts[:, 0] < hi))[0]
            assert set(need) <= set(idx)
        assert total == len(pts)
        counts = [mg.owner_mask(pts, plan, r).sum() for r in range(world)]
        assert max(counts) < 2.0 * len(pts) / world + 500           # balanced slabs
    empty = mg.plan_shards(np.zeros((0, 3), np.float32), 4)
    assert len(mg.shard_points(np.zeros((0, 3), np.float32), empty, 2)) == 0


@pytest.mark.parametrize("axis", [1, 2])
def test_plan_shards_properties_on_the_other_axes(axis):
    """The twin of test_plan_shards_properties for a map that is longest along y or z (a vehicle that drives north-south,
    a shaft): the same properties, read along that axis."""
    mg = importlib.import_module("lio-slam_amd.multigpu")
    rng = np.random.default_rng(0)
    extent = np.roll(np.array([120, 15, 4]), axis)
    pts = (rng.uniform(-1, 1, (20000, 3)) * extent).astype(np.float32)
    for world in (1, 2, 4, 8):
        plan = mg.plan_shards(pts, world)
        b = plan["bounds"]
        assert plan["axis"] == axis
        assert b[0] == 0 and b[-1] == plan["dims"][axis] and (np.diff(b) >= 0).all()
        total = 0
        for r in range(world):
            idx = mg.shard_points(pts, plan, r)
            own = mg.owner_mask(pts, plan, r)
            total += own.sum()
            assert set(np.nonzero(own)[0]) <= set(idx)
            lo = pts[own][:, axis].min() - 1.0 if own.any() else 0
            hi = pts[own][:, axis].max() + 1.0 if own.any() else 0
            need = np.nonzero((pts[:, axis] > lo) & (pts[:, axis] < hi))[0]
            assert set(need) <= set(idx)
        assert total == len(pts)
        counts = [mg.owner_mask(pts, plan, r).sum() for r in range(world)]
        assert max(counts) < 2.0 * len(pts) / world + 500
    # a plan balanced by a load sample, along the same axis
    load = pts[np.abs(pts[:, axis]) < 30]
    p_load = mg.plan_shards(pts, 4, load_xyz=load)
    assert p_load["axis"] == axis and np.all(np.diff(p_load["bounds"]) >= 0)
    c = np.clip(mg.cell_coord(load[:, axis], p_load["origin"][axis], p_load["inv_cell"], p_load["dims"][axis]), 0, p_load["dims"][axis] - 1)
    share = np.array([((c >= p_load["bounds"][r]) & (c < p_load["bounds"][r + 1])).sum() for r in range(4)]) / len(load)
    assert share.max() < 0.25 + 0.03, share


def test_slab_plan_properties():
    """Host logic of the sharded map (lio-slam_amd/multigpu.py): bounds are monotone and cover the grid, a plan balanced by
    a load sample equalises that sample (not the map), a wider halo only ever adds map points, and every map point is held
    by the rank that owns its cell."""
    mg = importlib.import_module("lio-slam_amd.multigpu")
    rng = np.random.default_rng(5)
    # a long map with uniform density, and a "scan load" concentrated in its middle
    map_xyz = np.stack([rng.uniform(0, 300, 60000), rng.uniform(-10, 10, 60000), rng.uniform(0, 5, 60000)], 1).astype(np.float32)
    load = np.stack([rng.normal(150, 25, 40000), rng.uniform(-10, 10, 40000), rng.uniform(0, 5, 40000)], 1).astype(np.float32)
    for world in (2, 4, 8):
        p_map = mg.plan_shards(map_xyz, world)
        p_load = mg.plan_shards(map_xyz, world, load_xyz=load)
        for plan, sample in ((p_map, map_xyz), (p_load, load)):
            b = plan["bounds"]
            assert b[0] == 0 and b[-1] == plan["dims"][plan["axis"]] and np.all(np.diff(b) >= 0) and plan["axis"] == 0
            c = np.clip(mg.cell_coord(sample[:, 0], plan["origin"][0], plan["inv_cell"], plan["dims"][0]), 0, plan["dims"][0] - 1)
            share = np.array([((c >= b[r]) & (c < b[r + 1])).sum() for r in range(world)]) / len(sample)
            assert share.max() < 1.0 / world + 0.03, (world, share)           # balanced by what it was planned from
        # the load-balanced slabs are narrow where the load is and wide at the ends
        if world > 2:                                                          # (two symmetric halves are the same either way)
            assert np.diff(p_load["bounds"]).min() < np.diff(p_map["bounds"]).min()
        for rank in range(world):
            i1 = mg.shard_points(map_xyz, p_load, rank, 1)
            i16 = mg.shard_points(map_xyz, p_load, rank, 16)
            assert set(i1.tolist()) <= set(i16.tolist()) and len(i16) >= len(i1)
            own = mg.owner_mask(map_xyz, p_load, rank)
            assert own[i1].sum() == own.sum()                                  # every owned point is in the held set
    # the plan cell follows the gate radius (the device-side owner test derives its cell from the same fields)
    assert abs(float(mg.default_cell(0.49)) - 0.7 * 1.001) < 1e-6
