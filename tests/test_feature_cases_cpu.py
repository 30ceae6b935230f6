"""The sweeps of tests/feature_cases.py, the part that needs no GPU: for every named case the oracle's own outputs show
that the case reaches the edge it is named for (so tests/test_gpu_features_edges.py cannot pass vacuously), and the small
cases pin the oracle against the Python transcription of tests/test_oracle_features.py on these shapes.  Every test prints
the count that proves its edge (pytest -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_cases as F                                 # noqa: E402
from test_oracle_features import _py_features             # noqa: E402


def _by_id(name):
    return {c["id"]: c for c in F.cases(name)}


def test_generator_rules():
    sw = F.make_sweep([0, 12, 70, 3, 400], "gaps", "uniform", 1)
    assert list(sw["start_ring"]) == [4, 4, 16, 86, 89] and list(sw["end_ring"]) == [-6, 6, 76, 79, 479]
    assert len(sw["cloud"]) == 485 and sw["cloud"].dtype == np.float32 and np.isfinite(sw["cloud"]).all()
    d = np.abs(np.diff(F._columns(4096, "gaps", np.random.default_rng(0))))
    assert set(d) == {1, 10, 11}
    ext = F._columns(100, "extreme", np.random.default_rng(0))
    assert ext.min() == -32768 and ext.max() == 32767
    again = F.make_sweep([0, 12, 70, 3, 400], "gaps", "uniform", 1)
    assert all(np.array_equal(sw[k], again[k]) for k in ("cloud", "col", "range"))        # a seed is a sweep
    for rule in F.RANGE_RULES:
        r = F.make_sweep([500], "ramp", rule, 2)["range"]
        assert np.isfinite(r).all() and r.min() > 0.5


def test_shared_cell(oracle):
    cases = F.cases("shared_cell")
    for prefix, rings in (("shared_cell-", F.SHARED_RINGS), ("shared_cell_long-", F.SHARED_LONG_RINGS)):
        total = 0
        mine = [c for c in cases if c["id"].startswith(prefix)]
        assert len(mine) == 3
        for c in mine:
            sw = c["sweep"]
            assert sw["lengths"] == rings and set(sw["col"]) == set(range(8))
            found = F.shared_cells(oracle, sw)
            print(f"{c['id']}: last point of ring A picked by ring B alone at {found}")
            assert len(found) >= 2
            assert all(cell == sw["end_ring"][a] + 5 for a, cell in found)
            if prefix == "shared_cell_long-":                  # ... and behind a ring that takes long to finish
                assert sum(sw["lengths"][a] >= 3000 for a, _ in found) >= 2
            total += len(found)
        assert total >= 5


def test_corner_cap(oracle):
    c, = F.cases("corner_cap")
    ref = F.reference(oracle, c)
    rows = F.sector_report(ref, c["sweep"], 1.0)
    comb = [r for r in rows if r[0] == 0]
    capped = [r for r in comb if r[3] == 20 and r[5] > 0]     # 20 corners and candidates left over: the 21st visit broke the loop
    print("corner_cap: comb sectors (corners, above, left over):", [(r[3], r[4], r[5]) for r in comb])
    assert len(capped) >= 1 and all(r[4] > 20 for r in capped)
    spike = [r for r in rows if r[0] == 1]
    print("corner_cap: spike sectors (corners, above, left over):", [(r[3], r[4], r[5]) for r in spike])
    # isolated spikes 12 apart: each is unpicked when visited, so `above` is the number of candidates at the time of visit
    assert [r[4] for r in spike] == list(F.CAP_SPIKES)
    assert [r[3] for r in spike] == [min(m, 20) for m in F.CAP_SPIKES]
    assert [r[5] for r in spike] == [max(m - 20, 0) for m in F.CAP_SPIKES]


def test_chunk_edges(oracle):
    total = {}
    for c in F.cases("chunk_edges"):
        sw = c["sweep"]
        sizes = [sorted({ep - sp for sp, ep in F.sectors(s, e)}) for s, e in zip(sw["start_ring"], sw["end_ring"])]
        assert sizes == [[m] for m in F.CHUNK_SIZES]           # six sectors of exactly m sorted elements, m + 1 visits
        ref = F.reference(oracle, c)
        late = {1: 0, -1: 0}                                   # picks made at visit 64 or later: only a second chunk finds them
        for s, e in zip(sw["start_ring"], sw["end_ring"]):
            for sp, ep in F.valid_sectors(s, e):
                for lab in (1, -1):
                    late[lab] += sum(v >= 64 for v in F.visits_of_picks(ref, sp, ep, lab))
        print(f"{c['id']}: sector sizes {[s[0] for s in sizes]}, corners {int((ref['label'] == 1).sum())}, "
              f"surfaces {int((ref['label'] == -1).sum())}, picked at visit >= 64: {late[1]} corners, {late[-1]} surfaces")
        assert late[1] + late[-1] >= 10
        total = {k: total.get(k, 0) + v for k, v in late.items()}
    assert total[1] >= 10 and total[-1] >= 10


def test_sort_sizes(oracle):
    by = _by_id("sort_sizes")
    for cid in ("sort_sizes-keys", "sort_sizes-keys-comb"):
        sw = by[cid]["sweep"]
        keys = [F.key_count(s, e) for s, e in zip(sw["start_ring"], sw["end_ring"])]
        print(f"{cid}: ring lengths {sw['lengths']}, sort sizes {keys}")
        assert keys == list(F.KEY_COUNTS)
    sw = by["sort_sizes-lists"]["sweep"]
    lists = [len(l) for l in F.candidate_lists(F.reference(oracle, by["sort_sizes-lists"]), sw)]
    print(f"sort_sizes-lists: ring lengths {sw['lengths']}, surface candidate lists {lists}")
    assert lists == list(F.LIST_LENGTHS)


def test_longest_ring(oracle):
    for c in F.cases("longest_ring"):
        sw = c["sweep"]
        i = int(np.argmax(sw["lengths"]))
        assert sw["lengths"][i] == F.MAX_RING == sw["end_ring"][i] - sw["start_ring"][i] + 10
        ref = F.reference(oracle, c)
        s, e = sw["start_ring"][i], sw["end_ring"][i]
        n_lab = int((ref["label"][s:e + 1] != 0).sum())
        print(f"{c['id']}: ring {i} of {sw['lengths']} holds {F.MAX_RING} points, window [{max(s - 5, 0)}, {e + 4}], {n_lab} labelled")
        assert n_lab > 20
    too = F.too_long_sweep()
    assert max(too["lengths"]) == F.MAX_RING + 1


def test_ties(oracle):
    c, = F.cases("ties")
    thr = c["cfg"]["edgeThreshold"]
    assert thr == c["cfg"]["surfThreshold"] and np.float32(thr) == thr
    ref = F.reference(oracle, c)
    at = ref["curvature"] == np.float32(thr)
    idle = at & (ref["picked"] == 0)
    print(f"ties: threshold {thr}, {int(at.sum())} points have exactly that curvature, {int(idle.sum())} of them stay unpicked")
    assert at.sum() >= 50
    assert (ref["label"][at] == 0).all()                       # `>` and `<` are strict: never a corner, never a surface
    assert idle.sum() >= 5                                     # ... although nothing else stood in their way
    assert (ref["label"] == 1).sum() > 0 and (ref["label"] == -1).sum() > 0


def test_one_voxel(oracle):
    by = _by_id("one_voxel")
    c = by["one_voxel-0.2"]
    sw, ref = c["sweep"], F.reference(oracle, c)
    lists = F.candidate_lists(ref, sw)
    outs = [oracle.voxel_grid(sw["cloud"][l], 0.2)[0] for l in lists]
    counts = [(len(l), len(o)) for l, o in zip(lists, outs)]
    print("one_voxel-0.2: per ring (candidates, after the filter):", counts)
    assert counts[1][0] > 100 and counts[1][1] == 1                            # one voxel
    assert counts[3][0] > 100 and counts[3][1] == counts[3][0]                 # index overflow: passed through
    assert np.array_equal(outs[3], sw["cloud"][lists[3]])
    for i in (0, 2, 4):
        assert 1 < counts[i][1] < counts[i][0]                                 # filtered normally
    assert np.array_equal(ref["surface"], np.concatenate(outs))
    n = {cid: len(F.reference(oracle, by[cid])["surface"]) for cid in by}
    print("one_voxel: surface points per leaf:", n)
    assert n["one_voxel-50"] < n["one_voxel-0.2"] < n["one_voxel-1e-4"]


def test_n_scan(oracle):
    want = {"n_scan-1": 1, "n_scan-6": 6, "n_scan-128": 128, "n_scan-1024": 1024}
    for c in F.cases("n_scan"):
        sw = c["sweep"]
        live = int((sw["end_ring"] >= sw["start_ring"]).sum())
        ref = F.reference(oracle, c)
        print(f"{c['id']}: {len(sw['start_ring'])} rings, {live} not empty, {len(sw['cloud'])} points, "
              f"{len(ref['corner'])} corners, {len(ref['surface'])} surface points")
        assert len(sw["start_ring"]) == want[c["id"]] and len(sw["cloud"]) < 30000
        assert len(ref["surface"]) > 0
    sw = _by_id("n_scan")["n_scan-1024"]["sweep"]
    assert 15 <= (sw["end_ring"] >= sw["start_ring"]).sum() <= 22
    assert _by_id("n_scan")["n_scan-6"]["sweep"]["lengths"] == [4000] * 6     # the Livox shape: N_SCAN 6, Horizon_SCAN 4000


def test_steps_known_answers(oracle):
    """Each event of the `steps` rule is alone within +-8 points and the columns are a ramp, so markOccludedPoints has a
    known answer around it: FE:115-121 marks i-5..i, FE:122-128 marks i+1..i+6, FE:133-137 marks i, and only above the gate."""
    c, = F.cases("steps")
    sw = c["sweep"]
    picked = oracle.mark_occluded(sw["range"], sw["col"])
    tally = {}
    for i, kind, side in sw["events"]:
        marked = list(np.nonzero(picked[i - 7:i + 9])[0] + i - 7)
        want = [] if side < 0 else {"up": list(range(i + 1, i + 7)), "down": list(range(i - 5, i + 1)), "beam": [i]}[kind]
        assert marked == want, (i, kind, side)
        tally[(kind, side)] = tally.get((kind, side), 0) + 1
    print("steps: events (kind, side of the gate) ->", tally)
    assert len(tally) == 6 and min(tally.values()) >= 3
    d = np.abs(np.diff(sw["range"].astype(np.float64)))
    assert ((d > 0.2999) & (d < 0.3001)).sum() >= 20 and ((d > 0.1999) & (d < 0.2001)).sum() >= 20
    assert not np.isin(d, [np.float32(0.3), np.float32(0.2)]).any()


SMALL = [("sort_sizes", "sort_sizes-lists"), ("chunk_edges", "chunk_edges-comb"), ("chunk_edges", "chunk_edges-quantised"),
         ("steps", "steps"), ("ties", "ties")]


@pytest.mark.parametrize("name,cid", SMALL, ids=[s[1] for s in SMALL])
def test_small_cases_against_python_transcription(oracle, name, cid):
    c = _by_id(name)[cid]
    sw, cfg = c["sweep"], F.oracle_cfg(c["cfg"])
    ref = F.reference(oracle, c)
    curv, picked, label, corners, ring_lists = _py_features(sw["cloud"], sw["start_ring"], sw["end_ring"], sw["col"], sw["range"],
                                                            edge_thr=cfg["edge_threshold"], surf_thr=cfg["surf_threshold"])
    np.testing.assert_array_equal(ref["curvature"], curv)
    np.testing.assert_array_equal(ref["picked"], picked)
    np.testing.assert_array_equal(ref["label"], label)
    np.testing.assert_array_equal(ref["corner"], sw["cloud"][corners])
    assert ring_lists == F.candidate_lists(ref, sw)
    surf = [oracle.voxel_grid(sw["cloud"][l], cfg["surf_leaf"])[0] for l in ring_lists if len(l)]
    np.testing.assert_array_equal(ref["surface"], np.concatenate(surf))
    print(f"{cid}: {len(sw['cloud'])} points, {len(corners)} corners, {int((label == -1).sum())} surfaces: "
          "oracle == Python transcription")
