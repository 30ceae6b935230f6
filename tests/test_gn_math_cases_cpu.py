"""The designed classes of tests/gn_math_cases.py, on the oracle alone (no GPU):
  * the split of the oracle moved nothing: lo_lm_step after the normal equations equals lo_lm_optimization on real
    correspondence sets, lo_corner_fit equals lo_corner_optimization on the corner case of tests/test_gpu_corner.py;
  * every class reaches what it is named after;
  * every 6x6 case has finite oracle outputs in every word (the cap is 100 %: the device step is not defined past it)."""
import ctypes as C

import numpy as np
import pytest

import gn_math_cases as G

N_CPU = 4096
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the split
@pytest.fixture(scope="module")
def corridor_case(synth):
    return synth.make_case("vlp16", n_keyframes=4, seed=22, kind="corridor", device="cpu")


def _lm_both_ways(oracle, case, it):
    """lo_lm_optimization on the correspondences of iteration `it` of a registration, and lo_lm_step on its normal equations."""
    q = case["queries"][0]
    cfg = oracle.default_config(knn_mode=1, n_threads=4)
    pose_end, res, matP_end, corr = oracle.scan2map(cfg, q["scan"], case["map"], q["pose_init"], corr_iter=it)
    assert res.iters > it and res.n_corr_iter[it] >= cfg.min_corr
    flag, coeff, _ = corr
    sel = flag == 1
    ori = np.ascontiguousarray(np.asarray(q["scan"], np.float32)[:, :3][sel])
    cf = np.ascontiguousarray(coeff[sel])
    pose0 = np.array(q["pose_init"], np.float32) if it == 0 else np.array(res.pose_iter[it - 1], np.float32)
    # the members as they stand before iteration `it`: untouched before the first, the first iteration's afterwards
    matP0 = np.zeros(36, np.float32) if it == 0 else matP_end.reshape(36).copy()
    deg0 = 0 if it == 0 else int(res.is_degenerate)
    pose_a, matP_a, deg_a = pose0.copy(), matP0.copy(), np.array([deg0], np.int32)
    AtA, AtB = np.zeros(36, np.float32), np.zeros(6, np.float32)
    conv_a = oracle.lib.lo_lm_optimization(C.byref(cfg), it, ori.reshape(-1), cf.reshape(-1), len(ori), pose_a, matP_a, deg_a, AtA, AtB)
    assert np.array_equal(_bits(pose_a), _bits(np.array(res.pose_iter[it], np.float32))), "not the registration's own iteration"
    pose_b, matP_b, deg_b, conv_b = oracle.lm_step(cfg, it, AtA, AtB, pose0, matP0, deg0)
    return (pose_a, matP_a.reshape(6, 6), int(deg_a[0]), int(conv_a)), (pose_b, matP_b, deg_b, conv_b)


@pytest.mark.parametrize("which", ["street", "corridor"])
@pytest.mark.parametrize("it", [0, 2])
def test_lm_step_is_the_tail_of_lm_optimization(oracle, small_case, corridor_case, which, it):
    a, b = _lm_both_ways(oracle, small_case if which == "street" else corridor_case, it)
    assert np.array_equal(_bits(a[0]), _bits(b[0])), "pose"
    assert np.array_equal(_bits(a[1]), _bits(b[1])), "matP"
    assert a[2:] == b[2:], "is_degenerate, converged"
    if which == "corridor" and it == 0:
        assert a[2] == 1, "the corridor case is degenerate"


def test_lm_step_batch_is_a_loop_over_lm_step(oracle):
    b = G.gn_class("corridor", 64, oracle)[0]
    cfg = oracle.default_config()
    pose, matP, deg, conv = oracle.lm_step_batch(cfg, b.it, b.AtA32().reshape(-1, 36), b.AtB32(), b.pose, b.matP, b.deg)
    for i in range(len(b)):
        p1, m1, d1, c1 = oracle.lm_step(cfg, int(b.it[i]), b.AtA32()[i], b.AtB32()[i], b.pose[i], b.matP[i], int(b.deg[i]))
        assert np.array_equal(_bits(p1), _bits(pose[i])) and np.array_equal(_bits(m1.reshape(36)), _bits(matP[i])) and (d1, c1) == (deg[i], conv[i])


def test_corner_fit_is_the_tail_of_corner_optimization(oracle, synth):
    case = synth.add_corners(synth.make_case("vlp16", n_keyframes=8, seed=9, device="cpu", n_queries=4), "vlp16", seed=9)
    cfg = oracle.default_config(knn_mode=1, n_threads=4)
    total = 0
    for q in case["queries"][:2]:
        pose = np.array(q["pose_init"], np.float32)
        corners = np.ascontiguousarray(np.asarray(q["corners"], np.float32).reshape(-1, 3))
        cmap = np.ascontiguousarray(np.asarray(case["corner_map"], np.float32).reshape(-1, 3))
        flag, coeff, nn = oracle.corner_optimization(cfg, pose, corners, cmap)
        gated = np.flatnonzero(nn[:, 0] >= 0)
        T = np.ascontiguousarray(oracle.get_transformation(pose[3], pose[4], pose[5], pose[0], pose[1], pose[2]).reshape(12))
        sel = np.zeros((len(gated), 3), np.float32)
        for r, i in enumerate(gated):
            oracle.lib.lo_point_associate(T, corners[i], sel[r])
        f2, c2 = oracle.corner_fit_batch(cfg, cmap[nn[gated]], sel)
        assert np.array_equal(f2, flag[gated]) and np.array_equal(_bits(c2), _bits(coeff[gated]))
        f1, c1 = oracle.corner_fit(cfg, cmap[nn[gated[0]]], sel[0])
        assert f1 == flag[gated[0]] and np.array_equal(_bits(c1), _bits(coeff[gated[0]]))
        assert not flag[nn[:, 0] < 0].any() and not coeff[nn[:, 0] < 0].any()
        total += int(flag.sum())
    assert total > 100


def test_transform_of_equals_get_transformation(oracle):
    rng = np.random.default_rng(5)
    pose = np.concatenate([rng.uniform(-3.2, 3.2, (N_CPU, 3)), rng.uniform(-300, 300, (N_CPU, 3))], 1).astype(np.float32)
    T, trig = G.transform_of(pose)
    want = np.stack([oracle.get_transformation(p[3], p[4], p[5], p[0], p[1], p[2], 0).reshape(12) for p in pose])
    assert np.array_equal(_bits(T), _bits(want))
    assert np.array_equal(_bits(trig[:, 2]), _bits(-want[:, 8]))                         # sin(pitch) = -T[2][0]


# ------------------------------------------------------------------------------------------------ 6x6: finiteness and coverage
@pytest.fixture(scope="module")
def gn_cpu(oracle):
    """Every 6x6 class at the CPU size with its oracle results, built once."""
    out = {}
    for name in G.GN_CLASSES:
        dropped = []
        bs = G.gn_class(name, N_CPU, oracle, dropped)
        out[name] = (bs, [G.oracle_step(oracle, b) for b in bs], dropped)
    return out


@pytest.mark.parametrize("name", list(G.GN_CLASSES))
def test_every_6x6_case_is_finite_in_the_oracle(gn_cpu, name):
    bs, res, dropped = gn_cpu[name]
    assert sum(len(b) for b in bs) == N_CPU
    for b, o in zip(bs, res):
        assert np.isfinite(b.sums).all() and np.isfinite(b.sums.astype(np.float32)).all() and np.isfinite(b.pose).all()
        for k in ("pose", "matP"):
            assert np.isfinite(o[k]).all(), f"{b.tag}: non-finite {k}"
        T, trig = G.transform_of(o["pose"][:64])
        assert np.isfinite(T).all() and np.isfinite(trig).all()
    # what finite_only had to drop while building the class: nothing, or a few per cent; qr_singular by design about a quarter
    gen = N_CPU + max(32, int(N_CPU * G.SURPLUS.get(name, 0.125)))
    print(f"{name}: dropped {dropped} of {gen} generated")
    assert sum(dropped) <= (0.35 if name == "qr_singular" else 0.01) * gen
    if name in ("scene", "all_degenerate", "diagonal", "pivot_ties", "eps_offdiag", "convergence_edge"):
        assert sum(dropped) == 0


def _cleared(oracle, A):
    """Per matrix: how many eigenvalues the rule MO:1794-1805 clears (from the smallest up, while below the threshold)."""
    out = np.zeros(len(A), np.int64)
    ws = []
    for i, a in enumerate(A):
        w, _ = oracle.eigen6(a)
        ws.append(w)
        k = 0
        while k < 6 and w[5 - k] < G.EIG_THRESH:
            k += 1
        out[i] = k
    return out, np.stack(ws)


def test_corridor_clears_one_to_five_rows(oracle, gn_cpu):
    (b,), (o,), _ = gn_cpu["corridor"]
    k, _ = _cleared(oracle, b.AtA32())
    counts = np.bincount(k, minlength=7)
    print("corridor: cases per number of cleared rows", counts.tolist())
    assert (counts[1:6] >= N_CPU // 10).all() and counts[0] == 0 and counts[6] == 0
    assert (o["deg"] == 1).all()
    # a projector with k cleared rows has rank 6 - k
    rank = np.linalg.matrix_rank(o["matP"].reshape(-1, 6, 6).astype(np.float64), tol=1e-3)
    assert np.array_equal(rank, 6 - k)


def test_scene_has_both_outcomes_of_the_rule(gn_cpu):
    (b,), (o,), _ = gn_cpu["scene"]
    assert N_CPU // 10 < o["deg"].sum() < N_CPU - N_CPU // 10


def test_all_degenerate_is_a_zero_projector(gn_cpu):
    (b,), (o,), _ = gn_cpu["all_degenerate"]
    assert (o["deg"] == 1).all() and not o["matP"].any()
    assert np.array_equal(_bits(o["pose"]), _bits(b.pose)) and (o["conv"] == 1).all()       # the update is 0: converged at iteration 0


def test_diagonal_returns_its_own_values_with_ties(oracle, gn_cpu):
    (b,), (o,), _ = gn_cpu["diagonal"]
    A = b.AtA32()
    k, w = _cleared(oracle, A)
    d = A[:, np.arange(6), np.arange(6)]
    assert np.array_equal(_bits(w), _bits(-np.sort(-d, axis=1))), "no rotation: the eigenvalues are the diagonal, sorted"
    ties = (np.diff(np.sort(d, axis=1), axis=1) == 0).any(1)
    assert ties.sum() > N_CPU // 4
    on = (d == G.EIG_THRESH).any(1) & (d == G.pred(G.EIG_THRESH)).any(1)
    assert on.sum() > N_CPU // 20, "the threshold and its predecessor in one matrix: the strict < of the rule"
    # the row permutation the selection sort leaves: diag(100, 100, pred(100), 5, 100, succ(100)) -> rows 5, 1, 4, 0, 2, 3
    _, V = oracle.eigen6(A[0])
    assert np.array_equal(np.argmax(V, axis=1), [5, 1, 4, 0, 2, 3]) and np.array_equal(np.sort(V.reshape(-1))[-6:], np.ones(6, np.float32))
    # sorted descending, the eigenvalues below the threshold are the tail the rule clears: matP keeps exactly the unit vectors
    # of the entries that are not below it (strict <: the threshold itself is kept, its predecessor is not)
    want = np.zeros((N_CPU, 6, 6), np.float32)
    want[:, np.arange(6), np.arange(6)] = ~(d < G.EIG_THRESH)
    assert np.array_equal(k, (d < G.EIG_THRESH).sum(1))
    same = (want.reshape(N_CPU, 36) == o["matP"]).all(1)
    assert same.all(), f"{(~same).sum()} projectors are not the diagonal selection, first {np.flatnonzero(~same)[:5]}"
    assert np.array_equal(o["deg"], (k > 0).astype(np.int32))


def test_pivot_ties_start_tied(gn_cpu):
    (b,), _, _ = gn_cpu["pivot_ties"]
    A = np.abs(b.AtA32())
    off = A[:, G.IU[0], G.IU[1]][:, G.IU[0] != G.IU[1]]
    assert off.shape[1] == 15 and (off == np.round(off)).all()
    n_max = (off == off.max(1, keepdims=True)).sum(1)
    assert (n_max >= 2).mean() > 0.9 and (n_max == 15).sum() >= N_CPU // 4
    kind2 = np.arange(N_CPU) % 4 == 2                                                       # the maximum sits in the last column only
    last = A[:, :5, 5].max(1)
    inner = np.where(np.triu(np.ones((6, 6), bool), 1)[None] & (np.arange(6)[None, None, :] < 5), A, -1).max((1, 2))
    assert (last[kind2] > inner[kind2]).mean() > 0.8


def test_eps_offdiag_breaks_at_once_or_rotates_once(oracle, gn_cpu):
    (b,), _, _ = gn_cpu["eps_offdiag"]
    A = b.AtA32()
    off = np.abs(A[:, G.IU[0], G.IU[1]][:, G.IU[0] != G.IU[1]])
    at_once = (off <= G.EPS).all(1)
    one = (off > G.EPS).sum(1) == 1
    assert at_once.sum() >= N_CPU // 3 and one.sum() >= N_CPU // 3 and (off.max(1) <= G.succ(G.succ(G.EPS))).all()
    d = A[:, np.arange(6), np.arange(6)]
    moved = 0
    for i in range(N_CPU):
        w, V = oracle.eigen6(A[i])
        unrotated = np.array_equal(_bits(w), _bits(-np.sort(-d[i])))
        if at_once[i]:
            assert unrotated and np.array_equal(np.sort(np.abs(V).reshape(-1))[-6:], np.ones(6, np.float32))
        moved += not np.array_equal(np.abs(V), (np.abs(V) == 1).astype(np.float32))
    assert moved >= N_CPU // 3, "cases with an off-diagonal above eps rotate"


def test_qr_singular_has_both_outcomes(oracle, gn_cpu):
    (b,), (o,), _ = gn_cpu["qr_singular"]
    A, B = b.AtA32(), b.AtB32()
    ok = np.array([oracle.solve6(A[i], B[i])[1] for i in range(N_CPU)])
    X = np.stack([oracle.solve6(A[i], B[i])[0] for i in range(N_CPU)])
    rank = np.linalg.matrix_rank(A.astype(np.float64))
    print(f"qr_singular: singular by the 10 eps test {int((ok == 0).sum())}, solved {int((ok == 1).sum())}, largest |X| {np.abs(X).max():.3g}")
    assert (rank < 6).all(), "rank-deficient"
    assert (ok == 0).sum() > N_CPU // 5 and not X[ok == 0].any()
    assert (ok == 1).sum() > N_CPU // 5 and (np.abs(X[ok == 1]).max(1) > 1.0).sum() > N_CPU // 50 and np.isfinite(X).all()


def test_a_zero_column_is_not_finite_in_the_oracle(oracle):
    """Why qr_singular holds no zero matrix and no zeroed row-and-column pair: the reflector of an all-zero column is
    normalised by sqrt(0), and cv::solve returns NaN rather than calling the system singular.  Recorded, not judged."""
    x, ok = oracle.solve6(np.zeros((6, 6), np.float32), np.ones(6, np.float32))
    assert ok == 1 and np.isnan(x).all()
    A = np.diag(np.array([300, 200, 0, 500, 150, 120], np.float32))
    x, ok = oracle.solve6(A, np.ones(6, np.float32))
    assert ok == 1 and np.isnan(x).all()


def test_convergence_edge_sits_on_both_thresholds(gn_cpu):
    bs, res, _ = gn_cpu["convergence_edge"]
    assert [b.cfg["force_all_iters"] for b in bs] == [0, 1]
    for b, o in zip(bs, res):
        n = len(b)
        X = (b.AtB32() / b.AtA32()[:, np.arange(6), np.arange(6)]).astype(np.float32)    # AtB / d, exact
        s = o["solve"]
        assert np.array_equal(_bits((b.pose + X)[s]), _bits(o["pose"][s])), "the QR returned AtB / d bit for bit"
        r = (X[:, :3] * F(57.29578)).astype(np.float64)
        t = (X[:, 3:] * F(100)).astype(np.float64)
        dR = np.sqrt((r * r).sum(1)).astype(np.float32).astype(np.float64)
        dT = np.sqrt((t * t).sum(1)).astype(np.float32).astype(np.float64)
        for d in (dR, dT):
            assert (d < 0.05).sum() >= n // 4 and (d >= 0.05).sum() >= n // 4
            assert np.abs(d - 0.05).max() < 8 * 2.0 ** -28        # +-4 ulps of X, times at most 1.5625 ulps of 0.05 per ulp of X, plus one rounding
            assert (d == float(np.nextafter(F(0.05), F(0)))).any() or (d == float(F(0.05))).any()
        assert np.array_equal(o["conv"][s] == 1, ((dR < 0.05) & (dT < 0.05))[s])
        nc = b.nc()
        assert (nc == G.MIN_CORR - 1).sum() > n // 10 and (nc == G.MIN_CORR).sum() > n // 10
        assert (b.it == G.MAX_ITERS - 1).sum() > n // 10 and (b.it == 0).sum() > n // 10
        assert not o["deg"].any()


def test_later_iteration_projects_and_leaves_alone(oracle, gn_cpu):
    (b,), (o,), _ = gn_cpu["later_iteration"]
    assert (b.it > 0).all() and 0 < b.deg.sum() < len(b)
    assert np.array_equal(_bits(o["matP"]), _bits(b.matP)) and np.array_equal(o["deg"], b.deg)
    X = np.stack([oracle.solve6(b.AtA32()[i], b.AtB32()[i])[0] for i in range(len(b))])
    plain = np.array_equal(_bits((b.pose + X)[b.deg == 0]), _bits(o["pose"][b.deg == 0]))
    assert plain, "is_degenerate 0: the update is the solve's"
    proj = (_bits(b.pose + X) != _bits(o["pose"])).any(1)[b.deg == 1]
    assert proj.mean() > 0.9, "is_degenerate 1: the stored projector changes the update"


def test_scaled_reaches_both_ends(gn_cpu):
    bs, res, _ = gn_cpu["scaled"]
    small = [o for b, o in zip(bs, res) if "2^-30" in b.tag]
    big = [(b, o) for b, o in zip(bs, res) if "2^20" in b.tag]
    assert len(small) == 2 and len(big) == 2
    for o in small:
        assert (o["deg"] == 1).all() and not o["matP"].any()
    assert max(b.AtA32().max() for b, _ in big) > 1e11


def test_speculation_slices(gn_cpu):
    bs, res, _ = gn_cpu["speculation"]
    tags = [b.tag for b in bs]
    assert len(tags) == 6 and sum(b.skip_eigen for b in bs) == 3 and sum(b.hold_if_done for b in bs) == 2
    for b, o in zip(bs, res):
        if b.skip_eigen or (b.it > 0).all():
            assert np.array_equal(_bits(o["matP"]), _bits(b.matP)) and np.array_equal(o["deg"], b.deg), b.tag
        assert 0 < b.deg.sum() < len(b), "stored flags of both kinds"
        if b.hold_if_done:
            ends = (o["conv"] == 1) | (b.it + 1 >= G.MAX_ITERS) | ~o["solve"]
            assert len(b) // 10 < ends.sum() < len(b) - len(b) // 10, (b.tag, int(ends.sum()))


# ------------------------------------------------------------------------------------------------ five points and a point
@pytest.fixture(scope="module")
def corner_cpu(oracle):
    cfg = oracle.default_config()
    out = {}
    for name in G.CORNER_CLASSES:
        sets, pts, note = G.corner_class(name, N_CPU)
        flag, coeff = oracle.corner_fit_batch(cfg, sets, pts)
        nan = np.isnan(coeff).any(1)
        out[name] = dict(sets=sets, pts=pts, note=note, flag=flag, coeff=coeff, nan=nan, line=nan | (coeff != 0).any(1))
    return out


def test_edge_like_and_blob(corner_cpu):
    e, b = corner_cpu["edge_like"], corner_cpu["blob"]
    assert e["line"].mean() > 0.9 and 0.5 < e["flag"].mean() < 0.95
    assert np.abs(e["sets"]).max() > 400 and np.linalg.norm(e["pts"] - e["sets"].mean(1), axis=1).max() < 2.5
    assert 0.3 < b["line"].mean() < 0.8, "anisotropy on both sides of e0 = 3 e1"


def test_threshold_lattice_lands_above_below_and_on(corner_cpu):
    c = corner_cpu["threshold_lattice"]
    k = c["note"]["k"].astype(np.float32)
    e0 = (F(18) * k * k / F(2 ** 14)) / F(5)                                                # every operation before the division is exact
    e1 = (F(6) * k * k / F(2 ** 14)) / F(5)
    assert np.array_equal(c["line"], e0 > F(3) * e1), "the oracle's line test is e0 > 3 e1 on the float32 covariance"
    sweep = slice(0, 399)
    assert np.array_equal(c["note"]["k"][sweep], np.arange(1, 400))
    above, equal = int(c["line"][sweep].sum()), int((e0 == F(3) * e1)[sweep].sum())
    print(f"threshold_lattice, k = 1 .. 399: {above} above, {399 - above} not above, {equal} exactly equal")
    assert (above, 399 - above, equal) == (114, 285, 166)
    assert c["flag"].sum() > 0 and (c["flag"] == 0).sum() > 0


def test_rank_deficient_and_ties(corner_cpu):
    r = corner_cpu["rank_deficient"]
    kind = np.arange(N_CPU) % 5
    assert not r["line"][kind == 2].any() and not r["line"][kind == 4].any(), "a single point has no axis: 0 > 3 * 0 fails"
    assert r["line"][kind <= 1].mean() > 0.9 and r["line"][kind == 3].mean() > 0.9
    t = corner_cpu["pivot_ties3"]["sets"]
    d = t - G.centroid_f32(t)[:, None]
    a01, a02, a12 = (d[:, :, 0] * d[:, :, 1]).sum(1), (d[:, :, 0] * d[:, :, 2]).sum(1), (d[:, :, 1] * d[:, :, 2]).sum(1)
    tied = (np.abs(a01) == np.abs(a02)) & (np.abs(a02) == np.abs(a12))
    assert tied.mean() > 0.95 and (tied & (a01 != 0)).mean() > 0.8


def test_scales(corner_cpu):
    s12, s60, s40 = corner_cpu["scaled_2^-12"], corner_cpu["scaled_2^-60"], corner_cpu["scaled_2^+40"]
    # 2^-12: covariance entries at or below FLT_EPSILON, no rotation, the axis is a coordinate axis
    d = s12["sets"] - G.centroid_f32(s12["sets"])[:, None]
    cov = np.abs(np.einsum("nja,njb->nab", d, d) / 5)
    assert (cov[:N_CPU // 2, [0, 0, 1], [1, 2, 2]].max(1) <= G.EPS).all(), "the edge-like half: no off-diagonal above FLT_EPSILON"
    assert s60["line"].any() and s40["nan"].mean() > 0.5


def test_on_the_line_is_accepted_with_nan_coefficients(corner_cpu):
    c = corner_cpu["on_the_line"]
    kind = c["note"]["kind"]
    for k in (0, 1):                                                                       # the point at the centroid; on the axis
        m = kind == k
        both = (c["flag"] == 1) & np.isnan(c["coeff"][:, :3]).all(1) & (c["coeff"][:, 3] == 0)   # s (0 / 0) three times, then s * ld2 = 1 * 0
        print(f"on_the_line kind {k}: {int(both[m].sum())} of {int(m.sum())} accepted with NaN coefficients")
        assert both[m].mean() > 0.9
    m = kind == 2                                                                          # accept_edge
    assert c["line"][m].all() and not c["nan"][m].any()
    acc = c["flag"][m].mean()
    print(f"accept_edge: {acc:.3f} accepted")
    assert 0.25 < acc < 0.75
    ld2 = np.abs(c["coeff"][m, 3].astype(np.float64)) / np.maximum(np.linalg.norm(c["coeff"][m, :3].astype(np.float64), axis=1), 1e-30)
    assert np.abs(ld2 - 1.0).max() < 1e-5, "the distance is within a few ulps of (1 - min_s) / weight = 1"
