"""CPU: the scenes of tests/sim3_scene.py hold what tests/test_gpu_sim3.py needs them to hold, and the oracle (sim3_hypotheses,
optimize_sim3) is pinned on them against float64: Horn through numpy.linalg.eigh, CheckInliers with each camera's own intrinsics and
bounds, the degenerate rows, and what OptimizeSim3 returns on every case the device test runs.  The bounds are 4 x the largest deviation
measured here, oracle against float64 only (sim3_scene.ORACLE_*; docs/NOTEBOOK.md section 14 lists the cases)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sim3_scene as ss  # noqa: E402

N, H = 70, 200
I13 = np.r_[1.0, np.eye(3).ravel(), 0.0, 0.0, 0.0].astype(np.float32)


def _grid_case(oracle, angle, scale, fix):
    sc, gt = ss.scene(0, N, angle, scale)
    tri = ss.triples(0, N, H)
    return sc, gt, tri, oracle.sim3_hypotheses(triples=tri, fix_scale=fix, **sc)


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("angle,scale", ss.GRID)
def test_oracle_against_horn_f64(oracle, angle, scale, fix):
    """s, R, t of every hypothesis whose eigen-gap is above 1e-3 against float64; at most 5 % of a case's hypotheses fall below the gap."""
    sc, gt, tri, (T, nin, mask) = _grid_case(oracle, angle, scale, fix)
    assert np.isfinite(T).all()
    dR, ds, dt, gap = ss.deviations(T, sc, tri, fix)
    ok = gap > ss.GAP_MIN
    print(f"angle {angle:.6f} scale {scale} fix {int(fix)}: dR {dR[ok].max():.3e} ds {ds[ok].max():.3e} dt {dt[ok].max():.3e} below gap {(~ok).sum()}/{H}")
    assert (~ok).mean() <= ss.GAP_SHARE_MAX
    assert dR[ok].max() <= ss.BOUND_DR and ds[ok].max() <= ss.BOUND_DS and dt[ok].max() <= ss.BOUND_DT
    assert np.array_equal(nin, mask.sum(axis=1))
    if fix:
        assert np.all(T[:, 0] == 1.0)
    # the hypotheses of three good points find the similarity (those are most of them: 10 % outliers)
    good = ~gt["bad"][tri].any(axis=1)
    assert good.mean() > 0.6
    if not fix:
        assert np.median(np.abs(T[good, 0] / gt["s"] - 1)) < 0.02 and nin.max() > 0.6 * (~gt["bad"]).sum()


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("angle,scale", ss.GRID)
def test_oracle_masks_against_inliers_f64(oracle, angle, scale, fix):
    """The oracle's float decisions equal the float64 ones on every pair whose errors lie more than 1 % from their bounds; at most 2 % of a
    case's pairs lie inside the band."""
    sc, gt, tri, (T, nin, mask) = _grid_case(oracle, angle, scale, fix)
    ref, clear = ss.decide(*ss.inliers_f64(T, sc), sc)
    print(f"angle {angle:.6f} scale {scale} fix {int(fix)}: in band {(~clear).mean():.4f} inlier share {ref.mean():.3f}")
    assert (~clear).mean() <= ss.BAND_SHARE_MAX
    assert np.array_equal(mask.astype(bool)[clear], ref[clear])


@pytest.mark.parametrize("angle,scale", ss.GRID)
def test_distinct_cameras_matter(oracle, angle, scale):
    """A solver that took K1 for K2, or one camera's bounds for the other's, decides at least 5 % of the clear pairs differently."""
    sc, gt, tri, (T, nin, mask) = _grid_case(oracle, angle, scale, False)
    assert not np.array_equal(sc["K1"], sc["K2"]) and (sc["max_err1"] != sc["max_err2"]).mean() > 0.5
    ref, clear = ss.decide(*ss.inliers_f64(T, sc), sc)
    for knob in (ss.swap_K, ss.swap_err):
        sw = knob(sc)
        ref2, clear2 = ss.decide(*ss.inliers_f64(T, sw), sw)
        both = clear & clear2
        share = (ref != ref2)[both].mean()
        print(f"angle {angle:.6f} scale {scale} {knob.__name__}: {share:.3f}")
        assert share >= ss.SWAP_SHARE_MIN
        # and the oracle called that way follows the float64 decision of that call
        To, no, mo = oracle.sim3_hypotheses(triples=tri, fix_scale=False, **sw)
        assert np.array_equal(To, T) and np.array_equal(mo.astype(bool)[clear2], ref2[clear2])


def test_scene_contents():
    for angle, scale in ss.GRID:
        sc, gt = ss.scene(0, N, angle, scale)
        assert (sc["P1c"][:, 2] > 0).all() and (sc["P2c"][:, 2] > 0).all()
        assert 1 <= gt["bad"].sum() <= 0.25 * N
        # ground truth: the good points follow it to the noise
        fit = gt["s"] * (sc["P2c"].astype(np.float64) @ gt["R"].T) + gt["t"]
        assert np.abs(sc["P1c"] - fit)[~gt["bad"]].max() < 0.5 * scale
        assert np.isclose(np.trace(gt["R"]), 1 + 2 * np.cos(angle), atol=1e-12)
        with pytest.raises(ValueError):
            sc["P1c"][0, 0] = 0.0                                  # cached scenes are read-only
    same, _ = ss.scene(0, N, 0.3, 1.0, False)
    assert np.array_equal(same["K1"], same["K2"]) and np.array_equal(same["max_err1"], same["max_err2"])


def test_identity_rows(oracle):
    """P1c == P2c: q = (1, 0, 0, 0) exactly (vn == 0, the guarded division), R == I, s == 1, t == 0, every point an inlier."""
    for seed, n in ((0, 70), (1, 129)):
        sc = ss.identity(ss.scene(seed, n, 0.0, 1.0)[0])
        for fix in (False, True):
            T, nin, mask = oracle.sim3_hypotheses(triples=ss.triples(seed, n, H), fix_scale=fix, **sc)
            assert np.array_equal(T, np.broadcast_to(I13, T.shape)) and (nin == n).all() and mask.all()


def test_repeated_index_rows(oracle):
    """[i, i, i] with a centroid that is exact in float ((x + x + x) / 3 == x): every centred point is 0, den == 0: s and t NaN, R == I (all
    eigenvalues equal: the strict > keeps the first, q = (1, 0, 0, 0)), no inlier.  [i, i, j]: two distinct points, which Horn fits exactly
    (rank-1 M: R is one of a family), so i and j are inliers -- not an empty row."""
    sc, gt = ss.scene(0, N, 0.3, 1.0)
    ex = ss.exact_centroid(sc)
    assert len(ex) >= 5 and len(ex) < N                     # both kinds of point exist
    tri = np.array([[i, i, i] for i in ex], np.int32)
    T, nin, mask = oracle.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    assert np.isnan(T[:, 0]).all() and np.isnan(T[:, 10:]).all() and np.array_equal(T[:, 1:10], np.broadcast_to(I13[1:10], (len(ex), 9)))
    assert not mask.any() and not nin.any()
    j = [int(np.setdiff1d(np.flatnonzero(~gt["bad"]), [i])[k]) for k, i in enumerate(ex)]
    good_i = [k for k, i in enumerate(ex) if not gt["bad"][i]]
    tri2 = np.array([[i, i, jj] for i, jj in zip(ex, j)] + [[jj, i, i] for i, jj in zip(ex, j)], np.int32)
    T2, nin2, mask2 = oracle.sim3_hypotheses(triples=tri2, fix_scale=False, **sc)
    assert np.isfinite(T2).all()
    for k in good_i:
        assert mask2[k, ex[k]] and mask2[k, j[k]]


def test_depth_zero_point(oracle):
    """P2c[i, 2] == 0: its image in camera 2 is infinite or NaN, err2 < bound is false under every hypothesis; T and every other column stay."""
    sc, gt = ss.scene(0, N, 0.3, 1.0)
    tri = ss.triples(0, N, H)
    T0, n0, m0 = oracle.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    i = int(np.argmax(m0.sum(axis=0)))                         # the point most hypotheses accept
    assert m0[:, i].mean() > 0.3
    tri = tri[~(tri == i).any(axis=1)]
    T0, n0, m0 = oracle.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    T1, n1, m1 = oracle.sim3_hypotheses(triples=tri, fix_scale=False, **ss.depth0(sc, i))
    assert np.array_equal(T0, T1) and not m1[:, i].any()
    assert np.array_equal(np.delete(m0, i, axis=1), np.delete(m1, i, axis=1)) and np.array_equal(n1, n0 - m0[:, i])


@pytest.mark.parametrize("fix", [False, True])
def test_collinear_sets(oracle, fix):
    """Minimal sets within 1e-3 of a line: the two largest eigenvalues nearly coincide (R is one of a family), the residual is unique."""
    sc, gt, tri = ss.collinear_scene()
    P1t, P2t = sc["P1c"][tri], sc["P2c"][tri]
    s64, R64, t64, gap = ss.horn_f64(P1t, P2t, fix)
    assert gap.max() < 1e-4
    opt = ss.align_residual(P1t, P2t, s64, R64, t64)
    T, nin, mask = oracle.sim3_hypotheses(triples=tri, fix_scale=fix, **sc)
    assert np.isfinite(T).all()
    res = ss.align_residual(P1t, P2t, *ss.unpack(T))
    rel = np.abs(res - opt) / opt
    print(f"fix {int(fix)}: residual excess {rel.max():.3e}, optimum {opt.min():.3e} .. {opt.max():.3e}, |R - R64| up to {np.abs(ss.unpack(T)[1] - R64).max():.2f}")
    assert rel.max() <= ss.BOUND_COLLINEAR_RES
    assert np.abs(ss.unpack(T)[1] - R64).max() > 1e-3      # R itself is NOT comparable here


# ---- OptimizeSim3
@pytest.mark.parametrize("name", list(ss.OPT_CASES))
def test_optimize_sim3_cases(oracle, name):
    """What the oracle returns on each case of the device test, and that the case is what it is built to be: which pairs are gross on the
    input, how many survive round 1, which second round runs."""
    (S0, P1, P2, o1, o2, w1, w2, Ka, Kb), fix, th2, spec = ss.opt_case(name)
    kw = spec["kw"]
    n = len(P1)
    gross = np.zeros(n, bool); gross[list(kw.get("gross", ()))] = True
    assert not np.array_equal(Ka, Kb)
    S, inl, nin = oracle.optimize_sim3(S0, fix, P1, P2, o1, o2, w1, w2, Ka, Kb, th2)
    # on the input: at ANY similarity that fits the others, a gross pair's chi2 is far above th2 (80 px, weakest weight 0.078: > 700)
    if gross.any():
        assert kw.get("noise") == 0.0 and kw.get("out_frac") == 0.0
        c12, c21 = ss.chi2_f64(S if nin else S0, P1, P2, o1, o2, w1, w2, Ka, Kb)
        assert c12[gross].min() > 20 * th2
        assert n - gross.sum() == spec["survivors"]
    if spec["second_round"] == 0:
        assert nin == 0 and not inl.any() and np.array_equal(S, S0)
        return
    assert nin == inl.sum() and nin >= 10
    c12, c21 = ss.chi2_f64(S, P1, P2, o1, o2, w1, w2, Ka, Kb)
    assert (np.maximum(c12, c21)[inl > 0] <= th2 * (1 + 1e-9)).all()
    if spec["survivors"] is not None:
        assert nin == spec["survivors"] and np.array_equal(inl.astype(bool), ~gross)
    if kw.get("noise", 0.6) == 0.0:
        assert max(c12[inl > 0].max(), c21[inl > 0].max()) < 1e-3           # noise-free: the optimum is the truth
    if spec["second_round"] == 5:
        # optimize(5) runs only if round 1 removed nothing: every pair is alive at the end and passes
        assert inl.all()
    else:
        # optimize(10) runs if round 1 removed a pair.  A pair is removed when its chi2 exceeds th2 at the round-1 estimate; the pairs rejected
        # at the end exceed th2 by a factor > 3 at the optimum, and no estimate fits them and the accepted majority together
        rej = inl == 0
        assert rej.any() and np.maximum(c12, c21)[rej].min() > 3 * th2
    if fix:
        assert S[7] == S0[7] == 1.3
    else:
        assert S[7] != S0[7]
    assert np.abs(S - S0).max() > 1e-3                      # it optimised


def test_optimize_sim3_quaternion_sign(oracle):
    (S0, *rest), fix, th2, _ = ss.opt_case("n257")
    Sa, ia, na = oracle.optimize_sim3(S0, fix, *rest, th2)
    Sb, ib, nb = oracle.optimize_sim3(np.r_[-S0[:4], S0[4:]], fix, *rest, th2)
    assert na == nb and np.array_equal(ia, ib)
    assert np.abs(ss.quat_to_R(Sa[:4]) - ss.quat_to_R(Sb[:4])).max() < 1e-12 and np.abs(Sa[4:] - Sb[4:]).max() < 1e-12
