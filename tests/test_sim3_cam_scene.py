"""tests/sim3_cam_scene.py on the CPU: the float64 restatement of OptimizeSim3 against the oracle on pinhole cameras, what the fisheye
scenes of the two Sim3 steps contain, and the measurements behind the constants the GPU tests (tests/test_gpu_sim3_cam.py) use."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sim3_cam_scene as cs  # noqa: E402
import sim3_scene as ss  # noqa: E402


# ---- 1. the restatement against the oracle
@pytest.mark.parametrize("name", list(ss.OPT_CASES))
def test_restatement_equals_oracle_on_pinhole_cameras(oracle, name):
    """optimize_sim3_f64 with two pinhole models on every case of sim3_scene.OPT_CASES: the oracle's mask and count, S within 1e-7 (a tenth
    of the device's gate against the oracle)."""
    (S0, P1, P2, o1, o2, w1, w2, Ka, Kb), fix, th2, spec = ss.opt_case(name)
    So, io, no = oracle.optimize_sim3(S0, fix, P1, P2, o1, o2, w1, w2, Ka, Kb, th2)
    S, inl, n = cs.optimize_sim3_f64(S0, fix, P1, P2, o1, o2, w1, w2, (cs.pinhole(Ka), cs.pinhole(Kb)), th2)
    assert n == no and np.array_equal(inl, io)
    d = float(np.abs(S - So).max())
    print(f"{name}: |S - S_oracle| {d:.3e}")
    assert d < cs.RESTATEMENT_GATE and cs.ORACLE_S_DIFF < cs.RESTATEMENT_GATE      # (the scene file's header records the largest d and its case)
    if spec["second_round"] == 0:
        assert n == 0 and np.array_equal(S, S0)


def test_nudge_is_a_no_op_on_pinhole_cameras():
    (S0, P1, P2, o1, o2, w1, w2, Ka, Kb), fix, th2, _ = ss.opt_case("n257")
    m = (cs.pinhole(Ka), cs.pinhole(Kb))
    a, b = (cs.optimize_sim3_f64(S0, fix, P1, P2, o1, o2, w1, w2, m, th2, nd) for nd in (0, 1))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_smooth_and_quantised_projection_differ_by_theta_rounding_only():
    """project_model's three modes on a fisheye camera agree to the float rounding of theta and psi (~1e-7 rad at r <= 500 px) up to
    theta = 1.8 rad."""
    rng = np.random.default_rng(5)
    X = rng.normal(0, 3, (500, 3))
    X = X[cs.theta(X) <= 1.8]
    for m in (cs.RM, cs.TM):
        ex, q, f = (cs.project_model(m, X, mode) for mode in ("exact", "f64", "f32"))
        assert np.abs(ex - q).max() < 2e-4 and np.abs(ex - f).max() < 2e-3
        up = cs.project_model(m, X, "f64", np.ones(len(X), np.int64))
        assert 0 < np.abs(up - q).max() < 2e-4


# ---- 2. what the fisheye hypothesis scenes contain
@pytest.mark.parametrize("pair", list(cs.PAIRS))
def test_hypothesis_scene_geometry(pair):
    for N in cs.HYP_N:
        sc, gt, tri, models = cs.hyp_case(pair, N)
        P1, P2 = sc["P1c"], sc["P2c"]
        assert P1.shape == P2.shape == (N, 3) and tri.shape == (cs.HYP_H, 3)
        assert cs.theta(P2).max() >= 1.2 and cs.theta(P1).max() >= 1.2
        if N < 63:
            continue
        assert P2[cs.AXIS, 0] == 0 and P2[cs.AXIS, 1] == 0 and P2[cs.AXIS, 2] > 0          # on the optical axis of camera 2
        assert P2[cs.Z0, 2] == 0                                                            # z == 0
        assert P2[cs.BEHIND, 2] < 0 and cs.theta(P2[cs.BEHIND])[0] > np.pi / 2              # z < 0 in its own camera
        assert (P1[:, 2] < 0).any()
        for k, X in enumerate((P1, P2)):                                                    # finite under KannalaBrandt8, everywhere
            if models[k][0] == cs.KB8:
                assert np.isfinite(cs.project_model(models[k], X, "f32")).all() and np.isfinite(cs.project_model(models[k], X)).all()


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("N", cs.HYP_N)
@pytest.mark.parametrize("pair", list(cs.PAIRS))
def test_hypothesis_scene_caps(pair, N, fix):
    """Under the restatement alone: few pairs inside BAND, few hypotheses under GAP_MIN; from 63 points on, between 20 % and 95 % of the
    clear pairs are inliers, and replacing either fisheye model by the pinhole model of its fx, fy, cx, cy changes at least 5 % of the
    decisions that are clear under both.  (N = 3: the three points are every minimal set; there is nothing to count.)"""
    sc, gt, tri, models = cs.hyp_case(pair, N)
    T, inl, clear, gap_ok = cs.hyp_reference(sc, tri, fix, models)
    assert (~clear).mean() <= ss.BAND_SHARE_MAX and (~gap_ok).mean() <= ss.GAP_SHARE_MAX
    if N < 63:
        return
    share = inl[clear].mean()
    print(f"inliers among the clear pairs: {share:.3f}")
    assert 0.20 <= share <= 0.95
    for k in (0, 1):
        if models[k][0] != cs.KB8:
            continue
        other = tuple(cs.as_pinhole(m) if j == k else m for j, m in enumerate(models))
        _, inl2, clear2, _ = cs.hyp_reference(sc, tri, fix, other)
        both = clear & clear2
        swap = (inl != inl2)[both].mean()
        print(f"camera {k + 1} as a pinhole camera: {swap:.3f} of the clear decisions change")
        assert swap >= ss.SWAP_SHARE_MIN


def test_special_points_are_decided_by_the_fisheye_model():
    """On the on-axis, z = 0 and z < 0 points of camera 2 the fisheye camera has clear decisions of both kinds over the hypotheses, where a
    pinhole camera has none to give (z = 0: not a number) or another (z < 0)."""
    sc, gt, tri, models = cs.hyp_case("rm_tum", 257)
    T, inl, clear, _ = cs.hyp_reference(sc, tri, False, models)
    for i in (cs.AXIS, cs.Z0, cs.BEHIND):
        assert clear[:, i].mean() > 0.9
    assert inl[:, [cs.AXIS, cs.Z0, cs.BEHIND]][clear[:, [cs.AXIS, cs.Z0, cs.BEHIND]]].any()
    _, inl2, clear2, _ = cs.hyp_reference(sc, tri, False, (models[0], cs.as_pinhole(models[1])))
    assert not inl2[:, cs.Z0].any()


# ---- 3. the fisheye OptimizeSim3 cases
def test_cases_mirror_the_pinhole_cases():
    assert set(ss.OPT_CASES) - {"n257_swapped"} <= set(cs.OPT_CASES_CAM) and {"n257_swapped", "n257_pin_tum", "n257_rm_pin"} <= set(cs.OPT_CASES_CAM)
    for name, spec in ss.OPT_CASES.items():
        c = cs.OPT_CASES_CAM[name]
        assert (c["th2"], c["survivors"], c["second_round"]) == (spec["th2"], spec["survivors"], spec["second_round"])
        assert c["kw"].get("N") == spec["kw"].get("N") and c["kw"].get("gross", ()) == spec["kw"].get("gross", ())
    assert cs.opt_case_cam("n257_swapped")[4] == (cs.TM, cs.RM)
    assert cs.opt_case_cam("n257_pin_tum")[4][0][0] == cs.PINHOLE and cs.opt_case_cam("n257_rm_pin")[4][1][0] == cs.PINHOLE


@pytest.mark.parametrize("name", list(cs.OPT_CASES_CAM))
def test_optimize_case(name):
    """What each case is built for: survivors, the second round's length, the early return; theta reaches 1.2 rad next to a fisheye camera."""
    (S0, P1, P2, o1, o2, w1, w2), fix, th2, spec, models = cs.opt_case_cam(name)
    S, inl, n = cs.opt_reference(name)
    if models[0][0] == cs.KB8 and models[1][0] == cs.KB8:
        assert cs.theta(P1).max() >= 1.2 and cs.theta(P2).max() >= 1.2
    if spec["second_round"] == 0:
        assert n == 0 and not inl.any() and np.array_equal(S, S0)
        # nine pairs pass round 1: the count at S0's neighbourhood is what the case was built for
        return
    assert n == inl.sum() >= 10
    if spec["survivors"] is not None:
        assert n == spec["survivors"]
    if fix:
        assert S[7] == 1.3
    c12, c21 = cs.chi2_cam_f64(S, P1, P2, o1, o2, w1, w2, models)
    assert np.array_equal(inl.astype(bool), inl.astype(bool) & (c12 <= th2) & (c21 <= th2))
    assert np.abs(S - S0).max() > 1e-3                       # the optimiser moved


def test_survivor_boundary():
    """9 / 10 / 11 pairs pass round 1 in the three survivor cases, built without noise: 9 returns early, 10 and 11 run the second round."""
    assert [cs.opt_reference(n)[2] for n in ("survive9", "survive10", "survive11")] == [0, 10, 11]
    (S0, P1, P2, o1, o2, w1, w2), fix, th2, spec, models = cs.opt_case_cam("survive9")
    S10 = cs.opt_reference("survive10")[0]
    c12, c21 = cs.chi2_cam_f64(S10, P1, P2, o1, o2, w1, w2, models)
    assert int(((c12 <= th2) & (c21 <= th2)).sum()) == 9


def test_stability_and_the_bound():
    """Every case returns the same mask and count with theta moved one float ulp either way (at most one named case may not, and none
    does); the largest |S(nudge) - S(0)| over them is the record the device's bound is ten times of."""
    unstable = [n for n in cs.OPT_CASES_CAM if not cs.is_stable(n)]
    assert unstable == ([] if cs.UNSTABLE_CASE is None else [cs.UNSTABLE_CASE])
    diffs = cs.theta_ulp_s_diff()
    for name, d in diffs.items():
        print(f"{name}: |S(nudge) - S(0)| {d:.3e}")
    worst = max(diffs, key=diffs.get)
    assert worst == cs.THETA_ULP_S_DIFF_CASE and 0.5 * cs.THETA_ULP_S_DIFF <= diffs[worst] <= 1.01 * cs.THETA_ULP_S_DIFF
    assert cs.S_BOUND == 10 * cs.THETA_ULP_S_DIFF


def test_model_matters_to_the_optimum():
    """Either fisheye camera taken as a pinhole camera moves the restatement's result far beyond the bound: a kernel that ignores a model fails."""
    (S0, *rest), fix, th2, spec, models = cs.opt_case_cam("n257")
    S = cs.opt_reference("n257")[0]
    for k in (0, 1):
        other = tuple(cs.as_pinhole(m) if j == k else m for j, m in enumerate(models))
        S2, inl2, n2 = cs.optimize_sim3_f64(S0, fix, *rest, other, th2)
        assert n2 != cs.opt_reference("n257")[2] or np.abs(S2 - S).max() > 10 * cs.S_BOUND
