"""CPU: the scenes of tests/pose_scene.py hold what tests/test_gpu_pose.py needs them to hold, and the oracle's PoseOptimization
(orc_pose_optimize) is pinned on every one of them against pose_f64, the numpy float64 restatement: identical flags and count, the pose
within 4 x the largest deviation measured here (pose_scene.ORACLE_*; docs/NOTEBOOK.md section 15 lists the cases).  Asserted per scene, on
pose_f64's counters: no classified chi2 within 1e-4 of 5.991, planted outliers beyond index 1 280, re-admitted edges on both sides of it,
rounds that end on a rejected trial, iterations of several trials, and that exchanging fx with fy (cx with cy) changes the flags."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_scene as ps  # noqa: E402

CASES = ps.all_cases()
_cache = {}


def _both(oracle, name, kw):
    """(scene, oracle result, pose_f64 result) of a named case, computed once."""
    if name not in _cache:
        sc = ps.scene(**kw)
        _cache[name] = (sc, oracle.pose_optimize(*ps.args(sc)), ps.pose_f64(*ps.args(sc)))
    return _cache[name]


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_oracle_against_pose_f64(oracle, name, kw):
    """Identical outlier mask and n_inliers; the pose within BOUND_DT / BOUND_DQ; no classified chi2 of any round within BAND_MIN of 5.991
    (the condition under which 'identical flags' is a fair demand of any correct implementation that is within 1e-6 in the pose)."""
    sc, (po, oo, no), (p64, o64, n64, info) = _both(oracle, name, kw)
    dt, dq = np.abs(po[:3] - p64[:3]).max(), np.abs(po[3:] - p64[3:]).max()
    print(f"{name}: dt {dt:.2e} dq {dq:.2e} min_band {info['min_band']:.2e} min_rho {info['min_rho']:.2e} tail outliers {int(sc['bad'][ps.REG:].sum())} "
          f"readmit {info['readmit_lo']}/{info['readmit_hi']} rejected_end {info['rejected_end']} empty {info['empty_rounds']} trials {info['trials']}")
    assert info["min_band"] >= ps.BAND_MIN
    assert np.array_equal(oo, o64) and no == n64 == len(oo) - int(oo.sum())
    assert dt <= ps.BOUND_DT and dq <= ps.BOUND_DQ
    assert abs(np.linalg.norm(po[3:]) - 1) < 1e-12 and po[6] >= 0
    assert info["failed_solves"] == 0


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_scene_contents(oracle, name, kw):
    """What a scene is built to be: points in front of the camera at mixed depths, outliers on both sides of index 1 280, a solvable
    problem (the planted outliers are found, the pose is recovered) unless every edge is an outlier."""
    sc, (po, oo, no), _ = _both(oracle, name, kw)
    N = len(sc["Xw"])
    Xc = sc["Xw"] @ ps.quat_to_R(sc["pose_gt"][3:]).T + sc["pose_gt"][:3]
    assert (Xc[:, 2] >= 4.0 - 1e-9).all() and (Xc[:, 2] <= 40.0 + 1e-9).all()
    assert (sc["w"] <= 1.0).all() and (sc["w"] >= 1.2 ** -14 - 1e-12).all()
    if N >= 64:
        assert Xc[:, 2].max() > 3 * Xc[:, 2].min() and len(np.unique(sc["w"])) == 8
    with pytest.raises(ValueError):
        sc["obs"][0, 0] = 0.0                                   # cached scenes are read-only
    if kw.get("all_out"):
        assert sc["bad"].all()
        return
    if kw.get("head_out"):
        assert sc["bad"][:ps.REG].all() and not sc["bad"][ps.REG:].any() and oo[:ps.REG].all() and no >= 0.9 * (N - ps.REG)
        return
    if N >= 1537:
        assert sc["bad"][ps.REG:].sum() >= ps.TAIL_OUTLIERS_MIN and sc["bad"][:ps.REG].sum() >= ps.TAIL_OUTLIERS_MIN
        assert oo[ps.REG:][sc["bad"][ps.REG:]].all()             # and every one of them is flagged at the end
    if N >= 63:
        assert oo[sc["bad"]].mean() >= 0.9 and np.abs(po - sc["pose_gt"]).max() < 0.05
    if N >= 255:
        signs = np.sign((sc["obs"] - ps.project(sc["K"], Xc))[sc["bad"]])
        assert len(np.unique(signs, axis=0)) == 4                # the gross outliers do not pull one way


def test_shares_on_the_reference_counters(oracle):
    """Re-admitted edges (flagged after one round, cleared after the next) on both sides of index 1 280 in the scenes named for it; rounds
    that end on a rejected trial and iterations of two or more trials below and above 1 280; rounds without an active edge."""
    for name, kw in ps.READMIT.items():
        info = _both(oracle, name, kw)[2][3]
        assert info["readmit_lo"] >= ps.READMIT_MIN and info["readmit_hi"] >= ps.READMIT_MIN, (name, info)
    for name, kw in ps.REJECTED.items():
        info = _both(oracle, name, kw)[2][3]
        assert info["rejected_end"] >= 1 and max(max(t) for t in info["trials"] if t) >= 2, (name, info)
    for name, kw in ps.ALL_OUT.items():
        info = _both(oracle, name, kw)[2][3]
        assert info["empty_rounds"] == 3 and info["rounds"] == 4 and info["trials"][1:] == [[], [], []]


@pytest.mark.parametrize("n", [300, 1537])
@pytest.mark.parametrize("knob", [ps.swap_f, ps.swap_c], ids=["fx<->fy", "cx<->cy"])
def test_camera_sensitivity(oracle, n, knob):
    """The default-camera scene called with fx and fy (cx and cy) exchanged: at least 30 % of the flags change, and the oracle called that
    way still agrees with pose_f64 called that way."""
    sc = ps.scene(**ps.CAMERAS[("default", n)])
    oo = oracle.pose_optimize(*ps.args(sc))[1]
    sw = knob(sc)
    po2, o2, n2 = oracle.pose_optimize(*ps.args(sw))
    share = (o2 != oo).mean()
    print(f"N {n} {knob.__name__}: {share:.3f} of the flags change")
    assert share >= ps.SWAP_SHARE_MIN
    p64, o64, n64, info = ps.pose_f64(*ps.args(sw))
    if info["min_band"] >= ps.BAND_MIN:
        assert np.array_equal(o2, o64) and n2 == n64


# ---- degenerate rows, pinned on the oracle
@pytest.mark.parametrize("name", list(ps.ALL_OUT))
def test_every_edge_an_outlier(oracle, name):
    """Every observation moved by +-80 px: round 1 flags every edge, rounds 2 to 4 have nothing to optimise: 0 inliers, all flags 1, the
    returned pose is the normalised input bit for bit."""
    sc, (po, oo, no), (p64, o64, n64, info) = _both(oracle, name, ps.ALL_OUT[name])
    assert no == 0 and oo.all() and np.array_equal(po, ps.normalize_pose(sc["pose0"]))
    assert np.array_equal(p64, po)
    # the same from a quaternion that is not normalised
    raw = np.r_[sc["pose0"][:3], -3.0 * sc["pose0"][3:]]
    po2, oo2, no2 = oracle.pose_optimize(raw, *ps.args(sc)[1:])
    assert no2 == 0 and oo2.all() and np.abs(po2 - po).max() < 1e-15 and abs(np.linalg.norm(po2[3:]) - 1) < 1e-15 and po2[6] >= 0


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 8, 9, 10, 11])
def test_round_count_at_ten_edges(oracle, n):
    """N = 3 .. 9: one round; N = 10 and 11: four (optimizer.edges().size() < 10)."""
    sc = ps.scene(seed=0, N=n)
    po, oo, no = oracle.pose_optimize(*ps.args(sc))
    p64, o64, n64, info = ps.pose_f64(*ps.args(sc))
    assert info["rounds"] == (1 if n < 10 else 4)
    assert info["min_band"] >= ps.BAND_MIN
    assert np.array_equal(oo, o64) and no == n64
    assert np.abs(po[:3] - p64[:3]).max() <= ps.BOUND_DT and np.abs(po[3:] - p64[3:]).max() <= ps.BOUND_DQ


def test_fewer_than_three(oracle):
    for n in (0, 1, 2):
        sc = ps.scene(seed=0, N=n)
        raw = np.r_[sc["pose0"][:3], 3.0 * sc["pose0"][3:]]
        p64, o64, n64, info = ps.pose_f64(raw, *ps.args(sc)[1:])
        assert n64 == 0 and not o64.any() and np.array_equal(p64, raw) and info["rounds"] == 0
        if n:
            po, oo, no = oracle.pose_optimize(raw, *ps.args(sc)[1:])
            assert no == 0 and not oo.any() and np.array_equal(po, raw)


@pytest.mark.parametrize("factor", [3.0, -1.0, -3.0])
def test_quaternion_scale_and_sign(oracle, factor):
    """The input quaternion scaled by 3, by -1 and by -3: normalised first (sign, then norm), so the flags are those of the normalised input
    and the pose agrees to the rounding of that normalisation, 1e-12; the output is of unit norm with w >= 0."""
    sc = ps.scene(**ps.CAMERAS[("default", 300)])
    assert sc["pose0"][6] > 0
    po, oo, no = oracle.pose_optimize(*ps.args(sc))
    raw = np.r_[sc["pose0"][:3], factor * sc["pose0"][3:]]
    po2, oo2, no2 = oracle.pose_optimize(raw, *ps.args(sc)[1:])
    print(f"factor {factor}: |pose - pose(normalised input)| {np.abs(po2 - po).max():.2e}")
    assert no2 == no and np.array_equal(oo2, oo) and np.abs(po2 - po).max() < 1e-12
    assert abs(np.linalg.norm(po2[3:]) - 1) < 1e-12 and po2[6] >= 0
    if factor == -1.0:
        assert np.array_equal(po2, po)                           # a sign costs no rounding


@pytest.mark.parametrize("point,kind", [((0.3, -0.2, 0.0), "inf"), ((0.0, 0.0, 0.0), "nan")])
def test_point_in_the_principal_plane(oracle, point, kind):
    """Identity pose, noise-free observations, one point with z == 0 exactly.  What the oracle does, pinned, and pose_f64 agrees:
    (0.3, -0.2, 0): the projection is infinite, chi2 = inf, H and b are NaN (0 x inf), every solve of round 1 fails; chi' = DBL_MAX is
       finite and inf - DBL_MAX = inf > 0, so each of the ten iterations 'accepts' its one trial without having moved; the edge is flagged
       (float(inf) > 5.991f), rounds 2 to 4 run without it on exact data (steps of 1e-17 on rounding residue): N - 1 inliers, the pose is
       the input to 1e-12.
    (0, 0, 0): 0 / 0, chi2 = NaN, the sums are NaN in every round, every solve fails, rho = NaN ends each iteration after one trial
       (NaN < 0 is false) and is neither 0 nor a tenth trial, so all ten iterations of all four rounds run; NaN > 5.991f is false: the edge is
       reported as an inlier, N inliers.
       The returned pose is the input bit for bit."""
    N = 40
    sc = ps.depth0_scene(0, N, point)
    po, oo, no = oracle.pose_optimize(*ps.args(sc))
    p64, o64, n64, info = ps.pose_f64(*ps.args(sc))
    print(f"{kind}: n_inliers {no} flags {oo.sum()} trials {info['trials']} failed {info['failed_solves']}")
    assert np.array_equal(oo, o64) and no == n64
    assert np.abs(po - sc["pose0"]).max() < 1e-12 and np.abs(p64 - sc["pose0"]).max() < 1e-12
    if kind == "inf":
        assert no == N - 1 and oo[N // 2] == 1 and oo.sum() == 1
        assert info["trials"][0] == [1] * 10 and info["failed_solves"] == 10
    else:
        assert no == N and not oo.any() and np.array_equal(po, sc["pose0"]) and np.array_equal(p64, sc["pose0"])
        assert info["trials"] == [[1] * 10] * 4 and info["failed_solves"] == 40


def test_classification_is_in_float(oracle):
    """An edge whose chi2 is 5.9910002 at the optimum: above 5.991 as a double, not above 5.991f as a float -- an inlier, as the reference's
    `const float chi2 = e->chi2(); if (chi2 > chi2Mono[it])` has it."""
    N = 40
    sc = ps.threshold_scene(0, N)
    po, oo, no = oracle.pose_optimize(*ps.args(sc))
    p64, o64, n64, info = ps.pose_f64(*ps.args(sc))
    c = ps.chi2_f64(po, *ps.args(sc)[1:])[0][N // 2]
    print(f"chi2 of the edge at the oracle's pose: {c:.10f}")
    assert 5.991 + 1e-7 < c < 5.991 + 3e-7 and np.float32(c) <= ps.CHI2_MONO
    assert no == n64 == N and not oo.any() and not o64.any()
    assert np.abs(po - sc["pose0"]).max() < 1e-7                # the edge's pull: 1e-12 x 2.4e6 px against 39 edges of weight 0.08 to 1
