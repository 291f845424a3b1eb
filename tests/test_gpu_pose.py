"""GPU parity of k_pose_optimize (Optimizer::PoseOptimization, one workgroup per frame) through dvm_pose_optimize and dvm_pose_pool_optimize
on the scenes of tests/pose_scene.py (fx != fy; tests/test_oracle_pose.py pins the scenes and the oracle on the CPU): on both sides of the
1 280 correspondences a workgroup keeps in registers (beyond them the flags and the last chi2 live in global memory), on the block and wave
tails, on both sides of the mapped / copied staging switch (S > 1280 or B S > 8192), inside ragged batches with garbage past n[f], and
on the degenerate rows.

Comparison rule: pose within 1e-6 of the oracle (POSE_TOL of test_gpu_ba.py), outlier flags and n_inliers identical (every scene keeps
every classified chi2 at least 1e-4 relative from 5.991, asserted on the CPU), output quaternion of unit norm to 1e-12 with w >= 0.  The
kernel sums in a fixed order: the same frame gives the same bits whatever the stride, the batch around it or the staging path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_scene as ps  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6
_orc = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _oracle(oracle, sc):
    """The oracle's (pose, outlier, n_inliers) of a scene, computed once per scene object."""
    key = id(sc)
    if key not in _orc:
        _orc[key] = (sc, oracle.pose_optimize(*ps.args(sc)))
    return _orc[key][1]


def _pack(frames, stride):
    """Batch arrays of dvm_pose_optimize for a list of scenes (None: an empty frame): rows past n[f] are NaN in Xw, obs and inv_sigma2."""
    B = len(frames)
    poses = np.zeros((B, 7)); Xw = np.full((B, stride, 3), np.nan); obs = np.full((B, stride, 2), np.nan); w = np.full((B, stride), np.nan)
    n = np.zeros(B, np.int32)
    for f, sc in enumerate(frames):
        k = len(sc["Xw"]); n[f] = k
        poses[f] = sc["pose0"]
        Xw[f, :k], obs[f, :k], w[f, :k] = sc["Xw"], sc["obs"], sc["w"]
    return poses, Xw, obs, w, n


def _device(capi, frames, stride):
    """[(pose, outlier[:n], n_inliers)] of one dvm_pose_optimize call over `frames` (all with the first frame's camera)."""
    poses, Xw, obs, w, n = _pack(frames, stride)
    pg, og, ng = capi.pose_optimize(poses, Xw, obs, w, n, frames[0]["K"])
    return [(pg[f], og[f, :n[f]], int(ng[f])) for f in range(len(frames))]


def _one(capi, sc, stride=None):
    return _device(capi, [sc], max(1, len(sc["Xw"])) if stride is None else stride)[0]


def _assert_parity(dev, orc, name=""):
    (pg, og, ng), (po, oo, no) = dev, orc
    d = np.abs(pg - po).max()
    print(f"{name}: |pose - oracle| {d:.3e}, {int(og.sum())} flagged of {len(og)}")
    assert ng == no and np.array_equal(og, oo) and ng == len(og) - int(og.sum())
    assert d < POSE_TOL
    assert abs(np.linalg.norm(pg[3:]) - 1) < 1e-12 and pg[6] >= 0


def _assert_same_bits(a, b):
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("n", list(ps.SIZES))
def test_sizes(capi, oracle, n):
    """One frame, stride = N, default camera, 10 % outliers at 35 px: N < 10 (one round), 10 and 11 (four), the wave and block tails, the
    last register-resident edge and the first in global memory (1 281: one tail edge, thread 0's; 1 537: every thread has one, thread 0
    two; 2 561: thread 0 alone runs the tail loop twice ... 8 192: the largest stride a chain launches with)."""
    sc = ps.scene(**ps.SIZES[n])
    assert len(sc["Xw"]) == n
    _assert_parity(_one(capi, sc), _oracle(oracle, sc), f"N {n}")


def test_stride_and_staging(capi, oracle):
    """The same frame (N = 1 000) at strides N, N + 1, 1 280, 1 281 and 8 192 and inside batches on both sides of B S <= 8192 (S = 1 280
    with B = 6: mapped, B = 7: copied; S = 1 281, B = 1: copied): bit-equal everywhere, equal to the oracle once."""
    sc = ps.scene(**ps.STAGING)
    N = len(sc["Xw"])
    base = _one(capi, sc)
    _assert_parity(base, _oracle(oracle, sc), "stride N")
    for stride in (N + 1, 1280, 1281, 8192):
        _assert_same_bits(_one(capi, sc, stride), base)
    other = ps.scene(seed=1, N=777)
    ref_other = _one(capi, other)
    for B in (6, 7):
        frames = [other if f % 2 else sc for f in range(B)]
        for f, out in enumerate(_device(capi, frames, 1280)):
            _assert_same_bits(out, ref_other if f % 2 else base)


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_batch_independence(capi, oracle, order):
    """One batch at stride 2 600 with n = [2561, 0, 2, 1281, 9, 1280, 300] (and the same frames in reverse order, so that every long
    frame sits once at f = 0 and once behind others), NaN past n[f]: every frame equals the oracle and its own single-frame call bit for
    bit; the n = 0 and n = 2 frames return 0 inliers and their input pose -- given with a quaternion of norm 3 -- as it came."""
    frames = []
    for kw in ps.BATCH:
        sc = ps.scene(**kw)
        if kw["N"] < 3:
            sc = ps.with_pose(sc, np.r_[sc["pose0"][:3], 3.0 * sc["pose0"][3:]])
        frames.append(sc)
    if order == "reversed":
        frames = frames[::-1]
    out = _device(capi, frames, ps.BATCH_STRIDE)
    for f, (sc, dev) in enumerate(zip(frames, out)):
        n = len(sc["Xw"])
        if n < 3:
            assert dev[2] == 0 and not dev[1].any() and np.array_equal(_bits(dev[0]), _bits(sc["pose0"])), f
        else:
            _assert_parity(dev, _oracle(oracle, sc), f"frame {f} n {n}")
        _assert_same_bits(dev, _one(capi, sc))


@pytest.mark.parametrize("name,n", list(ps.CAMERAS))
def test_cameras(capi, oracle, name, n):
    """(520, 390, 300, 250), (390, 520, 250, 300) and the suite's (149, 149, 320, 240) at N = 300 and 1 537: fx and fy, cx and cy each in
    their own row of the projection and of the Jacobian (exchanging them changes 54 to 92 % of the flags: test_oracle_pose)."""
    sc = ps.scene(**ps.CAMERAS[(name, n)])
    _assert_parity(_one(capi, sc), _oracle(oracle, sc), f"{name} N {n}")


@pytest.mark.parametrize("name", list(ps.READMIT) + list(ps.REJECTED))
def test_readmission_and_rejected_trials(capi, oracle, name):
    """Scenes in which edges flagged after one round pass again after the next, on both sides of index 1 280, and scenes whose rounds
    end on a rejected trial (the inliers then report the errors of the state that was thrown away) -- counted on the CPU."""
    sc = ps.scene(**{**ps.READMIT, **ps.REJECTED}[name])
    _assert_parity(_one(capi, sc), _oracle(oracle, sc), name)


@pytest.mark.parametrize("name", list(ps.ALL_OUT))
def test_every_edge_an_outlier(capi, oracle, name):
    """Every edge at +-80 px: rounds 2 to 4 have no active edge; 0 inliers, all flags 1, the normalised input pose bit for bit -- also from
    a quaternion of norm 3 and negative w."""
    sc = ps.scene(**ps.ALL_OUT[name])
    dev = _one(capi, sc)
    assert dev[2] == 0 and dev[1].all() and np.array_equal(_bits(dev[0]), _bits(ps.normalize_pose(sc["pose0"])))
    _assert_parity(dev, _oracle(oracle, sc), name)
    raw = ps.with_pose(sc, np.r_[sc["pose0"][:3], -3.0 * sc["pose0"][3:]])
    _assert_parity(_one(capi, raw), oracle.pose_optimize(*ps.args(raw)), name + " raw")


@pytest.mark.parametrize("name", list(ps.HEAD_OUT))
def test_only_tail_edges_active(capi, oracle, name):
    """Every register-resident edge (index < 1 280) is a gross outlier, the 720 behind them are good: from round 2 on the active count,
    the sums and the classification of the inliers come from the edges in global memory alone."""
    sc = ps.scene(**ps.HEAD_OUT[name])
    dev = _one(capi, sc)
    _assert_parity(dev, _oracle(oracle, sc), name)
    assert dev[1][:ps.REG].all() and dev[2] >= 0.9 * (len(sc["Xw"]) - ps.REG)


def test_degenerate(capi, oracle):
    """N = 3 .. 9 (one round) against 10 and 11 (four); the input quaternion scaled by 3, -1 and -3; a point with z == 0 exactly (infinite
    and NaN projections: what the oracle does is pinned in test_oracle_pose.test_point_in_the_principal_plane)."""
    for n in range(3, 12):
        sc = ps.scene(seed=0, N=n)
        _assert_parity(_one(capi, sc), _oracle(oracle, sc), f"N {n}")
    sc = ps.scene(**ps.CAMERAS[("default", 300)])
    base = _oracle(oracle, sc)
    for factor in (3.0, -1.0, -3.0):
        raw = ps.with_pose(sc, np.r_[sc["pose0"][:3], factor * sc["pose0"][3:]])
        dev = _one(capi, raw)
        _assert_parity(dev, oracle.pose_optimize(*ps.args(raw)), f"q x {factor}")
        assert np.array_equal(dev[1], base[1]) and np.abs(dev[0] - base[0]).max() < POSE_TOL
    N = 40
    for point, inliers in (((0.3, -0.2, 0.0), N - 1), ((0.0, 0.0, 0.0), N)):
        sc = ps.depth0_scene(0, N, point)
        dev = _one(capi, sc)
        _assert_parity(dev, oracle.pose_optimize(*ps.args(sc)), f"z == 0 at {point}")
        assert dev[2] == inliers and dev[1][N // 2] == (inliers == N - 1)
        if inliers == N:
            assert np.array_equal(_bits(dev[0]), _bits(sc["pose0"]))


def test_classification_is_in_float(capi, oracle):
    """chi2 = 5.9910002 at the optimum (pose_scene.threshold_scene): above 5.991 as a double, not above 5.991f as a float: an inlier."""
    N = 40
    sc = ps.threshold_scene(0, N)
    dev = _one(capi, sc)
    _assert_parity(dev, oracle.pose_optimize(*ps.args(sc)), "threshold")
    assert dev[2] == N and not dev[1].any()


def test_pool_boundary(capi, oracle):
    """PosePool.optimize at n = 1 280 (a lane's slot in mapped memory, stride 1 280) and n = 1 281 (handed to dvm_pose_optimize): both
    bit-equal to capi.pose_optimize of the same frame; n = 0: 0 inliers, the pose as given."""
    pool = capi.PosePool(max_batch=4)
    try:
        for n in (1280, 1281):
            sc = ps.scene(**ps.SIZES[n])
            pose, outl, nin, _ = pool.optimize(*ps.args(sc))
            _assert_same_bits((pose, outl, nin), _one(capi, sc))
            _assert_parity((pose, outl, nin), _oracle(oracle, sc), f"pool n {n}")
        raw = np.r_[0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 3.0]
        pose, outl, nin, _ = pool.optimize(raw, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0), ps.K_DEFAULT)
        assert nin == 0 and len(outl) == 0 and np.array_equal(_bits(pose), _bits(raw))
    finally:
        pool.close()


def test_repeatable(capi):
    """N = 2 561 twice in one process: every output byte equal (the tail's flags and chi2 are rewritten, not accumulated)."""
    sc = ps.scene(**ps.SIZES[2561])
    poses, Xw, obs, w, n = _pack([sc], 2561)
    a = capi.pose_optimize(poses, Xw, obs, w, n, sc["K"])
    b = capi.pose_optimize(poses, Xw, obs, w, n, sc["K"])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
