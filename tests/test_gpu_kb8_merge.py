"""The inter-agent merge flow (dvm_slam_amd/merge.py: BoW query -> SearchByBoW -> Sim3Solver -> OptimizeSim3 -> SearchBySim3) between two
fisheye agents: steps 3 and 4 through dvm_sim3_hypotheses_cam / dvm_optimize_sim3_cam when `models` is given, the present calls when it is
not.  The scene is tests/sim3_cam_scene.two_agent_scene_kb8: merge_scene's two agents, both seeing through the robot's camera."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sim3_cam_scene as cs  # noqa: E402
from merge_scene import make_two_agent_scene  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _triples(seed, H=300):
    tr = np.random.default_rng(seed).integers(0, 1 << 30, (H, 3)).astype(np.int64)
    tr[:, 1] += (tr[:, 1] == tr[:, 0]); tr[:, 2] += 2 * ((tr[:, 2] == tr[:, 0]) | (tr[:, 2] == tr[:, 1]))
    return tr


def _recording_ops(merge, voc):
    class Ops(merge.GpuOps):
        """GpuOps that keeps the arguments of steps 3 and 4."""
        def sim3_hypotheses(self, *a):
            self.hyp_args = a
            return super().sim3_hypotheses(*a)

        def optimize_sim3(self, *a):
            self.opt_args = a
            return super().optimize_sim3(*a)

        def sim3_hypotheses_cam(self, *a):
            self.hyp_args = a
            return super().sim3_hypotheses_cam(*a)

        def optimize_sim3_cam(self, *a):
            self.opt_args = a
            return super().optimize_sim3_cam(*a)
    return Ops(voc)


def _run(merge, ops, sc, triples, models):
    peers = [dict(p) for p in sc["peers"]]
    db = merge.fill_database(ops, peers, levelsup=2)
    return merge.merge_with_peer(ops, sc["a"], sc["pa"], peers, sc["peer_pts"], db, 2, triples, models=models)


@pytest.mark.parametrize("seed", [0, 1])
def test_merge_between_two_fisheye_agents(capi, oracle, seed):
    from dvm_slam_amd import merge, synth
    voc = synth.vocabulary(k=10, L=4, seed=5)
    sc = cs.two_agent_scene_kb8(oracle, seed)
    assert 3 <= len(sc["peers"]) <= 8
    models = tuple(cs.camera_model(capi, m) for m in sc["models"])
    ops = _recording_ops(merge, voc)
    r = _run(merge, ops, sc, _triples(seed), models)
    # the true candidate among the distractors, enough correspondences, a hypothesis that most of them follow
    assert r["candidate"] == sc["true_idx"] and r["n_bow_matches"] > 100
    h = r["best_hyp"]
    assert 0.6 * r["n_bow_matches"] < r["hyp_inliers"][h] <= r["n_bow_matches"] and r["hyp_inliers"].min() < 0.5 * r["hyp_inliers"].max()
    # steps 3 and 4 are the _cam entries on the same correspondences, bit for bit
    P1c, P2c, e1, e2, m1, m2, tri = ops.hyp_args
    T, nin, mask = capi.sim3_hypotheses_cam(P1c, P2c, e1, e2, models[0], models[1], tri, False)
    assert np.array_equal(_bits(T), _bits(r["hyp_T"])) and np.array_equal(nin, r["hyp_inliers"])
    S12, P1, P2, o1, o2, w1, w2, m1, m2, th2 = ops.opt_args
    S, inl, n_in = capi.optimize_sim3_cam(S12, False, P1, P2, o1, o2, w1, w2, models[0], models[1], th2)
    assert np.array_equal(_bits(S), _bits(r["S12"])) and np.array_equal(inl, r["sim3_inliers"]) and n_in == r["n_sim3_inliers"] > 80
    # the count is the restatement's count at the returned S12 on the clear pairs
    c12, c21 = cs.chi2_cam_f64(S, P1, P2, o1, o2, w1, w2, sc["models"])
    clear = (np.abs(c12 - th2) > 1e-2 * th2) & (np.abs(c21 - th2) > 1e-2 * th2)
    ref = (c12 <= th2) & (c21 <= th2)
    assert clear.mean() > 0.95 and np.array_equal(inl.astype(bool)[clear], ref[clear]) and int(inl[clear].sum()) == int(ref[clear].sum())
    # ... and the restatement of OptimizeSim3 from the same start agrees: mask, count, S within the bound
    Sr, ir, nr = cs.optimize_sim3_f64(S12, False, P1, P2, o1, o2, w1, w2, sc["models"], th2)
    assert nr == n_in and np.array_equal(ir, inl) and np.abs(Sr - S).max() <= cs.S_BOUND
    # the ground truth is recovered through the fisheye cameras
    from scipy.spatial.transform import Rotation
    gt = sc["gt"]
    assert abs(S[7] / gt["s"] - 1) < 0.02 and np.linalg.norm(Rotation.from_quat(S[:4]).as_matrix() - gt["R"]) < 0.02
    assert np.linalg.norm(S[4:7] - gt["t"]) < 0.05 * max(1.0, np.linalg.norm(gt["t"]))
    # taken for pinhole cameras of the same fx, fy, cx, cy, the same correspondences give another answer
    pin = tuple(cs.camera_model(capi, cs.as_pinhole(m)) for m in sc["models"])
    S2, inl2, n2 = capi.optimize_sim3_cam(S12, False, P1, P2, o1, o2, w1, w2, pin[0], pin[1], th2)
    assert n2 < n_in or np.abs(S2 - S).max() > 10 * cs.S_BOUND


def test_pinhole_flow_is_unchanged(capi, oracle):
    """make_two_agent_scene with models=None and with two pinhole models: every output of the flow equal bit for bit, and steps 3 and 4 of
    the models=None flow are the pinhole entries on the same correspondences."""
    from dvm_slam_amd import merge, synth
    voc = synth.vocabulary(k=10, L=4, seed=5)
    sc = make_two_agent_scene(oracle, 0, n_distract=4)
    K = sc["a"]["K"]
    pin = (capi.CameraModel.pinhole(*K), capi.CameraModel.pinhole(*K))
    ops = _recording_ops(merge, voc)
    a = _run(merge, ops, sc, _triples(0), None)
    hyp_args, opt_args = ops.hyp_args, ops.opt_args
    b = _run(merge, ops, sc, _triples(0), pin)
    assert a["candidate"] == sc["true_idx"] and a["n_sim3_inliers"] > 80 and set(a) == set(b)
    for k in a:
        if k == "pairs":
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k
        else:
            assert a[k] == b[k], k
    T, nin, mask = capi.sim3_hypotheses(*hyp_args, False)
    assert np.array_equal(_bits(T), _bits(a["hyp_T"])) and np.array_equal(nin, a["hyp_inliers"])
    S, inl, n_in = capi.optimize_sim3(opt_args[0], False, *opt_args[1:])
    assert np.array_equal(_bits(S), _bits(a["S12"])) and np.array_equal(inl, a["sim3_inliers"]) and n_in == a["n_sim3_inliers"]
