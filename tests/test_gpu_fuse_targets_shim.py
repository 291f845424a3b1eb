"""SearchInNeighborsChain (host/LocalMapping_shim.h), EXECUTED on mock keyframes and map points (tests/stubs/, tests/fuse_shim_driver/): two
identical worlds -- a current keyframe, 6 target keyframes that share some of its map points, hold others of their own on the same 3-D
points, and have free keypoints -- of which world A runs the chain (one speculative device run per direction plus the refreshes of stale
rows) and world B the plain loop (one dvmh_fuse per target on the descriptors of that moment).  The mock MapPoint::Replace does not
recompute descriptors, so both worlds take the same stand-in: the survivor takes the replaced point's descriptor.  Both must leave the same
map: every keyframe's mvpMapPoints, every point's observations, bad flag, observation count and mpReplaced, and nFused per target."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fuse_targets_scene as fts
import shim_world as sw

pytestmark = pytest.mark.gpu

DRV_DIR = os.path.join(sw.ROOT, "tests", "fuse_shim_driver")
CURRENT = 3                                    # the scene's keyframe that plays mpCurrentKeyFrame; the other six are the targets
_lib = None


def _driver():
    global _lib
    if _lib is None:
        from dvm_slam_amd import capi
        capi.lib(); capi.host_lib()
        path = os.path.join(DRV_DIR, "libfuseshimdriver.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", DRV_DIR], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(path)
        _lib.sw_create.restype = C.c_void_p
        _lib.sw_error.restype = C.c_char_p
    return _lib


class FuseWorld(sw.World):
    def __init__(self):
        self.L = _driver()
        self.h = C.c_void_p(self.L.sw_create())
        self.kf, self.mp, self.maps, self.tables = [], [], [], sw.scale_tables()

    def run(self, chain, targets, seam):
        t = np.ascontiguousarray(targets, np.int32)
        fused = np.full(len(t) + 1, -7, np.int32)
        fn = self.L.swf_chain if chain else self.L.swf_loop
        calls = self._chk(fn(self.h, CURRENT, sw._p(t), len(t), int(seam), sw._p(fused)))
        return calls, fused


def _world():
    """The same world every time it is called (seeded)."""
    sc = fts.scene(4, 7)
    pts = sc["pts"]
    rng = np.random.default_rng(11)
    W = FuseWorld()
    m = W.add_map(0)
    for k, kf in enumerate(sc["targets"]):
        T = kf["Tcw"]
        W.add_keyframe(m, 100 + k, np.concatenate([T[4:7], T[0:4]]), kf["K"], kf["kps"], kf["desc"], bounds=(0, 0, 640, 480))

    def add_point(i, desc):
        return W.add_mappoint(m, 1000 + len(W.mp), pts["pos"][i], pts["normal"][i], float(pts["min_dist"][i]), float(pts["max_dist"][i]), desc)
    own = {}                                   # row of pts -> the current keyframe's map point on it
    pt_of_kp = sc["targets"][CURRENT]["pt_of_kp"]
    for idx in np.nonzero(pt_of_kp >= 0)[0]:
        i = int(pt_of_kp[idx])
        if i not in own and rng.random() < 0.85:
            own[i] = add_point(i, pts["desc"][i])
            W.observe(CURRENT, own[i], int(idx))
    shared = unshared = 0
    for k, kf in enumerate(sc["targets"]):
        if k == CURRENT:
            continue
        seen = set()
        for idx in np.nonzero(kf["pt_of_kp"] >= 0)[0]:
            i = int(kf["pt_of_kp"][idx])
            if i in seen:
                continue
            seen.add(i)
            r = rng.random()
            if r < 0.3 and i in own:
                W.observe(k, own[i], int(idx)); shared += 1          # the target already observes the current keyframe's point
            elif r < 0.7:
                W.observe(k, add_point(i, kf["desc"][idx]), int(idx)); unshared += 1   # a point of its own on the same 3-D point
    assert shared > 40 and unshared > 100
    for p in range(len(W.mp)):                 # observation counts on both sides of Fuse's `>` test
        W.L.sw_mp_set_obs_count(W.h, p, int(rng.integers(1, 7)))
    return W


def _state(W):
    return dict(matches=[W.kf_matches(k).tolist() for k in range(len(W.kf))],
                points=[(W.mp_observations(p), {k: W.get_mp(p)[k] for k in ("bad", "n_obs", "replaced")}) for p in range(len(W.mp))])


@pytest.mark.parametrize("seam", [True, False], ids=("descriptors_change", "descriptors_stay"))
def test_chain_leaves_the_map_of_the_plain_loop(seam):
    targets = [k for k in range(7) if k != CURRENT]
    A, B = _world(), _world()
    before = _state(A)
    assert before == _state(B)
    calls_a, fused_a = A.run(True, targets, seam)
    calls_b, fused_b = B.run(False, targets, seam)
    after = _state(A)
    assert after == _state(B)
    assert np.array_equal(fused_a, fused_b) and calls_b == 7
    # the scene exercises every branch of the apply step, in both directions
    replaced = [p for p, (_, s) in enumerate(after["points"]) if s["replaced"] >= 0]
    assert after != before and len(replaced) >= 20 and (fused_a[:6] > 0).sum() >= 4 and fused_a[6] > 0
    n_cur = sum(1 for k in before["matches"][CURRENT] if k >= 0)
    assert any(after["points"][p][1]["replaced"] < n_cur for p in replaced if p >= n_cur)      # a target's point gave way to the current keyframe's ...
    assert any(after["points"][p][1]["replaced"] >= n_cur for p in replaced if p < n_cur)      # ... and the other way round
    assert sum(1 for a, b in zip(after["matches"], before["matches"]) for x, y in zip(a, b) if y < 0 <= x) >= 10   # points added to free keypoints
    if seam:
        assert calls_a > 2, "the scene must make the stale path run"
    else:
        assert calls_a == 2                    # one device call per direction
    A.close(); B.close()


def test_candidates_are_marked_through_the_member_where_the_class_has_it():
    """LocalMapping.cc:840-842 on a point class with mnFuseCandidateForKF (the reference's MapPoint; the mock has none and gets a call-local set)."""
    out = np.full(8, -7, np.int32)
    _driver().swf_mark_candidate_with_member(sw._p(out))
    assert out.tolist() == [1, 0, 1, 1, 0, 8, 7, 0]
