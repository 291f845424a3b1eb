"""SearchByBoWCovisibles (host/LoopClosing_shim.h), EXECUTED on mock keyframes and map points (tests/stubs/, tests/bow_shim_driver/): a
current keyframe and the covisible lists of three BoW candidates go through the shim's ONE device call, and everything it returns is
compared with LoopClosing.cc:708-747 restated here around oracle.search_by_bow_kf_kf.  Two worlds: candidates with 0, 4 and 10
covisibles; the same with one bad and one null covisible."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bow_targets_scene as bts
import shim_world as sw

pytestmark = pytest.mark.gpu

DRV_DIR = os.path.join(sw.ROOT, "tests", "bow_shim_driver")
CUR = 0                                        # the world's keyframe that plays mpCurrentKF; keyframe 1 + t is the scene's target t
SIZES = (1, 5, 11)                             # vpCovKFi of the three candidates: the candidate and its 0, 4, 10 covisibles
_lib = None


def _driver():
    global _lib
    if _lib is None:
        from dvm_slam_amd import capi
        capi.lib(); capi.host_lib()
        path = os.path.join(DRV_DIR, "libbowshimdriver.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", DRV_DIR], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(path)
        _lib.sw_create.restype = C.c_void_p
        _lib.sw_error.restype = C.c_char_p
    return _lib


class BowWorld(sw.World):
    def __init__(self):
        self.L = _driver()
        self.h = C.c_void_p(self.L.sw_create())
        self.kf, self.mp, self.maps, self.tables = [], [], [], sw.scale_tables()


def _world(bad_kfs=()):
    """(world, keyframe dicts with mp = the world's map point index and bad = that point's flag).  The keyframes share map points: the
    point of a 3-D point is one MapPoint in every keyframe that sees it, so spMatchedMPi's first-seen-wins rule has something to decide."""
    sc = bts.scene(3, sum(SIZES), n_pts=150, n_clutter=30, n_nodes=12)
    W = BowWorld()
    m = W.add_map(0)
    point = {}                                 # the scene's map point id -> world index
    kfs = []
    for k, kf in enumerate([sc["cur"]] + sc["targets"]):
        W.add_keyframe(m, 100 + k, np.array([0, 0, 0, 0, 0, 0, 1], np.float32), [500, 500, 320, 240], kf["kps"], kf["desc"], bad=k in bad_kfs)
        fv = kf["fv"]
        W.L.sw_kf_set_feature_vector(W.h, k, len(fv["fv_nodes"]), sw._p(fv["fv_nodes"]), sw._p(fv["fv_off"]), sw._p(fv["fv_feat"]))
        mp = np.full(len(kf["mp"]), -1, np.int32)
        for idx in np.nonzero(kf["mp"] >= 0)[0]:
            pid = int(kf["mp"][idx])
            if pid not in point:
                point[pid] = W.add_mappoint(m, pid, np.zeros(3, np.float32), desc=kf["desc"][idx], bad=pid % 9 == 0)
            W.observe(k, point[pid], int(idx))
            mp[idx] = point[pid]
        kfs.append(dict(kf, mp=mp, bad=np.array([i >= 0 and W.mp[i]["bad"] for i in mp], np.uint8)))
    return W, kfs


def _expected(oracle, W, kfs, lists, nnratio, check_ori):
    """LoopClosing.cc:708-747 for one vpCovKFi (world keyframe indices, -1 = null)."""
    cur = kfs[CUR]
    N = len(cur["desc"])
    rows, nums = [], []
    most, most_j = 0, 0
    for j, k in enumerate(lists):
        if k < 0 or W.kf[k]["bad"]:
            rows.append(None); nums.append(0)
            continue
        num, ids = bts.oracle_row(oracle, cur, kfs[k], nnratio, check_ori)
        rows.append(ids); nums.append(num)
        if num > most:
            most, most_j = num, j
    seen = set()
    mp = np.full(N, -1, np.int32); kf_of = np.full(N, -1, np.int32)
    for j, ids in enumerate(rows):
        if ids is None:
            continue
        for i in range(N):
            p = int(ids[i])
            if p < 0 or W.mp[p]["bad"] or p in seen:
                continue
            seen.add(p)
            mp[i] = p; kf_of[i] = lists[j]
    return rows, nums, (most, most_j, len(seen)), mp, kf_of


@pytest.mark.parametrize("defects", [False, True], ids=("plain", "bad_and_null"))
def test_shim_against_the_restated_loop(oracle, defects):
    bad_kf = 1 + SIZES[0] + 2                                     # a covisible of the second candidate
    W, kfs = _world(bad_kfs=(bad_kf,) if defects else ())
    flat = np.arange(1, 1 + sum(SIZES), dtype=np.int32)
    if defects:
        flat[SIZES[0] + SIZES[1] + 4] = -1                        # a null covisible of the third candidate
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    N, E, Cn = len(kfs[CUR]["desc"]), len(flat), len(SIZES)
    n_e = np.full(E, -7, np.int32); row_size = np.full(E, -7, np.int32)
    mp_rows = np.full((E, N), -7, np.int32); idx2_rows = np.full((E, N), -7, np.int32)
    summary = np.full((Cn, 3), -7, np.int32); matched_mp = np.full((Cn, N), -7, np.int32); matched_kf = np.full((Cn, N), -7, np.int32)
    W._chk(W.L.swb_search_covisibles(W.h, CUR, sw._p(flat), sw._p(off), Cn, C.c_float(0.9), 1, sw._p(n_e), sw._p(row_size), sw._p(mp_rows),
                                     sw._p(idx2_rows), sw._p(summary), sw._p(matched_mp), sw._p(matched_kf)))
    total = 0
    for c in range(Cn):
        lists = [int(k) for k in flat[off[c]:off[c + 1]]]
        rows, nums, summ, mp, kf_of = _expected(oracle, W, kfs, lists, 0.9, True)
        for j, k in enumerate(lists):
            e = off[c] + j
            assert n_e[e] == nums[j]
            if rows[j] is None:
                assert row_size[e] == 0 and np.all(mp_rows[e] == -1) and np.all(idx2_rows[e] == -1)      # an empty row (:723-724)
                continue
            assert row_size[e] == N and np.array_equal(mp_rows[e], rows[j])
            hit = idx2_rows[e] >= 0
            assert np.array_equal(hit, rows[j] >= 0) and np.array_equal(kfs[k]["mp"][idx2_rows[e][hit]], rows[j][hit])
        assert tuple(summary[c]) == summ
        assert np.array_equal(matched_mp[c], mp) and np.array_equal(matched_kf[c], kf_of)
        total += summ[2]
        if len(lists) > 1 and not defects:
            assert len(set(kf_of[kf_of >= 0])) > 1               # points first seen in a later covisible: the rule decided something
    assert total > 100
    W.close()
