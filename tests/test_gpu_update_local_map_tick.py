"""A tick with UpdateLocalMap on the device, on the scene of tests/test_gpu_track_resident.py, one and three agents: rows set from a
keyframe graph over the scene's points; first half (track_resident) -> dvm_update_local_map_keyframes -> the covisibility expansion in
Python on the votes -> dvm_update_local_map_points -> the device's lists fed to track_local_map_resident.  The second half's outputs
equal, byte for byte, the run fed with the lists tests/local_map_scene.py builds on the host from the reference's loops."""
import numpy as np
import pytest

import keyframe_store_scene as kss
import local_map_scene as lms
import pixel_scene as ps
from test_gpu_track_frame import BOUNDS, _tcw7f
from test_gpu_track_local_map import _scene_table
from test_gpu_track_resident import Slots, _r64, _same_second_half

pytestmark = pytest.mark.gpu

N_KFS, SLOT_KEYPOINTS, KF_CAPACITY = 12, 1024, 16


class Agent:
    """One agent's map: the scene's point table at shuffled slots of its own MapStore, and N_KFS keyframes over it.  Every point sits in
    the row of one observing keyframe at least; keyframe 3 is queued (matches set, no observation yet)."""

    def __init__(self, capi, pts, seed):
        rng = np.random.default_rng(seed)
        self.capi = capi
        self.S = Slots(capi, pts, rng)
        self.points = [lms.MapPoint(int(s)) for s in self.S.slot_of]
        for p, bad in zip(self.points, pts["bad"]):
            p.bad = bool(bad)
        slots = np.sort(rng.permutation(KF_CAPACITY)[:N_KFS])
        self.kfs = [lms.KeyFrame(int(s), SLOT_KEYPOINTS - 7 * i) for i, s in enumerate(slots)]
        queued = self.kfs[3]
        home = rng.integers(0, N_KFS - 1, len(pts))
        home[home >= 3] += 1                                                         # (never the queued one)
        for t, kf in enumerate(self.kfs):
            mine = np.flatnonzero(home == t)
            extra = rng.permutation(len(pts))[:len(kf.matches) // 3]
            ids = np.concatenate([mine, extra])[:len(kf.matches)]
            assert len(mine) <= len(kf.matches)
            for kp, i in zip(rng.permutation(len(kf.matches))[:len(ids)], ids):
                kf.matches[int(kp)] = self.points[int(i)]
                if kf is not queued:
                    self.points[int(i)].add_observation(kf, int(kp))
        self.store = capi.KeyframeStore(KF_CAPACITY, SLOT_KEYPOINTS)
        self.store.put([kf.slot for kf in self.kfs], [kss.keyframe(200 + kf.slot, len(kf.matches)) for kf in self.kfs])
        sl = [kf.slot for kf in self.kfs]
        self.store.set_rows(capi.KFS_ROW_MATCHES, self.S.store, sl, [lms.row_matches(kf) for kf in self.kfs])
        self.store.set_rows(capi.KFS_ROW_OBSERVED, self.S.store, sl, [lms.row_observed(kf, self.points) for kf in self.kfs])
        self.by_slot = {kf.slot: kf for kf in self.kfs}
        self.point_at = {p.slot: p for p in self.points}

    def graph(self, frame_slots):
        frame = [None if s < 0 else self.point_at[int(s)] for s in frame_slots]
        return lms.Graph(self.kfs, self.points, frame, self.S.store.capacity, KF_CAPACITY, SLOT_KEYPOINTS)

    def expand(self, votes):
        """Tracking.cc:3183-3251 in miniature: the voted keyframes in slot order, then for each of them one neighbour not yet included
        (the next keyframe of the agent, cyclically); the call's kf_slot is that vector reversed."""
        local = [kf for kf in self.kfs if votes[kf.slot] > 0]
        for kf in list(local):
            nb = self.kfs[(self.kfs.index(kf) + 1) % N_KFS]
            if nb not in local:
                local.append(nb)
        return list(reversed(local))

    def close(self):
        self.store.close(); self.S.store.close()


@pytest.mark.parametrize("B", [1, 3])
def test_tick(capi, B):
    frames, poses = ps.render(12)
    ext1 = capi.OrbExtractor(max_batch=1)
    extB = capi.OrbExtractor(max_batch=B)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    pts, (k0, n0) = _scene_table(capi, ext1, frames, poses, scale, np.random.default_rng(17))
    agents = [Agent(capi, pts, 40 + b) for b in range(B)]
    trk = capi.TrackerBatch(extB, B)
    trk.reserve_local_map(B * _r64(len(pts)))
    ulm = capi.UpdateLocalMap()
    ulm.reserve(B, extB.cap, N_KFS, agents[0].S.store.capacity, KF_CAPACITY, SLOT_KEYPOINTS)
    K = ps.K.astype(np.float32)
    Ts = [_tcw7f(ps.pose7(*poses[0]))] * B
    imgs = np.stack([frames[1]] * B)
    mp_l = np.arange(n0, dtype=np.int32)

    def first_half():
        ins, keep = trk.prepare_resident(Ts, [(k0, a.S.to_slots(mp_l), None, a.S.store) for a in agents])
        r = trk.track_resident(imgs, ins, K, BOUNDS, scale, inv_s2, th=15.0)
        assert all(x["tracked"] for x in r)
        return [x["mp"].copy() for x in r]

    # the device's tick
    held = first_half()
    kf_res = ulm.keyframes([dict(kfs=a.store, points=a.S.store, mp_slot=m) for a, m in zip(agents, held)])
    orders = [a.expand(r["votes"]) for a, r in zip(agents, kf_res)]
    cleared = [np.where(r["frame_bad"] != 0, -1, m).astype(np.int32) for r, m in zip(kf_res, held)]
    pt_res = ulm.points([dict(kfs=a.store, points=a.S.store, kf_slot=[kf.slot for kf in o], mp_slot=m) for a, o, m in zip(agents, orders, cleared)])
    assert all(r["n_outside"] == 0 for r in pt_res) and all(r["n_local"] > 1000 for r in pt_res)
    got = trk.track_local_map_resident([a.S.store for a in agents], [r["local_slot"] for r in pt_res], [r["frame_mp"] for r in pt_res],
                                       th=1.0, want_track_points=True)
    got = [dict(x, **{k: x[k].copy() for k in ("mp", "outlier", "track_pts", "pose", "Tcw") if k in x}) for x in got]
    # the host's tick: the reference's loops on the graph
    held2 = first_half()
    lists = []
    for a, m, m2, r in zip(agents, held, held2, kf_res):
        assert np.array_equal(m, m2)
        g = a.graph(m)
        votes, frame_bad = lms.reference_keyframes(g)
        assert np.array_equal(r["votes"], votes) and np.array_equal(r["frame_bad"], frame_bad)
        assert votes[a.kfs[3].slot] == 0                                             # the queued keyframe gets no votes ...
        order = a.expand(votes)
        assert a.kfs[3] in order                                                     # ... and is walked as a neighbour
        lists.append(lms.reference_points(g, order))
    for r, (local, frame_mp, n_out) in zip(pt_res, lists):
        assert np.array_equal(r["local_slot"], local) and np.array_equal(r["frame_mp"], frame_mp) and n_out == 0
    ref = trk.track_local_map_resident([a.S.store for a in agents], [l[0] for l in lists], [l[1] for l in lists], th=1.0, want_track_points=True)
    for b in range(B):
        assert ref[b]["status"] == 0 and ref[b]["nmatches"] > 0
        _same_second_half(got[b], ref[b])
    ulm.close(); trk.close()
    for a in agents:
        a.close()
    extB.close(); ext1.close()
