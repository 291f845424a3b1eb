"""The tracked frame reading map points resident on the device (capi.MapStore), from pixels: dvm_track_finish_batch_resident
(Tracker / TrackerBatch.track_resident) against the uploaded first half, and dvm_track_local_map_batch_resident against the uploaded second
half -- bit for bit, map-point ids translated through the slot table.  The scenes are those of test_gpu_track_frame.py and
test_gpu_track_local_map_batch.py."""
import numpy as np
import pytest

import pixel_scene as ps
from test_gpu_track_frame import BOUNDS, _check, _map_from_frame, _tcw7f
from test_gpu_track_local_map import _mps, _scene_table

pytestmark = pytest.mark.gpu


def _r64(n):
    return (n + 63) // 64 * 64


def _records(capi, mps):
    """MAP_POINT_DTYPE or LOCAL_POINT_DTYPE -> store records"""
    if mps.dtype == capi.LOCAL_POINT_DTYPE:
        return mps.copy()
    r = np.zeros(len(mps), capi.LOCAL_POINT_DTYPE)
    r["pos"], r["desc"], r["n_obs"] = mps["pos"], mps["desc"], mps["n_obs"]
    r["normal"][:, 2] = 1.0; r["min_dist"] = 0.1; r["max_dist"] = 100.0
    return r


class Slots:
    """A store holding `mps` at shuffled slots: slot_of[id] is where map point id lives."""

    def __init__(self, capi, mps, rng, extra=29, store=None, base=0):
        n = len(mps)
        self.capi, self.n = capi, n
        if store is None:
            self.store = capi.MapStore(n + extra)
            self.slot_of = rng.permutation(n + extra)[:n].astype(np.int32)
        else:                                   # a second agent in the same store: its points behind the first one's
            self.store = store
            self.slot_of = (base + rng.permutation(n)).astype(np.int32)
        if n:
            self.store.update(self.slot_of, _records(capi, mps))

    def to_slots(self, ids):
        ids = np.asarray(ids, np.int32)
        return np.where(ids >= 0, self.slot_of[np.maximum(ids, 0)], -1).astype(np.int32)


def _as_slots(r, S):
    return dict(r, mp=S.to_slots(r["mp"]), dropped=S.to_slots(r["dropped"]))


@pytest.fixture(scope="module")
def scene():
    return ps.render(12)


@pytest.mark.parametrize("p_obs0,th,p_drop", [(0.0, 15.0, 0.1), (0.3, 15.0, 0.1), (0.0, 2.0, 0.1), (0.0, 15.0, 0.995)])
def test_single_frames_equal_uploaded_call(scene, p_obs0, th, p_drop):
    """Three consecutive frames; th = 2: the wider attempt runs; p_drop = 0.995: fewer than 20 matches even then (tracked == 0)."""
    from dvm_slam_amd import capi
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    trk = capi.Tracker(ext)
    rng = np.random.default_rng(3)
    n0, k0, d0, _ = ext.extract(frames[0])
    mps = _map_from_frame(capi, k0, d0, *poses[0], rng, p_obs0=p_obs0)
    kps_l, mp_l = k0, np.arange(n0, dtype=np.int32)
    mp_l[rng.random(n0) < p_drop] = -1
    outl_l = (rng.random(n0) < 0.05).astype(np.uint8)         # some LastFrame outliers: their entries are not sent
    S = Slots(capi, mps, rng)
    wide = tracked = 0
    for t in (1, 2, 3):
        Tcw_pred = _tcw7f(ps.pose7(*poses[t - 1]))
        if th == 2.0:
            # a prediction 0.096 m off along the camera's x axis: every projection lands some 8 px off (500 x 0.096 / 6), beyond th = 2 at
            # every level (2 x 1.2^7 = 7.2 px) and within th = 4 from level 4 up (4 x 1.2^4 = 8.3 px): the first attempt finds fewer than 20
            Tcw_pred[4] += np.float32(0.096)
        up = trk.track(frames[t], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, kps_l, mp_l, outl_l, mps, th=th)
        up = dict(up, kps=up["kps"].copy(), desc=up["desc"].copy())
        up_bytes = trk.last_upload_bytes()[0]
        res = trk.track_resident(frames[t], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, kps_l, S.to_slots(mp_l), outl_l, S.store, th=th)
        _check(res, _as_slots(up, S), exact_pose=True)
        for k in ("nmatches_map", "n_requeried", "mono_index"):
            assert res[k] == up[k], k
        assert np.array_equal(res["kps_un"]["x"], up["kps_un"]["x"]) and np.array_equal(res["Tcw"], up["Tcw"])
        # upload bytes, from the record sizes: 9 B per entry sent, at most 16 B per entry (rounded up to 64) plus 1 KB per frame
        n_ent = int(((mp_l >= 0) & (outl_l == 0)).sum())
        got = trk.last_upload_bytes()[0]
        assert 0 < got <= 16 * _r64(n_ent) + 1024, (got, n_ent)
        assert up_bytes > got                                     # the uploaded call carries the 69-byte queries
        wide += res["wide_window"]; tracked += res["tracked"]
    if th == 2.0:
        assert wide >= 1
    if p_drop > 0.9:
        assert tracked == 0
    elif th == 15.0:
        assert tracked == 3
    S.store.close(); trk.close(); ext.close()


def test_batch_of_six_equals_single_uploaded_calls():
    """Six agents (different streams, maps and entry counts; one below 20 matches), each with its own store, two sharing one."""
    from dvm_slam_amd import capi, synth
    B = 6
    ext1 = capi.OrbExtractor(max_batch=1)
    extB = capi.OrbExtractor(max_batch=B)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    trk1 = capi.Tracker(ext1)
    trkB = capi.TrackerBatch(extB, B)
    dense = synth.frame_stream(8)
    low = synth.frame_stream(4, texture="low")
    rng = np.random.default_rng(21)
    Kc = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
    imgs, Ts, lasts, maps = [], [], [], []
    for b in range(B):
        stream, t = (low, 1 + b % 3) if b == 2 else (dense, 1 + b)
        n0, k0, d0, _ = ext1.extract(stream[t - 1])
        z = rng.uniform(3, 9, n0).astype(np.float32)
        mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
        mps["pos"][:, 0] = (k0["x"] - Kc[2]) / Kc[0] * z; mps["pos"][:, 1] = (k0["y"] - Kc[3]) / Kc[1] * z; mps["pos"][:, 2] = z
        mps["desc"] = d0; mps["n_obs"] = np.where(rng.random(n0) < 0.2, 0, 1)
        mp_l = np.arange(n0, dtype=np.int32)
        mp_l[rng.random(n0) < (0.992 if b == 4 else 0.1 * b)] = -1
        imgs.append(stream[t]); Ts.append(np.array([0, 0, 0, 1, 0.002 * b, 0, 0], np.float32)); lasts.append((k0.copy(), mp_l, None, mps))
    # agents 0 and 1 share one store (agent 1's points behind agent 0's), the others have their own
    shared = capi.MapStore(len(lasts[0][3]) + len(lasts[1][3]))
    for b in range(B):
        mps = lasts[b][3]
        if b == 0:
            maps.append(Slots(capi, mps, rng, store=shared, base=0))
        elif b == 1:
            maps.append(Slots(capi, mps, rng, store=shared, base=len(lasts[0][3])))
        else:
            maps.append(Slots(capi, mps, rng))
    ins, keep = trkB.prepare_resident(Ts, [(k0, maps[b].to_slots(ml), ol, maps[b].store) for b, (k0, ml, ol, _) in enumerate(lasts)])
    got = trkB.track_resident(np.stack(imgs), ins, Kc, BOUNDS, scale, inv_s2, th=15.0)
    n_ent = [int((l[1] >= 0).sum()) for l in lasts]
    assert 0 < trkB.last_upload_bytes()[0] <= sum(16 * _r64(n) + 1024 for n in n_ent)
    wide = 0
    for b in range(B):
        k0, mp_l, _, mps = lasts[b]
        one = trk1.track(imgs[b], Ts[b], Kc, BOUNDS, scale, inv_s2, k0, mp_l, None, mps, th=15.0)
        _check(got[b], _as_slots(one, maps[b]), exact_pose=True)
        assert got[b]["n_requeried"] == one["n_requeried"] and got[b]["nmatches_map"] == one["nmatches_map"]
        wide += got[b]["wide_window"]
    assert wide >= 1 and got[4]["tracked"] == 0
    for m in maps[1:]:
        m.store.close()
    trkB.close(); trk1.close(); extB.close(); ext1.close()


def test_the_store_is_what_is_read(scene):
    """Between two ticks thirty map points move by 5 cm and ten flip n_obs, through dvm_map_store_update only: the resident tick equals the
    uploaded tick on the changed records and differs from its own previous result."""
    from dvm_slam_amd import capi
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    trk = capi.Tracker(ext)
    rng = np.random.default_rng(5)
    n0, k0, d0, _ = ext.extract(frames[0])
    mps = _map_from_frame(capi, k0, d0, *poses[0], rng)
    mp_l = np.arange(n0, dtype=np.int32)
    S = Slots(capi, mps, rng)
    Tcw_pred = _tcw7f(ps.pose7(*poses[0]))
    before = trk.track_resident(frames[1], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, k0, S.to_slots(mp_l), None, S.store)
    before = dict(before, mp=before["mp"].copy(), pose=before["pose"].copy())
    assert before["tracked"]
    matched = np.unique(before["mp"][before["mp"] >= 0])
    ids = np.flatnonzero(np.isin(S.slot_of, matched))[:30]                 # map points the tick did use
    assert len(ids) == 30
    mps2 = mps.copy()
    mps2["pos"][ids] += np.float32(0.05)
    mps2["n_obs"][ids[:10]] = np.where(mps2["n_obs"][ids[:10]] > 0, 0, 1)
    S.store.update(S.slot_of[ids], _records(capi, mps2[ids]))
    after = trk.track_resident(frames[1], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, k0, S.to_slots(mp_l), None, S.store)
    up = trk.track(frames[1], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, k0, mp_l, None, mps2)
    _check(after, _as_slots(up, S), exact_pose=True)
    assert after["nmatches_map"] == up["nmatches_map"]
    assert not np.array_equal(after["pose"], before["pose"]) and after["nmatches_map"] != before["nmatches_map"]
    S.store.close(); trk.close(); ext.close()


def _same_second_half(a, b):
    for k in ("status", "n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers"):
        assert a[k] == b[k], (k, a[k], b[k])
    if a["status"] != 0:
        return
    assert np.array_equal(a["mp"], b["mp"]) and np.array_equal(a["outlier"], b["outlier"])
    assert a["track_pts"].tobytes() == b["track_pts"].tobytes()
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["Tcw"].tobytes() == b["Tcw"].tobytes()


def test_second_half_equals_uploaded_batch(scene):
    """Tables of 0, 1, 64, 65 and about 3 000 entries (bad entries among them) and a frame the first half did not complete, after a
    resident finish and after an uploaded one: mp_out, outlier, track_pts, every result field and the pose bytes equal
    dvm_track_local_map_batch."""
    from dvm_slam_amd import capi
    frames, poses = scene
    B = 6
    ext1 = capi.OrbExtractor(max_batch=1)
    extB = capi.OrbExtractor(max_batch=B)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(17)
    pts, (k0, n0) = _scene_table(capi, ext1, frames, poses, scale, rng)
    assert 2500 < len(pts) < 4000 and pts["bad"].any() and (pts["n_obs"] == 0).any()
    sizes = [0, 1, 64, 65, len(pts), len(pts)]
    mps = _mps(capi, pts)
    S = Slots(capi, pts, rng)                                    # the whole record: pos, normal, distances, desc, n_obs, bad
    mp_ls = [np.arange(n0, dtype=np.int32) for _ in range(B)]
    mp_ls[5] = mp_ls[5].copy(); mp_ls[5][rng.random(n0) < 0.998] = -1        # frame 5: fewer than 20 matches, not completed
    Ts = [_tcw7f(ps.pose7(*poses[0]))] * B
    imgs = np.stack([frames[1]] * B)
    trkB = capi.TrackerBatch(extB, B)
    trkB.reserve_local_map(sum(_r64(n) for n in sizes))
    K = ps.K.astype(np.float32)
    ths = [1.0, 5.0, 1.0, 15.0, 1.0, 1.0]

    def first(resident):
        if resident:
            ins, keep = trkB.prepare_resident(Ts, [(k0, S.to_slots(mp_ls[b]), None, S.store) for b in range(B)])
            r = trkB.track_resident(imgs, ins, K, BOUNDS, scale, inv_s2, th=15.0)
            return [_ids(S, x["mp"]) for x in r], r
        ins, keep = trkB.prepare(Ts, [(k0, mp_ls[b], None, mps) for b in range(B)])
        r = trkB.track(imgs, ins, K, BOUNDS, scale, inv_s2, th=15.0)
        return [x["mp"].copy() for x in r], r

    def fms_of(mp_ids):      # the frame's points as table positions; a point beyond a truncated table is not held
        return [np.where(m < sizes[b], m, -1).astype(np.int32) for b, m in enumerate(mp_ids)]

    mp_ids, r = first(resident=False)
    assert [x["tracked"] for x in r] == [1, 1, 1, 1, 1, 0]
    fms = fms_of(mp_ids)
    ref = trkB.track_local_map([pts[:n] for n in sizes], fms, th=ths, want_track_points=True)
    up_bytes = trkB.last_upload_bytes()[1]
    assert [x["status"] for x in ref] == [0, 0, 0, 0, 0, 1] and ref[4]["nmatches"] > 0
    ref = [dict(x, **{k: x[k].copy() for k in ("mp", "outlier", "track_pts") if k in x}) for x in ref]
    live = sum(_r64(n) for n in sizes[:5])
    for resident_first in (True, False):
        mp_ids2, _ = first(resident=resident_first)
        assert all(np.array_equal(a, b) for a, b in zip(mp_ids, mp_ids2))
        got = trkB.track_local_map_resident([S.store] * B, [S.slot_of[:n] for n in sizes], fms, th=ths, want_track_points=True)
        for b in range(B):
            _same_second_half(got[b], ref[b])
        # upload bytes, from the record sizes: 4 B per table entry (each frame's rounded up to 64) + 4 B per keypoint of capacity + 1 KB per frame
        sec = trkB.last_upload_bytes()[1]
        assert 0 < sec <= 4 * live + 4 * extB.cap * B + 1024 * B, sec
        assert up_bytes >= 72 * sum(sizes[:5]) and up_bytes > sec
    # a slot never written is refused before anything runs, and the finish stays valid for a corrected call
    first(resident=True)
    bad = [S.slot_of[:n].copy() for n in sizes]
    unwritten = np.setdiff1d(np.arange(S.store.capacity), S.slot_of)
    bad[4][7] = unwritten[0]
    with pytest.raises(capi.DvmError) as e:
        trkB.track_local_map_resident([S.store] * B, bad, fms, th=ths)
    assert e.value.code == -1
    got = trkB.track_local_map_resident([S.store] * B, [S.slot_of[:n] for n in sizes], fms, th=ths, want_track_points=True)
    _same_second_half(got[4], ref[4])
    S.store.close(); trkB.close(); extB.close(); ext1.close()


def _ids(S, slots):
    """store slots -> map-point ids (the inverse of Slots.to_slots)"""
    inv = np.full(S.store.capacity, -1, np.int32)
    inv[S.slot_of] = np.arange(S.n, dtype=np.int32)
    slots = np.asarray(slots, np.int32)
    return np.where(slots >= 0, inv[np.maximum(slots, 0)], -1).astype(np.int32)
