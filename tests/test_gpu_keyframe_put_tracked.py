"""dvm_keyframe_store_put_tracked: Tracking::CreateNewKeyFrame on frames the tracker holds after a finish -- dvm_keyframe_store_put_device
on the frames' mvKeysUn and descriptors where the finish left them, behind the extractor's stream.  A promoted slot must equal
dvm_keyframe_store_put of the frame's downloaded kps_un / desc with the host transform's FeatureVector, field by field, and the chains
that read the store must return on it what they return on the put slot, bit for bit.  The world is
tests/test_gpu_track_reference_keyframe_batch.py's."""
import numpy as np
import pytest

import pixel_scene as ps
import test_gpu_track_reference_keyframe_batch as tb_
from test_gpu_keyframe_put_device import same_slots, same_vectors
from test_gpu_kb8_track_reference_keyframe import rig  # noqa: F401 (the KannalaBrandt8 agent's fixture)
from test_gpu_track_reference_keyframe_batch import scene, world  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS = 4096
STATE, INVALID = -6, -1
LEVELSUP = tb_.LEVELSUP


def tables(scale, inv_s2, K=ps.K, bounds=tb_.BOUNDS):
    scale = np.asarray(scale, np.float32)
    return dict(K=np.asarray(K, np.float32)[:4], bounds=np.asarray(bounds, np.float32), scale_factors=scale, level_sigma2=(scale ** 2).astype(np.float32),
                inv_level_sigma2=np.asarray(inv_s2, np.float32), log_scale_factor=float(np.log(scale[1])))


def put_host(capi, store, slot, voc, frame, tab, levelsup=LEVELSUP):
    """dvm_keyframe_store_put of a finish's downloaded frame; returns the host transform"""
    fv = capi.vocab_transform_host(voc, frame["desc"], levelsup)
    store.put([slot], [dict(tab, kps=frame["kps_un"], desc=frame["desc"], fv=fv)])
    return fv


def promoted_equals_put(capi, store, trk, ext, vocd, voc, frames_out, which, tab, levelsup=LEVELSUP):
    """frames `which` of the finish promoted to slots 1, 3, ...; each equals put (to slots 0, 2, ...) of the download"""
    dev = [2 * k + 1 for k in range(len(which))]
    got = store.put_tracked(trk, ext, vocd, which, dev, [tab] * len(which), levelsup=levelsup)
    assert store.last_put_bytes() < 1024 * len(which) + 4096            # the item records and the level tables, nothing per keypoint
    for k, b in enumerate(which):
        fv = put_host(capi, store, 2 * k, voc, frames_out[b], tab, levelsup)
        assert got[k]["n"] == frames_out[b]["n"] > 100
        same_vectors(got[k], fv)
        r, _ = same_slots(store, 2 * k, 2 * k + 1)
        assert np.array_equal(r["bounds"], tab["bounds"]) and np.array_equal(r["K"], tab["K"])
    return got


def _refused(capi, code, fn):
    with pytest.raises(capi.DvmError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_promotion_after_a_finish_and_the_chains_on_the_promoted_slots(scene, world, capi):  # noqa: F811
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    store = capi.KeyframeStore(8, SLOT_KEYPOINTS)
    tab = tables(w["scale"], w["inv_s2"])
    ts = [1, 2, 3, 4, 5]
    ext, tb = tb_._new_batch(capi, 5, local=5 * 16384)
    first = tb_._first_batch(tb, w, frames, poses, ts, ["ok"] * 5)
    which = [0, 2, 4]
    promoted_equals_put(capi, store, tb, ext, vocd, w["voc"], first, which, tab)
    # still accepted behind the second half and the reference-keyframe chain of the same finish
    kf = tb_._kf(capi, w, w["voc"])
    rk = tb.track_reference_keyframe(vocd, [kf] * 5, [tb_._tcw7f(ps.pose7(*poses[t - 1])) for t in ts], ps.K, w["inv_s2"])
    store.put_tracked(tb, ext, vocd, [1], [7], [tab])
    tb.track_local_map([w["pts"]] * 5, [(x if "mp" in x else f0)["mp"].astype(np.int32) for x, f0 in zip(rk, first)], th=1.0)
    store.put_tracked(tb, ext, vocd, [3], [6], [tab])
    put_host(capi, store, 7, w["voc"], first[3], tab)
    same_slots(store, 7, 6)
    # ---- downstream: host-put slots 0, 2, 4 against promoted slots 1, 3, 5
    host, dev = [0, 2, 4], [1, 3, 5]
    # Fuse
    pts = {k: np.ascontiguousarray(w["pts"][k][:300]) for k in ("pos", "normal", "min_dist", "max_dist", "desc")}
    tcw = [tb_._tcw7f(ps.pose7(*poses[ts[b]])) for b in which]
    ft = capi.FuseTargets()
    ft.reserve(300, 3, 0)
    rows = []
    for slots in (host, dev):
        ft.set_resident(store, slots, tcw)
        rows.append(ft.run(pts, 3.0))
    assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1]) and (rows[0][0] >= 0).sum() > 0
    ft.close()
    # SearchByBoW between keyframes
    m = capi.MapStore(len(w["pts"]))
    m.update(np.arange(len(w["pts"]), dtype=np.int32), w["pts"])
    mps = [(np.arange(first[b]["n"]) % len(w["pts"])).astype(np.int32) for b in which]
    bt = capi.BowTargets()
    bt.reserve(SLOT_KEYPOINTS, 2, 2 * SLOT_KEYPOINTS)
    rows = [[x.copy() for x in bt.search_resident(store, (s[0], m, mps[0]), [(s[1], m, mps[1]), (s[2], m, mps[2])])] for s in (host, dev)]
    assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1]) and rows[0][1].sum() > 0
    bt.close()
    # TrackReferenceKeyFrame on the promoted slots
    pose_last = [tb_._tcw7f(ps.pose7(*poses[t - 1])) for t in ts[:3]]
    out = []
    for slots in (host, dev):
        tb_._first_batch(tb, w, frames, poses, ts[:3], ["fail"] * 3)
        out.append(tb.track_reference_keyframe_resident(vocd, store, [(slots[k], m, mps[k]) for k in range(3)], pose_last, ps.K, w["inv_s2"]))
    for a, b in zip(*out):
        assert a["status"] == b["status"]
        tb_._same(a, b, [k for k in tb_.FORM_B_KEYS if k in a and k in b])
    assert max(r["nmatches"] for r in out[0]) >= 15
    tb.close(); ext.close(); store.close(); m.close(); vocd.close()


@pytest.mark.parametrize("distorted", [False, True])
def test_single_frame_tracker_and_form_a(scene, world, capi, distorted):  # noqa: F811
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    store = capi.KeyframeStore(4, SLOT_KEYPOINTS)
    dist, bounds = None, tb_.BOUNDS
    if distorted:
        cam = np.array([500.0, 500.0, 320.0, 240.0, -0.04, 0.01, 0.0005, -0.0003, 0.0], np.float32)
        dist = capi.Distortion(*[float(v) for v in cam])
        bounds = capi.image_bounds(cam, 640, 480)
    tab = tables(w["scale"], w["inv_s2"], bounds=bounds)
    A = tb_.Single(capi, w, local=len(w["pts"]))
    f = A.first(frames[3], tb_._pred(poses, 3, "fail"), tb_._last(w, "ok"), dist=dist, bounds=bounds)
    if distorted:
        assert not np.array_equal(f["kps_un"]["x"], f["kps"]["x"])
    promoted_equals_put(capi, store, A.trk, A.ext, vocd, w["voc"], [f], [0], tab)
    # the sequence of a frame whose motion model failed: the reference keyframe (form b), then the second half
    kf = tb_._kf(capi, w, w["voc"])
    rb = A.refkf(vocd, kf, tb_._tcw7f(ps.pose7(*poses[2])))
    assert rb["status"] == capi.DVM_TRACK_COMPLETE
    promoted_equals_put(capi, store, A.trk, A.ext, vocd, w["voc"], [f], [0], tab)
    A.trk.track_local_map(w["pts"], rb["mp"].astype(np.int32), th=1.0)
    promoted_equals_put(capi, store, A.trk, A.ext, vocd, w["voc"], [f], [0], tab)
    # form (a) of the reference-keyframe call: begin + chain, no finish
    r = A.trk.track_reference_keyframe(vocd, kf, tb_._tcw7f(ps.pose7(*poses[2])), img=frames[4], K=ps.K, bounds=bounds, inv_sigma2=w["inv_s2"], dist=dist)
    promoted_equals_put(capi, store, A.trk, A.ext, vocd, w["voc"], [r], [0], tab)
    A.close(); store.close(); vocd.close()


def test_kannala_brandt8_tracker(rig):  # noqa: F811
    import kb8_track_scene as kt
    capi, sc = rig["capi"], rig["sc"]
    store = capi.KeyframeStore(4, SLOT_KEYPOINTS)
    tab = tables(rig["scale"], rig["inv_s2"], K=kt.P[:4], bounds=kt.BOUNDS)
    ext = capi.OrbExtractor(max_batch=2)
    trk = capi.TrackerBatch(ext, 2)
    lasts = [(sc["kps_l"], sc["mp_l"], None, sc["mps"])] * 2
    ins, keep = trk.prepare([sc["Tcw_pred"], sc["Tcw_pred"]], lasts)
    got = trk.track(np.stack([sc["img_c"], sc["img_c"]]), ins, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], th=kt.TH, model=rig["model"])
    promoted_equals_put(capi, store, trk, ext, rig["vocd"], rig["w"]["voc"], got, [1], tab)
    trk.close(); ext.close(); store.close()


def test_refusals(scene, world, capi):  # noqa: F811
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    store = capi.KeyframeStore(4, SLOT_KEYPOINTS)
    tab = tables(w["scale"], w["inv_s2"])
    ext, tb = tb_._new_batch(capi, 2)
    other = capi.OrbExtractor(max_batch=2)

    def put(e=ext, frames_=(0,), slots=(0,)):
        return store.put_tracked(tb, e, vocd, list(frames_), list(slots), [tab] * len(slots))
    _refused(capi, STATE, put)                                     # before any finish
    first = tb_._first_batch(tb, w, frames, poses, [1, 2], ["ok", "ok"])
    _refused(capi, STATE, lambda: put(e=other))                    # another extractor
    _refused(capi, INVALID, lambda: put(frames_=(2,)))
    _refused(capi, INVALID, lambda: put(frames_=(-1,)))
    got = put(frames_=(1,))
    assert got[0]["n"] == first[1]["n"]
    # the next begin ends it, until the next finish
    imgs = np.ascontiguousarray(np.stack([frames[3], frames[4]]))
    capi.check(tb.L.dvm_track_begin_batch(tb.t, ext.h, imgs.ctypes.data, 2, imgs.shape[1], imgs.shape[2], imgs.strides[1], imgs.strides[0], 0, 1000))
    _refused(capi, STATE, put)
    _refused(capi, STATE, put)
    ext.sync()
    first = tb_._first_batch(tb, w, frames, poses, [3, 4], ["ok", "ok"])
    got = put(frames_=(0, 1), slots=(2, 3))
    assert [g["n"] for g in got] == [first[0]["n"], first[1]["n"]]
    tb.close(); ext.close(); other.close(); store.close(); vocd.close()
