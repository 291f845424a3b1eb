"""dvm_track_reference_keyframe_batch_resident: TrackReferenceKeyFrame on reference keyframes that live in a dvm_keyframe_store, their
map points in dvm_map_stores.  k_refkf_gather packs the chain's keyframe block on the device where the uploaded call packs it on the
host, and every kernel behind it is the uploaded call's, so each case compares with dvm_track_reference_keyframe_batch on the same
finish, output field by output field, bit for bit -- the uploaded call carrying mp = mp_slot and pos / n_obs / bad read from the
records.  The world is tests/test_gpu_track_reference_keyframe_batch.py's: a map point's id is its slot."""
import numpy as np
import pytest

import pixel_scene as ps
import test_gpu_track_reference_keyframe_batch as tb_
from test_gpu_kb8_track_reference_keyframe import rig  # noqa: F401 (the KannalaBrandt8 agent's fixture)
from test_gpu_track_reference_keyframe_batch import scene, world  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

KEYS = tb_.FORM_B_KEYS
LOCAL_KEYS = ("n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers", "mp", "outlier", "pose", "Tcw")
SLOT_KEYPOINTS = 4096
STATE, INVALID, CAPACITY = -6, -1, -3


def _putable(kf, K, scale, inv_s2, bounds=tb_.BOUNDS):
    s2 = (np.asarray(scale, np.float32) ** 2).astype(np.float32)
    return dict(kps=kf["kps"], desc=kf["desc"], fv=kf["fv"], K=np.asarray(K, np.float32), bounds=np.asarray(bounds, np.float32), scale_factors=scale,
                level_sigma2=s2, inv_level_sigma2=inv_s2, log_scale_factor=float(np.log(scale[1])))


class Stores:
    """A keyframe store and map stores over the world's table (slot = table index = the caller's id)."""

    def __init__(self, capi, w):
        self.capi, self.w = capi, w
        self.kfs = capi.KeyframeStore(8, SLOT_KEYPOINTS)
        self.maps = {}

    def map(self, name="pts", pts=None):
        if name not in self.maps:
            pts = self.w["pts"] if pts is None else pts
            m = self.capi.MapStore(len(pts))
            m.update(np.arange(len(pts), dtype=np.int32), pts)
            self.maps[name] = m
        return self.maps[name]

    def put(self, slot, kf, K=ps.K, bounds=tb_.BOUNDS):
        self.kfs.put(np.array([slot], np.int32), [_putable(kf, K, self.w["scale"], self.w["inv_s2"], bounds)])

    def close(self):
        self.kfs.close()
        for m in self.maps.values():
            m.close()


def _same(a, b, keys=KEYS):
    assert a["status"] == b["status"]
    if "mp" not in b:
        assert "mp" not in a and all(a[k] == b[k] for k in ("n", "nmatches", "n_edges", "n_bow", "n_fv"))
        return
    tb_._same(a, b, keys)


def test_mixed_tick_then_second_half(scene, world):  # noqa: F811
    """B = 5: one frame tracked by its motion model (NULL), four that run -- two keyframes, one of them twice under two mp_slot lists --,
    then dvm_track_local_map_batch behind either call."""
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    st = Stores(capi, w)
    ts = [1, 2, 3, 4, 5]
    modes = ["ok", "fail", "fail", "none", "none"]
    holes = w["kfs"][0]["mp"].copy(); holes[::5] = -1
    kf_up = [None, tb_._kf(capi, w, w["voc"], which=0), tb_._kf(capi, w, w["voc"], which=0, mp=holes), tb_._kf(capi, w, w["voc"], which=1),
             tb_._kf(capi, w, w["voc"], which=1)]
    st.put(5, kf_up[1]); st.put(2, kf_up[3])
    m = st.map()
    kf_res = [None, (5, m, kf_up[1]["mp"]), (5, m, holes), (2, m, kf_up[3]["mp"]), (2, m, kf_up[4]["mp"])]
    pose_last = [tb_._tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext, tb = tb_._new_batch(capi, 5, local=5 * 16384)
    out = {}
    for form in ("uploaded", "resident"):
        first = tb_._first_batch(tb, w, frames, poses, ts, modes)
        assert [bool(f["tracked"]) for f in first] == [True, False, False, False, False]
        mp0 = first[0]["mp"].astype(np.int32).copy()
        if form == "uploaded":
            r = tb.track_reference_keyframe(vocd, kf_up, pose_last, ps.K, w["inv_s2"])
        else:
            r = tb.track_reference_keyframe_resident(vocd, st.kfs, kf_res, pose_last, ps.K, w["inv_s2"])
        up_bytes = tb.last_refkf_upload_bytes()
        lm = tb.track_local_map([w["pts"]] * 5, [mp0] + [x["mp"].astype(np.int32) for x in r[1:]], th=1.0)
        out[form] = (r, lm, up_bytes)
    (ru, lu, bu), (rr, lr, br) = out["uploaded"], out["resident"]
    for b in range(5):
        _same(rr[b], ru[b])
        assert lr[b]["status"] == lu[b]["status"] == capi.DVM_TRACK_COMPLETE
        tb_._same(lr[b], lu[b], LOCAL_KEYS)
    assert all(rr[b]["nmatches"] >= 15 for b in range(1, 5)) and rr[2]["nmatches"] < rr[1]["nmatches"]
    # 4 B per keypoint and the per-frame arrays against descriptors, flags, positions and the FeatureVector
    n_tot = sum(len(k["kps"]) for k in kf_up[1:])
    assert br < 4 * (n_tot + 4 * 64) + 4096 and bu > 50 * n_tot
    tb.close(); ext.close(); st.close(); vocd.close()


def test_batch_of_one_on_a_single_frame_tracker(scene, world):  # noqa: F811
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    pts = w["pts"]
    vocd = capi.Vocabulary(w["voc"])
    st = Stores(capi, w)
    kf = tb_._kf(capi, w, w["voc"])
    st.put(0, kf)
    res_kf = (0, st.map(), kf["mp"])
    pose_last = tb_._tcw7f(ps.pose7(*poses[2]))
    A = tb_.Single(capi, w, local=len(pts))
    B = tb_.Single(capi, w, local=len(pts))
    A.trk.reserve_reference_keyframe_batch(8192); B.trk.reserve_reference_keyframe_batch(8192)
    pred = tb_._pred(poses, 3, "fail")
    fa = A.first(frames[3], pred, tb_._last(w, "ok")); fb = B.first(frames[3], pred, tb_._last(w, "ok"))
    assert not fa["tracked"] and not fb["tracked"]
    ra = capi.TrackerBatch.track_reference_keyframe(A.trk, vocd, [kf], [pose_last], ps.K, w["inv_s2"])[0]
    rb = B.trk.track_reference_keyframe_resident(vocd, st.kfs, res_kf, pose_last, ps.K, w["inv_s2"])
    _same(rb, ra)
    assert rb["status"] == capi.DVM_TRACK_COMPLETE
    # refused a second time on that finish, as the uploaded call is; the single call too
    for again in (lambda: B.trk.track_reference_keyframe_resident(vocd, st.kfs, res_kf, pose_last, ps.K, w["inv_s2"]), lambda: B.refkf(vocd, kf, pose_last)):
        with pytest.raises(capi.DvmError) as e:
            again()
        assert e.value.code == STATE
    fm = rb["mp"].astype(np.int32)
    tb_._same(B.trk.track_local_map(pts, fm, th=1.0), A.trk.track_local_map(pts, fm, th=1.0), LOCAL_KEYS)
    A.close(); B.close(); st.close(); vocd.close()


def test_edge_keyframes_in_one_batch(scene, world):  # noqa: F811
    """An empty keyframe, one without a FeatureVector, one whose points are all bad, one whose points are nearly all unobserved, one with
    few points, FeatureVectors of 1, 2, 3 (mod 4) nodes: FEW_MATCHES and FEW_MAP_MATCHES side by side with a complete frame."""
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    st = Stores(capi, w)
    k0 = w["kfs"][0]
    kf = tb_._kf(capi, w, w["voc"])
    none = dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))
    empty = dict(kps=k0["kps"][:0], desc=k0["desc"][:0], mp=np.zeros(0, np.int32), pos=np.zeros((0, 3), np.float32), n_obs=np.zeros(0, np.int32), bad=None, fv=none)
    nofv = dict(kf, fv=none)
    pb = w["pts"].copy(); pb["bad"] = 1
    p0 = w["pts"].copy(); p0["n_obs"] = 0; p0["n_obs"][:5] = 2
    few_mp = k0["mp"].copy(); few_mp[12:] = -1
    nf = len(kf["fv"]["fv_nodes"])
    cuts = [tb_._cut_fv(kf, r + 4 * ((nf - r) // 4)) for r in (1, 2, 3)]
    assert [len(c["fv"]["fv_nodes"]) % 4 for c in cuts] == [1, 2, 3]
    up = [empty, nofv, tb_._kf(capi, w, w["voc"], pts=pb), tb_._kf(capi, w, w["voc"], pts=p0), tb_._kf(capi, w, w["voc"], mp=few_mp)] + cuts + [kf]
    # slots: 0 empty, 1 no FeatureVector, 2 the whole keyframe, 3..5 the cut ones
    st.put(0, dict(empty, fv=None)); st.put(1, dict(nofv, fv=None)); st.put(2, kf)
    for i, c in enumerate(cuts):
        st.put(3 + i, c)
    m, mb, m0 = st.map(), st.map("bad", pb), st.map("unobserved", p0)
    res = [(0, None, np.zeros(0, np.int32)), (1, m, kf["mp"]), (2, mb, kf["mp"]), (2, m0, kf["mp"]), (2, m, few_mp)] + [(3 + i, m, kf["mp"]) for i in range(3)] + \
          [(2, m, kf["mp"])]
    B = len(up)
    ts = [1 + b % 3 for b in range(B)]
    pose_last = [tb_._tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext, tb = tb_._new_batch(capi, B)
    tb_._first_batch(tb, w, frames, poses, ts, ["none"] * B)
    ru = tb.track_reference_keyframe(vocd, up, pose_last, ps.K, w["inv_s2"])
    tb_._first_batch(tb, w, frames, poses, ts, ["none"] * B)
    rr = tb.track_reference_keyframe_resident(vocd, st.kfs, res, pose_last, ps.K, w["inv_s2"])
    for b in range(B):
        _same(rr[b], ru[b])
    s = [r["status"] for r in rr]
    assert s[0] == s[1] == s[2] == s[4] == capi.DVM_TRACK_FEW_MATCHES and rr[2]["nmatches"] == 0
    assert s[3] == capi.DVM_TRACK_FEW_MAP_MATCHES and s[-1] == capi.DVM_TRACK_COMPLETE
    tb.close(); ext.close(); st.close(); vocd.close()


def test_feature_vectors_that_end_in_node_minus_one(scene, world):  # noqa: F811
    import test_gpu_track_reference_keyframe as one
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    voc, levelsup = one.early_leaf_vocabulary(dict(desc=w["kfs"][0]["desc"], pts=w["pts"]))
    vocd = capi.Vocabulary(voc)
    st = Stores(capi, w)
    ts, which = [1, 3], [0, 1]
    up = [tb_._kf(capi, w, voc, which=k, levelsup=levelsup) for k in which]
    assert all(k["fv"]["fv_nodes"][-1] == -1 for k in up)
    for i, k in enumerate(up):
        st.put(i, k)
    res = [(i, st.map(), k["mp"]) for i, k in enumerate(up)]
    pose_last = [tb_._tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext, tb = tb_._new_batch(capi, 2)
    tb_._first_batch(tb, w, frames, poses, ts, ["none"] * 2)
    ru = tb.track_reference_keyframe(vocd, up, pose_last, ps.K, w["inv_s2"], levelsup=levelsup)
    tb_._first_batch(tb, w, frames, poses, ts, ["none"] * 2)
    rr = tb.track_reference_keyframe_resident(vocd, st.kfs, res, pose_last, ps.K, w["inv_s2"], levelsup=levelsup)
    for b in range(2):
        _same(rr[b], ru[b])
        assert rr[b]["status"] == capi.DVM_TRACK_COMPLETE and one.matches_in_node_minus_one(rr[b]) >= 5
    tb.close(); ext.close(); st.close(); vocd.close()


def test_kannala_brandt8_tracker(rig):  # noqa: F811
    import kb8_track_scene as kt
    capi, sc, kf = rig["capi"], rig["sc"], rig["kf"]
    st = Stores(capi, rig["w"])
    st.put(1, kf, K=kt.P[:4], bounds=kt.BOUNDS)
    res_kf = (1, st.map(), kf["mp"])
    extB = capi.OrbExtractor(max_batch=2)
    trkB = capi.TrackerBatch(extB, 2)
    trkB.reserve_reference_keyframe(4096)
    wrong = sc["Tcw_pred"].copy(); wrong[4] += 100.0
    lasts = [(sc["kps_l"], sc["mp_l"], None, sc["mps"])] * 2
    ins, keep = trkB.prepare([sc["Tcw_pred"], wrong], lasts)
    imgs = np.stack([sc["img_c"], sc["img_c"]])
    got = trkB.track(imgs, ins, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], th=kt.TH, model=rig["model"])
    assert [g["tracked"] for g in got] == [1, 0]
    ru = trkB.track_reference_keyframe(rig["vocd"], [None, kf], [None, sc["Tcw_pred"]], kt.P[:4], rig["inv_s2"])
    trkB.track(imgs, ins, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], th=kt.TH, model=rig["model"])
    rr = trkB.track_reference_keyframe_resident(rig["vocd"], st.kfs, [None, res_kf], [None, sc["Tcw_pred"]], kt.P[:4], rig["inv_s2"])
    for b in range(2):
        _same(rr[b], ru[b])
    assert rr[1]["status"] == capi.DVM_TRACK_COMPLETE and rr[1]["nmatches"] > 100 and rr[1]["outlier"].sum() > 0
    trkB.close(); extB.close(); st.close()


def test_refusals_leave_the_finish_usable_and_an_update_is_seen(scene, world):  # noqa: F811
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    st = Stores(capi, w)
    kf = tb_._kf(capi, w, w["voc"])
    n = len(kf["kps"])
    st.put(0, kf); st.put(3, kf)
    st.kfs.remove(np.array([3], np.int32))
    m = st.map()
    ts, modes = [1, 2], ["fail", "none"]
    pose_last = [tb_._tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext = capi.OrbExtractor(max_batch=2)
    tb = capi.TrackerBatch(ext, 2)
    good = (0, m, kf["mp"])

    def call(a=good, b=good):
        return tb.track_reference_keyframe_resident(vocd, st.kfs, [a, b], pose_last, ps.K, w["inv_s2"])

    def refused(code, *a):
        with pytest.raises(capi.DvmError) as e:
            call(*a)
        assert e.value.code == code, e.value.code

    tb_._first_batch(tb, w, frames, poses, ts, modes)
    refused(STATE)                                         # no reservation yet
    span = (n + 63) // 64 * 64
    tb.reserve_reference_keyframe(2 * span - 64)
    refused(CAPACITY)
    tb.reserve_reference_keyframe(2 * span)
    first = int(np.flatnonzero(kf["mp"] >= 0)[0])

    def with_slot(v):
        mp = kf["mp"].copy(); mp[first] = v
        return (0, m, mp)
    for bad in ((8, m, kf["mp"]), (-1, m, kf["mp"]), (1, m, kf["mp"]), (3, m, kf["mp"]), with_slot(len(w["pts"])), with_slot(-2), (0, m, None), (0, None, kf["mp"])):
        refused(INVALID, good, bad)
    if capi.device_count() > 1:
        far = capi.MapStore(len(w["pts"]), device=1)
        far.update(np.arange(len(w["pts"]), dtype=np.int32), w["pts"])
        refused(INVALID, good, (0, far, kf["mp"]))
        far_kfs = capi.KeyframeStore(1, 64, device=1)
        with pytest.raises(capi.DvmError) as e:
            tb.track_reference_keyframe_resident(vocd, far_kfs, [good, good], pose_last, ps.K, w["inv_s2"])
        assert e.value.code == INVALID
        far.close(); far_kfs.close()
        capi.MapStore(1, device=0).close()          # (the calling thread's current device is 0 again)
    # the finish is still there for the corrected call; the uploaded call on the same frames gives the same
    rr = call()
    refused(STATE)                                         # once per finish
    tb_._first_batch(tb, w, frames, poses, ts, modes)
    ru = tb.track_reference_keyframe(vocd, [kf, kf], pose_last, ps.K, w["inv_s2"])
    for b in range(2):
        _same(rr[b], ru[b])
        assert rr[b]["status"] == capi.DVM_TRACK_COMPLETE
    # the next tick after a map-store update (no synchronisation in between): half the keyframe's points went bad, the others moved
    ids = kf["mp"][kf["mp"] >= 0]
    rec = w["pts"][ids].copy()
    rec["bad"][::2] = 1
    rec["pos"][1::2] += np.float32(0.02)
    m.update(ids, rec)
    tb_._first_batch(tb, w, frames, poses, ts, modes)
    r2 = call()
    pts2 = w["pts"].copy(); pts2[ids] = rec
    kf2 = tb_._kf(capi, w, w["voc"], pts=pts2)
    tb_._first_batch(tb, w, frames, poses, ts, modes)
    u2 = tb.track_reference_keyframe(vocd, [kf2, kf2], pose_last, ps.K, w["inv_s2"])
    for b in range(2):
        _same(r2[b], u2[b])
    assert r2[0]["nmatches"] < rr[0]["nmatches"] and not np.array_equal(r2[0]["pose"], rr[0]["pose"])
    ext.sync()
    tb.close(); ext.close(); st.close(); vocd.close()
