"""dvm_track_reference_keyframe[_batch] for a KannalaBrandt8 agent: forms (a) and (b) and the batch with one frame that needs it against
dvmh_vocab_transform + dvmh_search_by_bow_kf_frame + dvm_pose_optimize_cam, bit for bit, and dvm_track_local_map behind the chain against
its own composition.  The keyframe and the vocabulary as tests/test_gpu_track_reference_keyframe.py builds them; the keyframe is the last
frame of tests/kb8_track_scene.py, its map points behind its keypoints through the fisheye model."""
import numpy as np
import pytest

import kb8_track_scene as kt
import test_gpu_track_local_map as tlm
import test_gpu_track_reference_keyframe as rk     # _kf / _check_against_separate: the pinhole test's composition, on kt.CamCalls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    from dvm_slam_amd import capi, synth
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    trk = capi.Tracker(ext)
    trk.reserve_reference_keyframe(8192)
    trk.reserve_local_map(4096)
    model = kt.model_of(capi)
    r = dict(capi=capi, ext=ext, trk=trk, scale=tab["scale"], inv_s2=tab["inv_sigma2"], model=model, cam=kt.CamCalls(capi, model))
    sc = r["sc"] = kt.reference(lambda im: ext.extract(im), r["scale"], r["inv_s2"])
    rng = np.random.default_rng(31)
    Ow = -sc["R"].T @ sc["t"]
    pts = kt.local_points(capi, sc["kps_l"], sc["mps"]["pos"].astype(np.float64), sc["mps"]["desc"], Ow, r["scale"], rng)
    voc = synth.vocabulary(k=10, L=6, ragged=False, seed=5)
    pool = np.concatenate([sc["mps"]["desc"], sc["desc_c"]])
    voc["desc"] = pool[rng.integers(0, len(pool), voc["n_nodes"])]
    mp = sc["mp_l"].copy()
    mp[rng.random(len(mp)) < 0.05] = -1
    r["w"] = dict(scale=r["scale"], inv_s2=r["inv_s2"], pts=pts, voc=voc, kps=sc["kps_l"], desc=sc["mps"]["desc"], mp=mp)
    r["kf"] = rk._kf(r["cam"], r["w"], voc)
    r["vocd"] = capi.Vocabulary(voc)
    yield r
    r["vocd"].close(); trk.close(); ext.close()


def _form_a(rig, trk=None):
    sc = rig["sc"]
    return (trk or rig["trk"]).track_reference_keyframe(rig["vocd"], rig["kf"], sc["Tcw_pred"], img=sc["img_c"], bounds=kt.BOUNDS, inv_sigma2=rig["inv_s2"],
                                                        model=rig["model"])


def _failed_first_half(rig, trk=None):
    """The motion model fails: a prediction far off, no point projects into the image."""
    sc = rig["sc"]
    wrong = sc["Tcw_pred"].copy(); wrong[4] += 100.0
    f = (trk or rig["trk"]).track(sc["img_c"], wrong, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], sc["kps_l"], sc["mp_l"], None, sc["mps"], th=kt.TH,
                                  model=rig["model"])
    assert not f["tracked"]
    return f


def test_form_a_equals_separate_calls(rig):
    capi, sc = rig["capi"], rig["sc"]
    r = _form_a(rig)
    assert r["n"] == len(sc["kps_c"]) and np.array_equal(r["kps"], sc["kps_c"]) and np.array_equal(r["desc"], sc["desc_c"]) and np.array_equal(r["kps_un"], sc["kps_c"])
    assert r["status"] == capi.DVM_TRACK_COMPLETE and r["nmatches"] > 100 and r["n_bow"] > 100
    rk._check_against_separate(rig["cam"], None, r, rig["kf"], rig["w"]["voc"], r["desc"], r["kps_un"], sc["Tcw_pred"], rig["inv_s2"], oracle=False)
    assert np.abs(r["pose"][:3] - sc["gt"][:3]).max() < 0.01          # and it finds the camera through the fisheye model
    assert r["outlier"].sum() > 0


def test_form_b_equals_form_a_and_the_second_half_follows(rig):
    capi, sc = rig["capi"], rig["sc"]
    a = _form_a(rig)
    _failed_first_half(rig)
    b = rig["trk"].track_reference_keyframe(rig["vocd"], rig["kf"], sc["Tcw_pred"], inv_sigma2=rig["inv_s2"], model=rig["model"])
    for k, v in a.items():
        if k not in ("kps", "desc", "kps_un"):
            assert np.array_equal(np.asarray(v), np.asarray(b[k])), k
    assert b["status"] == capi.DVM_TRACK_COMPLETE
    # dvm_track_local_map behind the chain: seeded from its pose, on the model the frame's finish ran on
    pts = rig["w"]["pts"]
    fused = rig["trk"].track_local_map(pts, b["mp"], th=5.0, want_track_points=True)
    sep = tlm._separate(rig["cam"], sc["kps_c"], sc["desc_c"], b["mp"], pts, b["Tcw"], kt.P[:4], kt.BOUNDS, rig["scale"], rig["inv_s2"], 5.0, False, 0.0)
    tlm._check(fused, sep, exact=True)
    assert fused["n_edges"] > 100
    # ... and behind form (a), which leaves the frame as a finish does
    a2 = _form_a(rig)
    fused = rig["trk"].track_local_map(pts, a2["mp"], th=1.0, want_track_points=True)
    sep = tlm._separate(rig["cam"], sc["kps_c"], sc["desc_c"], a2["mp"], pts, a2["Tcw"], kt.P[:4], kt.BOUNDS, rig["scale"], rig["inv_s2"], 1.0, False, 0.0)
    tlm._check(fused, sep, exact=True)


def test_form_a_refuses_distortion_under_the_fisheye_model(rig):
    capi, sc = rig["capi"], rig["sc"]
    dist = capi.Distortion(300.0, 300.0, 320.0, 240.0, -0.04, 0.01, 0.0, 0.0, 0.0)
    with pytest.raises(capi.DvmError) as e:
        rig["trk"].track_reference_keyframe(rig["vocd"], rig["kf"], sc["Tcw_pred"], img=sc["img_c"], bounds=kt.BOUNDS, inv_sigma2=rig["inv_s2"], dist=dist,
                                            model=rig["model"])
    assert e.value.code == -1 and "KannalaBrandt8" in str(e.value)
    # nothing was queued and the begin stays: the corrected call runs on it (form (a) without a new image is form (a) still)
    r = rig["trk"].track_reference_keyframe(rig["vocd"], rig["kf"], sc["Tcw_pred"], bounds=kt.BOUNDS, inv_sigma2=rig["inv_s2"], model=rig["model"])
    a = _form_a(rig)
    assert r["status"] == capi.DVM_TRACK_COMPLETE and np.array_equal(r["pose"], a["pose"]) and np.array_equal(r["mp"], a["mp"])


def test_batch_with_one_frame_that_needs_it(rig):
    capi, sc = rig["capi"], rig["sc"]
    extB = capi.OrbExtractor(max_batch=2)
    trkB = capi.TrackerBatch(extB, 2)
    trkB.reserve_reference_keyframe(4096)
    wrong = sc["Tcw_pred"].copy(); wrong[4] += 100.0
    lasts = [(sc["kps_l"], sc["mp_l"], None, sc["mps"])] * 2
    ins, keep = trkB.prepare([sc["Tcw_pred"], wrong], lasts)
    got = trkB.track(np.stack([sc["img_c"], sc["img_c"]]), ins, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], th=kt.TH, model=rig["model"])
    assert [g["tracked"] for g in got] == [1, 0]
    res = trkB.track_reference_keyframe(rig["vocd"], [None, rig["kf"]], [None, sc["Tcw_pred"]], kt.P[:4], rig["inv_s2"])
    assert res[0]["status"] == capi.DVM_TRACK_COMPLETE and "mp" not in res[0]
    _failed_first_half(rig)
    one = rig["trk"].track_reference_keyframe(rig["vocd"], rig["kf"], sc["Tcw_pred"], inv_sigma2=rig["inv_s2"], model=rig["model"])
    for k, v in one.items():
        assert np.array_equal(np.asarray(v), np.asarray(res[1][k])), k
    assert res[1]["status"] == capi.DVM_TRACK_COMPLETE
    trkB.close(); extB.close()
