"""The first half of a KannalaBrandt8 agent's tracked frame (dvm_tracker_set_camera_model, dvmh_track_with_motion_model[_batch]_cam,
Tracker.track(..., model=)): ONE device chain against the composition of the separate calls -- OrbExtractor.extract +
dvmh_search_by_projection_frames_cam + the edge gather in keypoint order + dvm_pose_optimize_cam -- bit for bit.  Those calls are held to
kb8_scene's float64 restatement by tests/test_gpu_kb8.py; tests/test_kb8_track_scene.py pins the scene on the CPU."""
import ctypes as C

import numpy as np
import pytest

import kb8_scene as ks
import kb8_track_scene as kt
import pixel_scene as ps

pytestmark = pytest.mark.gpu

DVM_ERR_INVALID, DVM_ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def rig():
    from dvm_slam_amd import capi
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    trk = capi.Tracker(ext)
    yield dict(capi=capi, ext=ext, trk=trk, scale=tab["scale"], inv_s2=tab["inv_sigma2"], model=kt.model_of(capi))
    trk.close(); ext.close()


@pytest.fixture(scope="module")
def ref(rig):
    """The scene tests/test_kb8_track_scene.py pins, on the device extractor's keypoints (the oracle's, bit for bit)."""
    return kt.reference(lambda im: rig["ext"].extract(im), rig["scale"], rig["inv_s2"])


def _both(rig, img, Tcw, kps_l, mp_l, outl_l, mps, th, check_ori=True):
    fused = rig["trk"].track(img, Tcw, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], kps_l, mp_l, outl_l, mps, th=th, check_ori=check_ori, model=rig["model"])
    sep = kt.separate_first(rig["capi"], rig["ext"], rig["model"], img, Tcw, rig["scale"], rig["inv_s2"], kps_l, mp_l, outl_l, mps, th, check_ori)
    assert fused["replayed_on_host"] == 0
    kt.check_first(fused, sep)
    return fused


@pytest.mark.parametrize("check_ori", [False, True])
def test_scene_chain_equals_separate_calls(rig, ref, check_ori):
    sc = ref
    f = _both(rig, sc["img_c"], sc["Tcw_pred"], sc["kps_l"], sc["mp_l"], None, sc["mps"], kt.TH, check_ori)
    assert f["tracked"] and not f["wide_window"] and f["nmatches_search"] > 500
    if not check_ori:
        # ... and it is the tracking step the float64 reference describes: the planted points rejected, the pose at the truth
        planted = np.flatnonzero(sc["planted"])
        assert not np.isin(f["mp"], planted).any() and np.isin(f["dropped"], planted).sum() >= 10
        assert np.abs(f["pose"] - sc["pose"]).max() < 1e-3 and np.abs(f["pose"][:3] - sc["gt"][:3]).max() < 0.01


def test_rendered_frames_chain_equals_separate_calls(rig):
    """Three frames of pixel_scene.render, each tracked from the one before: the map points behind the last frame's keypoints through the
    fisheye model, one in five without observations, one last-frame keypoint in ten without a point, the last frame's outlier flags set
    on a few."""
    capi, ext = rig["capi"], rig["ext"]
    frames, _ = ps.render(4)
    rng = np.random.default_rng(31)
    R = kt._rot(rng.normal(size=3), 0.3); t = rng.uniform(-1.0, 1.0, 3)
    Tcw = np.r_[kt.R_to_quat(R), t].astype(np.float32)
    for i in (1, 2, 3):
        n0, k0, d0, _ = ext.extract(frames[i - 1])
        mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
        mps["pos"] = kt.points_behind(k0, R, t, rng.uniform(4.0, 40.0, n0)).astype(np.float32); mps["desc"] = d0
        mps["n_obs"] = np.where(rng.random(n0) < 0.2, 0, 1)
        mp_l = np.arange(n0, dtype=np.int32); mp_l[rng.random(n0) < 0.1] = -1
        outl_l = (rng.random(n0) < 0.05).astype(np.uint8)
        f = _both(rig, frames[i], Tcw, k0, mp_l, outl_l, mps, 15.0)
        assert f["tracked"] and f["nmatches"] > 100


def test_dense_stream_requeries_on_device(rig):
    from dvm_slam_amd import synth
    capi, ext = rig["capi"], rig["ext"]
    frames = synth.frame_stream(4)
    rng = np.random.default_rng(9)
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    total = 0
    for i in (1, 2, 3):
        n0, k0, d0, _ = ext.extract(frames[i - 1])
        mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
        mps["pos"] = kt.points_behind(k0, np.eye(3), np.zeros(3), rng.uniform(3.0, 9.0, n0)).astype(np.float32); mps["desc"] = d0; mps["n_obs"] = 1
        f = _both(rig, frames[i], Tcw, k0, np.arange(n0, dtype=np.int32), None, mps, 15.0)
        total += f["n_requeried"]
    assert total > 0       # the case this test is for did occur


def _yawed(sc, px):
    """The true pose turned about the camera's y axis by px / fx rad: every projection some px pixels off along u."""
    p = kt.oplus(sc["gt"], np.r_[0.0, px / float(kt.P[0]), 0.0, 0.0, 0.0, 0.0])
    return np.r_[p[3:7], p[0:3]].astype(np.float32)


def _level0_points(sc, count):
    """mp_l with only `count` points left: unplanted, on keypoints of level 0, near the image centre (window radius th * 1)."""
    k = sc["kps_l"]
    ok = (~sc["planted"]) & (k["octave"] == 0) & (np.abs(k["x"] - 320) < 200) & (np.abs(k["y"] - 240) < 150)
    mp_l = np.full(len(k), -1, np.int32)
    idx = np.flatnonzero(ok)[:count]
    assert len(idx) == count
    mp_l[idx] = idx
    return mp_l


def test_doubled_window_retry(rig, ref):
    """A prediction 20 px off and points on level-0 keypoints only: nothing within th = 15, the matches within 2 th."""
    sc = ref
    f = _both(rig, sc["img_c"], _yawed(sc, 20.0), sc["kps_l"], _level0_points(sc, 60), None, sc["mps"], kt.TH, False)
    assert f["wide_window"] == 1 and f["tracked"] == 1 and f["nmatches_search"] >= 20


def test_few_matches_returns_no_pose(rig, ref):
    sc = ref
    Tcw = _yawed(sc, 20.0)
    f = _both(rig, sc["img_c"], Tcw, sc["kps_l"], _level0_points(sc, 12), None, sc["mps"], kt.TH, False)
    assert f["wide_window"] == 1 and f["tracked"] == 0 and 0 < f["nmatches_search"] < 20
    assert (f["mp"] >= 0).sum() == f["nmatches_search"] and (f["dropped"] == -1).all()      # mp_c as the (doubled) search left it
    assert np.array_equal(f["Tcw"], Tcw) and np.array_equal(f["pose"], np.r_[Tcw[4:7], Tcw[0:4]].astype(np.float64))


def _pinhole_frame(rig, frames, k0, mps, model=None):
    K = None if model is not None else ps.K
    return rig["trk"].track(frames[1], np.array([0, 0, 0, 1, 0, 0, 0], np.float32), K, kt.BOUNDS, rig["scale"], rig["inv_s2"], k0,
                            np.arange(len(k0), dtype=np.int32), None, mps, th=15.0, model=model)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def pinhole_case(rig):
    capi, ext = rig["capi"], rig["ext"]
    frames, _ = ps.render(2)
    n0, k0, d0, _ = ext.extract(frames[0])
    mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
    mps["pos"] = ps.backproject(k0, np.eye(3), np.zeros(3)).astype(np.float32); mps["desc"] = d0; mps["n_obs"] = 1
    return frames, k0, mps


def test_model_0_through_the_cam_entry_is_the_plain_entry(rig, pinhole_case):
    rig["trk"].set_camera_model(None)
    plain = _pinhole_frame(rig, *pinhole_case)
    cam = _pinhole_frame(rig, *pinhole_case, model=rig["capi"].CameraModel.pinhole(*ps.K))
    assert plain["tracked"] and plain["nmatches"] > 200
    _same(plain, cam)


def test_set_camera_model_none_restores_the_pinhole_chain(rig, ref, pinhole_case):
    sc = ref
    rig["trk"].set_camera_model(None)
    before = _pinhole_frame(rig, *pinhole_case)
    kb8 = _both(rig, sc["img_c"], sc["Tcw_pred"], sc["kps_l"], sc["mp_l"], None, sc["mps"], kt.TH)
    assert kb8["tracked"]
    # the tracker is still on the fisheye model: the plain entry's pinhole queries meet the fisheye PoseOptimization
    mixed = _pinhole_frame(rig, *pinhole_case)
    assert not np.array_equal(mixed["pose"], before["pose"])
    rig["trk"].set_camera_model(None)
    _same(_pinhole_frame(rig, *pinhole_case), before)


def test_batch_equals_single_frames(rig, ref):
    capi, sc = rig["capi"], ref
    extB = capi.OrbExtractor(max_batch=3)
    trkB = capi.TrackerBatch(extB, 3)
    n = len(sc["kps_l"])
    none = np.full(n, -1, np.int32)
    lasts = [(sc["kps_l"], none, None, sc["mps"]), (sc["kps_l"], _level0_points(sc, 40), None, sc["mps"]), (sc["kps_l"], sc["mp_l"], None, sc["mps"])]
    Ts = [sc["Tcw_pred"]] * 3
    ins, keep = trkB.prepare(Ts, lasts)
    got = trkB.track(np.stack([sc["img_c"], sc["img_l"], sc["img_c"]]), ins, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], th=kt.TH, model=rig["model"])
    imgs = (sc["img_c"], sc["img_l"], sc["img_c"])
    for b in range(3):
        kl, ml, _, mps = lasts[b]
        one = rig["trk"].track(imgs[b], Ts[b], None, kt.BOUNDS, rig["scale"], rig["inv_s2"], kl, ml, None, mps, th=kt.TH, model=rig["model"])
        kt.check_first(got[b], one, requeried=True)
        assert got[b]["replayed_on_host"] == 0
    assert [g["tracked"] for g in got] == [0, 1, 1] and got[0]["nmatches_search"] == 0 and got[1]["nmatches_search"] < 45
    trkB.close(); extB.close()


class _Queries(C.Structure):
    """dvm_track_queries (include/dvmslam_hip.h)"""
    _fields_ = [("nq", C.c_int32)] + [(k, C.c_void_p) for k in ("qdesc", "qx", "qy", "qr", "qmin", "qmax", "q_claims", "q_angle", "q_pos")] + \
               [("bounds", C.c_float * 4), ("dist", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("nlevels", C.c_int32), ("cam", C.c_double * 5),
                ("pose_in", C.c_double * 7), ("th_high", C.c_int32), ("check_ori", C.c_int32), ("min_matches", C.c_int32)]


class _Result(C.Structure):
    """dvm_track_result (include/dvmslam_hip.h)"""
    _fields_ = [(k, C.c_int32) for k in ("n", "mono_index", "status", "nmatches", "nmatches_before_rotation", "n_edges", "n_inliers", "nmatches_map",
                                         "nmatches_after", "n_requeried")] + [("pose", C.c_double * 7)]


def test_errors(rig, ref):
    capi, trk, ext, sc = rig["capi"], rig["trk"], rig["ext"], ref
    L = capi.lib()
    dist = capi.Distortion(300.0, 300.0, 320.0, 240.0, -0.04, 0.01, 0.0, 0.0, 0.0)

    def track(**kw):
        return trk.track(sc["img_c"], sc["Tcw_pred"], None, kt.BOUNDS, rig["scale"], rig["inv_s2"], sc["kps_l"], sc["mp_l"], None, sc["mps"], th=kt.TH, **kw)
    # an unknown model, a zero focal length: DVM_ERR_INVALID, the tracker keeps the model it had
    trk.set_camera_model(rig["model"])
    for bad in (capi.CameraModel.make(7, kt.P), capi.CameraModel.make(1, np.r_[0.0, kt.P[1:]])):
        with pytest.raises(capi.DvmError) as e:
            trk.set_camera_model(bad)
        assert e.value.code == DVM_ERR_INVALID
        with pytest.raises(capi.DvmError) as e:
            track(model=bad)
        assert e.value.code == DVM_ERR_INVALID
    # (still the fisheye model: distortion coefficients are refused, as only that model refuses them, and the message says why)
    with pytest.raises(capi.DvmError) as e:
        trk.track(sc["img_c"], sc["Tcw_pred"], kt.P[:4], kt.BOUNDS, rig["scale"], rig["inv_s2"], sc["kps_l"], sc["mp_l"], None, sc["mps"], th=kt.TH, dist=dist)
    assert e.value.code == DVM_ERR_INVALID and "KannalaBrandt8" in str(e.value) and "mDistCoef" in str(e.value)
    # k1 != 0 under model 1 is refused before anything is queued: a finish with valid arguments still succeeds on the same begin
    img = np.ascontiguousarray(sc["img_c"])
    vp = C.c_void_p
    L.dvm_track_begin.restype = C.c_int32
    L.dvm_track_begin.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.dvm_track_finish.restype = C.c_int32
    L.dvm_track_finish.argtypes = [vp] * 5 + [C.c_int32] + [vp] * 5
    capi.check(L.dvm_track_begin(trk.t, ext.h, img.ctypes.data, 480, 640, img.strides[0], 0, 1000))
    q = _Queries()
    q.bounds[:] = [float(v) for v in kt.BOUNDS]
    s2 = np.ascontiguousarray(rig["inv_s2"], np.float32)
    q.inv_level_sigma2, q.nlevels = s2.ctypes.data, len(s2)
    q.pose_in[:] = [0, 0, 0, 0, 0, 0, 1]
    q.th_high, q.check_ori, q.min_matches = 100, 1, 20
    cap = ext.cap
    kps = np.zeros(cap, capi.KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); assign = np.full(cap, -7, np.int32); outl = np.full(cap, 7, np.uint8)
    res = _Result()
    args = lambda: (trk.t, ext.h, C.addressof(q), kps.ctypes.data, desc.ctypes.data, cap, None, assign.ctypes.data, outl.ctypes.data, None, C.addressof(res))
    q.dist = C.addressof(dist)
    assert L.dvm_track_finish(*args()) == DVM_ERR_INVALID
    assert (assign == -7).all() and (outl == 7).all() and not kps["x"].any()
    q.dist = None
    capi.check(L.dvm_track_finish(*args()))
    assert res.n == len(sc["kps_c"]) and res.status == 1 and np.array_equal(kps["x"][:res.n], sc["kps_c"]["x"])      # DVM_TRACK_FEW_MATCHES: no query
    trk.set_camera_model(None)
