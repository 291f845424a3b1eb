"""GPU tests of the camera-model entries (dvm_pose_optimize_cam, dvm_is_in_frustum_cam, dvm_project_search_cam,
dvmh_search_by_projection_frames_cam):

  1. the pinhole guard: model 0 returns what the pinhole sibling returns, bit for bit;
  2. KannalaBrandt8 PoseOptimization against the numpy restatement pose_kb8 (tests/kb8_scene.py) at sizes around the block and wave tails
     and the 1 280 correspondences a workgroup keeps in registers, robomaster and tum parameters, points out to 80 deg: flags and n_inliers
     identical, pose within the measured tolerance -- 10 x the pose difference that one float32 ulp of theta makes in the restatement itself (the
     optimiser's residual takes theta from atan2f, whose last bit differs between libm and the device), or 1e-6 if that is larger;
  3. KannalaBrandt8 isInFrustum and the projection searches on a 960 x 540 frame against float64 restatements: decisions equal on every
     point the margin rule keeps, u and v within 1e-2 px;
  4. the frame-to-frame search on KannalaBrandt8 queries;
  5. a bad model, a zero focal length and a NULL model are DVM_ERR_INVALID and write nothing.
tests/test_kb8_model.py pins the restatement and the scenes on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import kb8_scene as ks  # noqa: E402
import pose_scene as ps  # noqa: E402

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def pose_tol():
    """10 x the pose difference one float32 ulp of theta makes in the restatement (measured once, about 1.5 s of numpy), or 1e-6 if larger."""
    return max(10 * ks.theta_ulp_pose_diff(), ks.POSE_TOL_FLOOR)
PIN = np.array([520.0, 390.0, 300.0, 250.0], np.float32)          # pose_scene.K_DEFAULT: exact in float32
PIN_WIDE = ks.PINHOLE_WIDE[:4]                                      # a pinhole camera for the 960 x 540 search scenes


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


def _pack(frames, stride):
    B = len(frames)
    poses = np.zeros((B, 7)); Xw = np.full((B, stride, 3), np.nan); obs = np.full((B, stride, 2), np.nan); w = np.full((B, stride), np.nan)
    n = np.zeros(B, np.int32)
    for f, sc in enumerate(frames):
        k = len(sc["Xw"]); n[f] = k
        poses[f] = sc["pose0"]
        Xw[f, :k], obs[f, :k], w[f, :k] = sc["Xw"], sc["obs"], sc["w"]
    return poses, Xw, obs, w, n


def _model(capi, name):
    return capi.CameraModel.make(1, ks.MODELS[name])


# ---- 1. the pinhole guard
@pytest.mark.parametrize("N", [3, 257, 1281])
def test_pinhole_pose_optimize_cam_is_pose_optimize(capi, N):
    sc = ps.scene(0, N)
    a = _pack([sc], N)
    ref = capi.pose_optimize(*a, [float(v) for v in PIN])
    got = capi.pose_optimize_cam(*a, capi.CameraModel.pinhole(*PIN))
    assert np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert N < 10 or ref[1].sum() > 0


def test_pinhole_pose_optimize_cam_ragged_batch(capi):
    frames = [ps.scene(0, n) for n in (3, 257, 1281)]
    a = _pack(frames, 1300)
    ref = capi.pose_optimize(*a, [float(v) for v in PIN])
    got = capi.pose_optimize_cam(*a, capi.CameraModel.pinhole(*PIN))
    assert np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


def _frustum_frame(capi, sc, K=(0.0, 0.0, 0.0, 0.0)):
    F = capi.FrustumFrame()
    F.Rcw = (C.c_float * 9)(*sc["Rcw"].reshape(-1)); F.tcw = (C.c_float * 3)(*sc["t"]); F.Ow = (C.c_float * 3)(*sc["Ow"])
    F.fx, F.fy, F.cx, F.cy = (float(v) for v in K)
    F.min_x, F.max_x, F.min_y, F.max_y = (float(v) for v in ks.BOUNDS)
    F.bf = 40.0; F.log_scale_factor = float(ks.LOG_SF); F.n_levels = ks.N_LEVELS
    return F


def _cam(sc, form, K=None):
    cam = dict(Tcw=sc["Tcw"], Ow=sc["Ow"], bounds=ks.BOUNDS, log_scale_factor=float(ks.LOG_SF), sim3_pair=2 if form == "reloc" else 0)
    if K is not None:
        cam["K"] = K
    return cam


def _pts(sc):
    return dict(pos=sc["pos"], normal=sc["normal"], min_dist=sc["min_dist"], max_dist=sc["max_dist"], desc=sc["desc"])


def test_pinhole_is_in_frustum_cam_is_is_in_frustum(capi):
    sc = ks.search_scene("pinhole", 0, 900, 1900)
    ref = capi.is_in_frustum(_frustum_frame(capi, sc, PIN_WIDE), sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], 0.5)
    got = capi.is_in_frustum_cam(_frustum_frame(capi, sc, (1.0, 2.0, 3.0, 4.0)), capi.CameraModel.pinhole(*PIN_WIDE), sc["pos"], sc["normal"], sc["min_dist"],
                                 sc["max_dist"], 0.5)
    assert ref.tobytes() == got.tobytes() and 50 < ref["in_view"].sum() < 800        # (not an empty comparison)


@pytest.mark.parametrize("form", ks.SEARCH_FORMS)
def test_pinhole_project_search_cam_is_project_search(capi, form):
    sc = ks.search_scene("pinhole", 0, 900, 1900, form == "fuse_sim3")
    g = capi.FrameGrid(2048)
    g.build(sc["kps"], sc["kdesc"], tuple(float(v) for v in ks.BOUNDS))
    gi = ks.INV_SIGMA2 if form == "fuse" else None
    m0, p0 = capi.project_search(g, _cam(sc, form, PIN_WIDE), _pts(sc), ks.SEARCH_TH[form], ks.SCALE, gate_inv_sigma2=gi)
    m1, p1 = capi.project_search_cam(g, _cam(sc, form, (9.0, 9.0, 9.0, 9.0)), capi.CameraModel.pinhole(*PIN_WIDE), _pts(sc), ks.SEARCH_TH[form], ks.SCALE,
                                     gate_inv_sigma2=gi)
    g.close()
    assert m0.tobytes() == m1.tobytes() and p0.tobytes() == p1.tobytes() and (m0["best_idx"] >= 0).sum() > 20


def _frames_args(fs):
    return dict(kps_c=fs["kps"], desc_c=fs["kdesc"], mp_c=np.full(len(fs["kps"]), -1, np.int32), Tcw=fs["Tcw"], bounds=ks.BOUNDS, scale_factors=ks.SCALE,
                kps_l=fs["kps_l"], mp_l=fs["mp_l"], outlier_l=None, mps=fs["mps"])


def test_pinhole_search_by_projection_frames_cam_is_its_sibling(capi):
    fs = ks.frames_scene("pinhole", 0)
    a = _frames_args(fs)
    for ori in (False, True):
        n0, mp0, _ = capi.search_by_projection_frames(K=PIN_WIDE, th=ks.FRAMES_TH, check_ori=ori, **a)
        n1, mp1, _ = capi.search_by_projection_frames_cam(model=capi.CameraModel.pinhole(*PIN_WIDE), th=ks.FRAMES_TH, check_ori=ori, **a)
        assert n0 == n1 and np.array_equal(mp0, mp1)
    assert n0 > 20


# ---- 2. KannalaBrandt8 PoseOptimization
_dev_pose = {}


def _device_pose(capi, model, N):
    if (model, N) not in _dev_pose:
        sc, ref, _ = ks.pose_scene(model, N)
        pg, og, ng = capi.pose_optimize_cam(*_pack([sc], N), _model(capi, model))
        _dev_pose[(model, N)] = (pg[0], og[0], int(ng[0]))
    return _dev_pose[(model, N)]


@pytest.mark.parametrize("model,N", ks.pose_cases())
def test_kb8_pose_optimize(capi, pose_tol, model, N):
    sc, (T, outl, nin, info, _), _ = ks.pose_scene(model, N)
    pg, og, ng = _device_pose(capi, model, N)
    d = float(np.abs(pg - T).max())
    print(f"{model} N={N}: |pose - restatement| {d:.3e} (tolerance {pose_tol:.3e}), {int(og.sum())} flagged")
    assert ng == nin and np.array_equal(og, outl)
    assert d < pose_tol
    assert abs(np.linalg.norm(pg[3:]) - 1) < 1e-12 and pg[6] >= 0


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_kb8_pose_optimize_ragged_batch_equals_single_calls(capi, model):
    frames = [ks.pose_scene(model, n)[0] for n in ks.POSE_RAGGED]
    pg, og, ng = capi.pose_optimize_cam(*_pack(frames, ks.REG_KB8 + 20), _model(capi, model))
    for f, n in enumerate(ks.POSE_RAGGED):
        p1, o1, n1 = _device_pose(capi, model, n)
        assert np.array_equal(_bits(pg[f]), _bits(p1)) and np.array_equal(og[f, :n], o1) and int(ng[f]) == n1


# ---- 3. KannalaBrandt8 isInFrustum and projection searches
@pytest.mark.parametrize("model", list(ks.MODELS))
@pytest.mark.parametrize("n_pts", ks.PT_COUNTS)
def test_kb8_is_in_frustum(capi, model, n_pts):
    sc = ks.search_scene(model, 0, n_pts, ks.KP_COUNTS[-1])
    ref = ks.frustum_ref(sc)
    got = capi.is_in_frustum_cam(_frustum_frame(capi, sc), _model(capi, model), sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], 0.5)
    keep = ~ref["drop"]
    assert keep.sum() >= (1 - ks.DROP_MAX) * n_pts
    assert np.array_equal(got["in_view"][keep], ref["in_view"][keep]) and np.array_equal(got["level"][keep], ref["level"][keep])
    vis = keep & (ref["in_view"] == 1)
    assert vis.any()
    d = max(np.abs(got["proj_x"][vis] - ref["uv"][vis, 0]).max(), np.abs(got["proj_y"][vis] - ref["uv"][vis, 1]).max())
    print(f"{model} {n_pts} points: {int(vis.sum())} in view, largest |uv - restatement| {d:.3e} px")
    assert d < ks.PX_MARGIN
    assert np.abs(got["depth"][vis] - ref["depth"][vis]).max() < 1e-4 and np.abs(got["view_cos"][vis] - ref["view_cos"][vis]).max() < 1e-5


@pytest.mark.parametrize("model,seed,n_pts,n_kp,form", ks.search_cases())
def test_kb8_project_search(capi, model, seed, n_pts, n_kp, form):
    sc = ks.search_scene(model, seed, n_pts, n_kp, form == "fuse_sim3")
    ref = ks.project_search_ref(sc, form, ks.SEARCH_TH[form])
    g = capi.FrameGrid(2048)
    g.build(sc["kps"], sc["kdesc"], tuple(float(v) for v in ks.BOUNDS))
    m, pr = capi.project_search_cam(g, _cam(sc, form), _model(capi, model), _pts(sc), ks.SEARCH_TH[form], ks.SCALE,
                                    gate_inv_sigma2=ks.INV_SIGMA2 if form == "fuse" else None)
    g.close()
    keep = ~ref["drop"]
    assert keep.sum() >= (1 - ks.DROP_MAX) * n_pts
    assert np.array_equal(pr["level"][keep], ref["level"][keep])
    assert np.array_equal(m["best_idx"][keep], ref["best_idx"][keep]) and np.array_equal(m["best_dist"][keep], ref["best_dist"][keep])
    vis = keep & (ref["level"] >= 0)
    assert vis.any()
    d = max(np.abs(pr["u"][vis] - ref["uv"][vis, 0]).max(), np.abs(pr["v"][vis] - ref["uv"][vis, 1]).max())
    print(f"{model} {form} {n_pts} points, {n_kp} keypoints: {int(vis.sum())} searched, {int((m['best_idx'][keep] >= 0).sum())} found, "
          f"largest |uv - restatement| {d:.3e} px")
    assert d < ks.PX_MARGIN
    assert np.array_equal(pr["radius"][vis], ref["radius"][vis].astype(np.float32))


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_kb8_project_search_sim3_pair_keeps_the_inline_pinhole_formula(capi, model):
    """cam.sim3_pair == 1 (SearchBySim3): the reference writes u = fx * (X * invz) + cx inline whatever the camera (ORBmatcher.cc:1401-1406),
    so the KannalaBrandt8 entry returns what dvm_project_search returns on the model's four pinhole floats, bit for bit."""
    sc = ks.search_scene("pinhole", 0, 900, 1900)
    p = ks.MODELS[model]
    S2 = np.r_[np.sqrt(1.1) * np.array([0.02, -0.01, 0.03, 1.0]) / np.linalg.norm([0.02, -0.01, 0.03, 1.0]), 0.05, -0.02, 0.1].astype(np.float32)
    g = capi.FrameGrid(2048)
    g.build(sc["kps"], sc["kdesc"], tuple(float(v) for v in ks.BOUNDS))
    cam = dict(_cam(sc, "fuse", p[:4]), sim3_pair=1, S2=S2)
    m0, p0 = capi.project_search(g, cam, _pts(sc), 7.5, ks.SCALE)
    m1, p1 = capi.project_search_cam(g, dict(cam, K=(9.0, 9.0, 9.0, 9.0)), _model(capi, model), _pts(sc), 7.5, ks.SCALE)
    g.close()
    assert m0.tobytes() == m1.tobytes() and p0.tobytes() == p1.tobytes() and (p0["level"] >= 0).sum() > 20


# ---- 4. the frame-to-frame search
@pytest.mark.parametrize("model", list(ks.MODELS))
def test_kb8_search_by_projection_frames(capi, model):
    fs = ks.frames_scene(model, 0)
    nm, mp, nq, frag = ks.frames_ref(fs, ks.FRAMES_TH)
    assert not frag.any()
    n, got, _ = capi.search_by_projection_frames_cam(model=_model(capi, model), th=ks.FRAMES_TH, check_ori=False, **_frames_args(fs))
    assert n == nm and np.array_equal(got, mp) and nm > 150


# ---- 5. errors
def test_bad_models_are_invalid_and_write_nothing(capi):
    L, H = capi.lib(), capi.host_lib()
    bad = [capi.CameraModel.make(2, ks.ROBOMASTER), capi.CameraModel.make(-1, ks.ROBOMASTER),
           capi.CameraModel.make(1, np.r_[0.0, ks.ROBOMASTER[1:]]), capi.CameraModel.make(0, np.r_[ks.ROBOMASTER[:1], 0.0, ks.ROBOMASTER[2:]]), None]
    sc, _, _ = ks.pose_scene("robomaster", 64)
    poses, Xw, obs, w, n = _pack([sc], 64)
    ss = ks.search_scene("robomaster", 0, 17, 65)
    fs = ks.frames_scene("robomaster", 0)
    g = capi.FrameGrid(2048)
    g.build(ss["kps"], ss["kdesc"], tuple(float(v) for v in ks.BOUNDS))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    F = _frustum_frame(capi, ss)

    class _Cam(C.Structure):
        _fields_ = [("Tcw", C.c_float * 7), ("Ow", C.c_float * 3), ("K", C.c_float * 4), ("b", C.c_float * 4), ("lsf", C.c_float), ("nl", C.c_int32),
                    ("sim3_pair", C.c_int32), ("S2", C.c_float * 7)]
    kc = _Cam(); kc.Tcw = (C.c_float * 7)(*ss["Tcw"]); kc.Ow = (C.c_float * 3)(*ss["Ow"]); kc.b = (C.c_float * 4)(*ks.BOUNDS); kc.lsf = float(ks.LOG_SF); kc.nl = ks.N_LEVELS
    for fn in (L.dvm_pose_optimize_cam, L.dvm_is_in_frustum_cam, L.dvm_project_search_cam, H.dvmh_search_by_projection_frames_cam):
        fn.restype = C.c_int32; fn.argtypes = None
    for mdl in bad:
        ref = None if mdl is None else C.byref(mdl)
        out = np.full((1, 7), 7.5); outl = np.full((1, 64), 0xAB, np.uint8); nin = np.full(1, -77, np.int32)
        assert L.dvm_pose_optimize_cam(C.c_int32(0), vp(poses), vp(Xw), vp(obs), vp(w), vp(n), C.c_int32(64), C.c_int32(1), ref, vp(out), vp(outl), vp(nin)) == -1
        assert np.all(out == 7.5) and np.all(outl == 0xAB) and nin[0] == -77
        tp = np.full(17 * 28, 0xAB, np.uint8)
        assert L.dvm_is_in_frustum_cam(C.byref(F), ref, vp(ss["pos"]), vp(ss["normal"]), vp(ss["min_dist"]), vp(ss["max_dist"]), C.c_int32(17), C.c_float(0.5),
                                       vp(tp), C.c_int32(0), None) == -1
        assert np.all(tp == 0xAB)
        mo = np.full(17 * 16, 0xAB, np.uint8); pr = np.full(17 * 16, 0xAB, np.uint8)
        assert L.dvm_project_search_cam(g.h, C.c_int32(0), None, C.byref(kc), ref, vp(ss["pos"]), vp(ss["normal"]), vp(ss["min_dist"]), vp(ss["max_dist"]),
                                        vp(ss["desc"]), None, C.c_int32(17), C.c_float(4.0), vp(ks.SCALE), None, C.c_double(5.99), vp(mo), vp(pr),
                                        C.c_int32(0), None) == -1
        assert np.all(mo == 0xAB) and np.all(pr == 0xAB)
        mp = np.full(len(fs["kps"]), -5, np.int32); rq = C.c_int32(-9)
        a = _frames_args(fs)
        assert H.dvmh_search_by_projection_frames_cam(C.c_int32(0), C.c_int32(len(fs["kps"])), vp(a["kps_c"]), vp(a["desc_c"]), vp(mp), vp(a["Tcw"]), ref,
                                                      vp(ks.BOUNDS), vp(ks.SCALE), C.c_int32(ks.N_LEVELS), C.c_int32(len(a["kps_l"])), vp(a["kps_l"]),
                                                      vp(a["mp_l"]), None, vp(a["mps"]), C.c_float(15.0), C.c_int32(0), C.byref(rq)) == -1
        assert np.all(mp == -5) and rq.value == -9
    g.close()
