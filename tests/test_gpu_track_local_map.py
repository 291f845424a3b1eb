"""dvm_track_local_map (Tracker.track_local_map): Tracking::TrackLocalMap (src/Tracking.cc:2668-2740) of the frame the first half just
tracked, as ONE device chain -- SearchLocalPoints (:3041-3106) -> SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints)
(src/ORBmatcher.cc:44-205) -> PoseOptimization seeded from the first half's float pose (src/Optimizer.cc:744-1028) -> mnMatchesInliers.
Checked against (a) the reference-ordered composition of the separate calls of this library (dvm_is_in_frustum +
dvmh_search_by_projection_points + dvm_pose_optimize), bit for bit, and (b) the same composition over the CPU oracle (assignments and flags
identical, pose within 1e-6)."""
import ctypes as C

import numpy as np
import pytest

import pixel_scene as ps

pytestmark = pytest.mark.gpu

BOUNDS = np.array([0, 640, 0, 480], np.float32)
KC = np.array([500.0, 500.0, 320.0, 240.0], np.float32)


def _tcw7f(p):   # (t, q) doubles -> dvm_se3f (q, t) floats
    return np.concatenate([p[3:7], p[0:3]]).astype(np.float32)


def _local_points(capi, kps, desc, X, Ow, scale, rng, p_obs0=0.15, p_bad=0.03):
    """dvm_local_point records of points X [n, 3] seen from camera centre Ow by keypoints kps: GetNormal = the viewing direction,
    mfMaxDistance = dist * scale[octave], mfMinDistance = mfMaxDistance / scale[nlevels - 1] (MapPoint::UpdateNormalAndDepth)."""
    n = len(kps)
    pts = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    pts["pos"] = X.astype(np.float32)
    v = X - Ow[None, :]
    d = np.linalg.norm(v, axis=1)
    pts["normal"] = (v / d[:, None]).astype(np.float32)
    dmax = (d * scale[kps["octave"]]).astype(np.float32)
    pts["max_dist"] = dmax
    pts["min_dist"] = (dmax / scale[-1]).astype(np.float32)
    pts["desc"] = desc
    pts["n_obs"] = np.where(rng.random(n) < p_obs0, 0, 1 + rng.integers(0, 4, n))
    pts["bad"] = (rng.random(n) < p_bad).astype(np.int32)
    return pts


def _mps(capi, pts):
    mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
    mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
    return mps


def _frustum(mod, Tcw, K, bounds, scale, matrices):
    R, t, Ow = matrices(Tcw)
    F = mod.FrustumFrame()
    F.Rcw[:] = [float(v) for v in np.asarray(R, np.float32).reshape(-1)]
    F.tcw[:] = [float(v) for v in t]
    F.Ow[:] = [float(v) for v in Ow]
    F.fx, F.fy, F.cx, F.cy = (float(np.float32(v)) for v in K)
    F.min_x, F.max_x, F.min_y, F.max_y = (float(v) for v in bounds)
    F.bf = 0.0
    F.log_scale_factor = float(np.float32(np.log(np.float64(scale[1]))))    # Frame::mfLogScaleFactor = log(mfScaleFactor)
    F.n_levels = len(scale)
    return F


def _separate(mod, kps_un, desc, frame_mp, pts, Tcw, K, bounds, scale, inv_s2, th, far, th_far):
    """TrackLocalMap in the reference's order over the separate calls of `mod` (capi or the oracle): SearchLocalPoints -> SearchByProjection
    -> PoseOptimization (seeded from the float pose widened to double) -> mnMatchesInliers."""
    gpu = hasattr(mod, "Tracker")
    n = len(pts)
    mp = np.array(frame_mp, np.int32, copy=True)
    bad = pts["bad"] != 0
    held = mp >= 0
    cleared = held & bad[np.maximum(mp, 0)] if n else np.zeros(len(mp), bool)
    mp[cleared] = -1
    seen = np.zeros(n, bool)
    seen[mp[mp >= 0]] = True
    F = _frustum(mod, Tcw, K, bounds, scale, mod.pose_matrices)
    if n:
        tp = mod.is_in_frustum(F, pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], 0.5)
    else:
        tp = np.zeros(0, mod.TRACK_DTYPE)
    tp["in_view"][seen | bad] = 0
    tpts = np.zeros(n, mod.TRACKED_POINT_DTYPE)
    for f in ("proj_x", "proj_y", "depth", "view_cos", "level"):
        tpts[f] = tp[f]
    tpts["in_view"] = tp["in_view"] != 0
    tpts["bad"] = bad
    tpts["desc"], tpts["n_obs"] = pts["desc"], pts["n_obs"]
    claimed = ((mp >= 0) & (pts["n_obs"][np.maximum(mp, 0)] > 0)).astype(np.uint8) if n else np.zeros(len(mp), np.uint8)
    if gpu:
        nm, mp2, _ = mod.search_by_projection_points(kps_un, desc, mp, claimed, bounds, scale, tpts, th, 0.8, far, th_far)
    else:
        nm, mp2 = mod.search_by_projection_points(kps_un, desc, mp, claimed, bounds, scale, tpts, th, 0.8, far, th_far)
    sel = np.flatnonzero(mp2 >= 0)
    Xw = pts["pos"][mp2[sel]].astype(np.float64).reshape(-1, 3)
    obs = np.column_stack([kps_un["x"][sel], kps_un["y"][sel]]).astype(np.float64).reshape(-1, 2)
    w = inv_s2[kps_un["octave"][sel]].astype(np.float64)
    pose_in = np.concatenate([Tcw[4:7], Tcw[0:4]]).astype(np.float64)
    if gpu:
        S = max(len(sel), 1)
        Xp = np.zeros((S, 3)); Op = np.zeros((S, 2)); Wp = np.zeros(S)
        Xp[:len(sel)], Op[:len(sel)], Wp[:len(sel)] = Xw, obs, w
        p, o, ni = mod.pose_optimize(pose_in[None], Xp[None], Op[None], Wp[None], [len(sel)], K)
        pose, outl, nin = p[0], o[0][:len(sel)], int(ni[0])
    else:
        pose, outl, nin = mod.pose_optimize(pose_in, Xw, obs, w, K)
        outl = np.asarray(outl)[:len(sel)]
    outlier = np.zeros(len(mp2), np.uint8)
    outlier[sel] = outl != 0
    keep = sel[outl == 0]
    return dict(track_pts=tp, n_to_match=int(tp["in_view"].sum()), nmatches=int(nm), mp=mp2, outlier=outlier, n_edges=len(sel),
                n_inliers=int(nin), matches_inliers=int((pts["n_obs"][mp2[keep]] > 0).sum()), pose=np.asarray(pose, np.float64),
                n_cleared_bad=int(cleared.sum()))


def _check(a, b, exact):
    for k in ("n_to_match", "nmatches", "n_edges", "n_inliers", "matches_inliers", "n_cleared_bad"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert np.array_equal(a["mp"], b["mp"]), int((a["mp"] != b["mp"]).sum())
    assert np.array_equal(a["outlier"], b["outlier"]), int((a["outlier"] != b["outlier"]).sum())
    if "track_pts" in a:
        for f in ("proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level", "in_view"):
            assert np.array_equal(a["track_pts"][f], b["track_pts"][f]), f
    if exact:
        assert np.array_equal(a["pose"], b["pose"]), (a["pose"], b["pose"])
    else:
        assert np.abs(a["pose"] - b["pose"]).max() < 1e-6, (a["pose"], b["pose"])


def _run_both(capi, po, trk, first, pts, scale, inv_s2, th, far, th_far, K=None, bounds=None, oracle=True):
    K = ps.K.astype(np.float32) if K is None else K
    bounds = BOUNDS if bounds is None else bounds
    fused = trk.track_local_map(pts, first["mp"], th=th, far_points=far, th_far=th_far, want_track_points=True)
    sep = _separate(capi, first["kps_un"], first["desc"], first["mp"], pts, first["Tcw"], K, bounds, scale, inv_s2, th, far, th_far)
    _check(fused, sep, exact=True)
    if oracle:
        orc = _separate(po, first["kps_un"], first["desc"], first["mp"], pts, first["Tcw"], K, bounds, scale, inv_s2, th, far, th_far)
        _check(fused, orc, exact=False)
    return fused


@pytest.fixture(scope="module")
def scene():
    frames, poses = ps.render(12)
    return frames, poses


def _scene_table(capi, ext, frames, poses, scale, rng, ids=(0, 1, 2)):
    """The local map: the back-projected keypoints of frames `ids` (frame ids[0]'s first, so that its points are table entries 0..n0-1)."""
    tabs, first = [], None
    for f in ids:
        n, k, d, _ = ext.extract(frames[f])
        R, t = poses[f]
        X = ps.backproject(k, R, t) + rng.normal(0, 0.01, (n, 3))
        tabs.append(_local_points(capi, k, d, X, -R.T @ t, scale, rng))
        if first is None:
            first = (k.copy(), n)
    return np.concatenate(tabs), first


@pytest.mark.parametrize("th,far", [(1.0, False), (5.0, False), (15.0, False), (1.0, True), (5.0, True)])
def test_local_map_equals_separate_calls_and_oracle(scene, th, far):
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(5)
    pts, (k0, n0) = _scene_table(capi, ext, frames, poses, scale, rng)
    assert 2500 < len(pts) < 4000 and (pts["n_obs"] == 0).any() and pts["bad"].any()
    th_far = float(np.median(np.linalg.norm(pts["pos"], axis=1))) if far else 0.0
    trk = capi.Tracker(ext)
    trk.reserve_local_map(len(pts))
    mps = _mps(capi, pts)
    kps_l, mp_l, outl_l = k0, np.arange(n0, dtype=np.int32), None
    counts = []
    for t in (1, 2, 3):
        Tcw_pred = _tcw7f(ps.pose7(*poses[t - 1]))
        first = trk.track(frames[t], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, kps_l, mp_l, outl_l, mps, th=15.0)
        assert first["tracked"]
        fused = _run_both(capi, po, trk, first, pts, scale, inv_s2, th, far, th_far)
        new = int(((fused["mp"] >= 0) & (fused["mp"] != first["mp"])).sum())
        counts.append(new)
        kps_l, mp_l, outl_l = first["kps_un"], fused["mp"], fused["outlier"]
    assert min(counts) > 0 and max(counts) > 100, counts      # a real search, not a degenerate one
    trk.close(); ext.close()


def test_local_map_dense_stream_requeries_on_device():
    """Dense bench stream, th = 15, the local map from the three previous frames: some query finds fewer than two of its four ranked
    candidates free and the device searches its window again; results equal the separate calls."""
    from dvm_slam_amd import capi, synth
    from oracle import pyoracle as po
    frames = synth.frame_stream(7)
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    trk = capi.Tracker(ext)
    trk.reserve_local_map(4096)
    rng = np.random.default_rng(9)
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    total_rq, total_nm, ran = 0, 0, 0
    for t in (3, 4, 5, 6):
        tabs, last = [], None
        for f in (t - 3, t - 2, t - 1):
            n0, k0, d0, _ = ext.extract(frames[f])
            z = rng.uniform(3, 9, n0)
            X = np.column_stack([(k0["x"] - KC[2]) / KC[0] * z, (k0["y"] - KC[3]) / KC[1] * z, z])
            tabs.append(_local_points(capi, k0, d0, X, np.zeros(3), scale, rng, p_obs0=0.1, p_bad=0.0))
            last = (k0.copy(), sum(len(x) for x in tabs[:-1]), n0)
        pts = np.concatenate(tabs)
        k0, off, n0 = last
        first = trk.track(frames[t], Tcw, KC, BOUNDS, scale, inv_s2, k0, np.arange(off, off + n0, dtype=np.int32), None, _mps(capi, pts), th=15.0)
        if not first["tracked"]:
            continue
        fused = _run_both(capi, po, trk, first, pts, scale, inv_s2, 15.0, False, 0.0, K=KC, oracle=(t == 3))
        total_rq += fused["n_requeried"]
        total_nm += fused["nmatches"]
        ran += 1
    assert ran >= 2 and total_rq > 0 and total_nm > 0, (ran, total_rq, total_nm)
    trk.close(); ext.close()


def test_local_map_distorted_camera(scene):
    """k1 != 0: the second half runs on the first half's device-undistorted mvKeysUn (equal to the separate calls on kps_un)."""
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    cam = np.array([500.0, 500.0, 320.0, 240.0, -0.04, 0.01, 0.0005, -0.0003, 0.0], np.float32)
    dist = capi.Distortion(*[float(v) for v in cam])
    bounds = capi.image_bounds(cam, 640, 480)
    rng = np.random.default_rng(11)
    pts, (k0, n0) = _scene_table(capi, ext, frames, poses, scale, rng)
    trk = capi.Tracker(ext)
    trk.reserve_local_map(len(pts))
    first = trk.track(frames[1], _tcw7f(ps.pose7(*poses[0])), ps.K, bounds, scale, inv_s2, k0, np.arange(n0, dtype=np.int32), None, _mps(capi, pts),
                      th=15.0, dist=dist)
    assert first["tracked"]
    assert not np.array_equal(first["kps_un"]["x"], first["kps"]["x"])      # the distortion did move the keypoints
    fused = _run_both(capi, po, trk, first, pts, scale, inv_s2, 1.0, False, 0.0, bounds=bounds)
    assert fused["nmatches"] > 0
    trk.close(); ext.close()


def test_local_map_edges(scene):
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(13)
    pts, (k0, n0) = _scene_table(capi, ext, frames, poses, scale, rng)
    pts["bad"] = 0
    mps = _mps(capi, pts)
    trk = capi.Tracker(ext)
    # no reservation / no tracked frame yet: call sequence errors
    with pytest.raises(capi.DvmError) as e:
        trk.track_local_map(pts[:10], np.zeros(0, np.int32))
    assert e.value.code == -6          # DVM_ERR_STATE
    trk.reserve_local_map(16384)
    Tcw_pred = _tcw7f(ps.pose7(*poses[0]))

    def first_half():
        f = trk.track(frames[1], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, k0, np.arange(n0, dtype=np.int32), None, mps, th=15.0)
        assert f["tracked"]
        return f

    # an empty table (the frame holds nothing): no query, no edge, the pose stays the widened float pose
    f = first_half()
    empty = _run_both(capi, po, trk, dict(f, mp=np.full(len(f["mp"]), -1, np.int32)), pts[:0], scale, inv_s2, 1.0, False, 0.0)
    assert empty["nmatches"] == 0 and empty["n_edges"] == 0 and empty["n_inliers"] == 0
    assert np.array_equal(empty["pose"], np.concatenate([f["Tcw"][4:7], f["Tcw"][0:4]]).astype(np.float64))
    # a second call after one finish: refused
    with pytest.raises(capi.DvmError) as e:
        trk.track_local_map(pts[:0], np.full(len(f["mp"]), -1, np.int32))
    assert e.value.code == -6
    # every in-view point already held by the frame: nothing to match
    f = first_half()
    held = np.unique(f["mp"][f["mp"] >= 0])
    remap = np.full(len(pts), -1, np.int32); remap[held] = np.arange(len(held))
    sub = pts[held]
    fm = np.where(f["mp"] >= 0, remap[np.maximum(f["mp"], 0)], -1).astype(np.int32)
    r = _run_both(capi, po, trk, dict(f, mp=fm), sub, scale, inv_s2, 5.0, False, 0.0)
    assert r["n_to_match"] == 0 and r["nmatches"] == 0 and r["n_edges"] == int((fm >= 0).sum())
    # the frame holds bad points: cleared and counted
    f = first_half()
    pb = pts.copy()
    hb = np.unique(f["mp"][f["mp"] >= 0])[::7]
    pb["bad"][hb] = 1
    r = _run_both(capi, po, trk, f, pb, scale, inv_s2, 1.0, False, 0.0)
    assert r["n_cleared_bad"] == int(np.isin(f["mp"], hb).sum()) > 0
    # a 12 000-point table (beyond a frame slot's keypoint cap): the original points and perturbed copies
    f = first_half()
    big = np.concatenate([pts] + [pts] * 3)[:12000].copy()
    big["pos"][len(pts):] += rng.normal(0, 0.02, (12000 - len(pts), 3)).astype(np.float32)
    big["n_obs"][len(pts):] = rng.integers(0, 3, 12000 - len(pts))
    r = _run_both(capi, po, trk, f, big, scale, inv_s2, 5.0, False, 0.0, oracle=False)
    assert r["n_to_match"] > 4000 and r["nmatches"] > 0
    # more points than reserved: DVM_ERR_CAPACITY; the frame is still there for a call that fits
    f = first_half()
    huge = np.concatenate([pts] * 6)[:16385]
    with pytest.raises(capi.DvmError) as e:
        trk.track_local_map(huge, f["mp"])
    assert e.value.code == -3          # DVM_ERR_CAPACITY
    _run_both(capi, po, trk, f, pts, scale, inv_s2, 1.0, False, 0.0, oracle=False)
    # after a new begin (no finish): DVM_ERR_STATE
    first_half()
    img = np.ascontiguousarray(frames[2])
    L = capi.lib()
    L.dvm_track_begin.restype = C.c_int32
    L.dvm_track_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    capi.check(L.dvm_track_begin(trk.t, ext.h, img.ctypes.data, 480, 640, img.strides[0], 0, 1000))
    with pytest.raises(capi.DvmError) as e:
        trk.track_local_map(pts, np.full(len(f["mp"]), -1, np.int32))
    assert e.value.code == -6
    ext.sync()
    trk.close(); ext.close()


def test_local_map_reservations_release_their_memory(scene):
    import torch
    from dvm_slam_amd import capi
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(17)
    pts, (k0, n0) = _scene_table(capi, ext, frames, poses, scale, rng)
    mps = _mps(capi, pts)
    Tcw_pred = _tcw7f(ps.pose7(*poses[0]))

    def cycle():
        trk = capi.Tracker(ext)
        trk.reserve_local_map(16384)
        trk.reserve_local_map(len(pts))          # a second reservation replaces the first
        f = trk.track(frames[1], Tcw_pred, ps.K, BOUNDS, scale, inv_s2, k0, np.arange(n0, dtype=np.int32), None, mps, th=15.0)
        trk.track_local_map(pts, f["mp"])
        trk.close()

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free
    cycle(); cycle()
    base = used()
    for _ in range(20):
        cycle()
    grown = used() - base
    assert grown <= 8 << 20, f"{grown / 2**20:.1f} MiB of device memory not returned after 20 tracker reservations"
    ext.close()


def test_ten_chained_frames_equal_separate_calls(scene):
    """Each frame's two halves feed the next frame's LastFrame (mvpMapPoints with the outliers TrackLocalMap keeps, mvbOutlier): the
    fused loop's trajectory and assignments equal those of the same loop over the separate calls, bit for bit."""
    from dvm_slam_amd import capi
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(23)
    pts, (k0, n0) = _scene_table(capi, ext, frames, poses, scale, rng, ids=(0, 2, 4, 6, 8))
    pts["bad"] = 0
    mps = _mps(capi, pts)
    K = ps.K.astype(np.float32)
    trk = capi.Tracker(ext)
    trk.reserve_local_map(len(pts))
    state = {m: (k0, np.arange(n0, dtype=np.int32), None, _tcw7f(ps.pose7(*poses[0]))) for m in ("fused", "separate")}
    for t in range(1, 11):
        for mode in ("fused", "separate"):
            kl, ml, ol, T = state[mode]
            first = trk.track(frames[t], T, ps.K, BOUNDS, scale, inv_s2, kl, ml, ol, mps, th=15.0)
            if mode == "fused":
                r = trk.track_local_map(pts, first["mp"], th=1.0)
            else:
                r = _separate(capi, first["kps_un"], first["desc"], first["mp"], pts, first["Tcw"], K, BOUNDS, scale, inv_s2, 1.0, False, 0.0)
            Tn = np.concatenate([r["pose"][3:7], r["pose"][0:3]]).astype(np.float32)
            state[mode] = (first["kps_un"].copy(), r["mp"].copy(), r["outlier"].copy(), Tn)
        a, b = state["fused"], state["separate"]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), t
    gt = ps.pose7(*poses[10])
    assert np.abs(state["fused"][3][4:7] - gt[:3]).max() < 0.05          # and it follows the camera
    trk.close(); ext.close()
