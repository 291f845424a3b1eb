"""dvm_track_reference_keyframe (Tracker.track_reference_keyframe): Tracking::TrackReferenceKeyFrame (src/Tracking.cc:2461-2520) as ONE device
chain -- Frame::ComputeBoW -> ORBmatcher(0.7, true).SearchByBoW(mpReferenceKF, F) (src/ORBmatcher.cc:214-393) -> PoseOptimization seeded
from mLastFrame's pose -> the outlier drop and nmatchesMap.  Checked against (a) the composition of this library's separate calls
(dvm_orb_extract + dvmh_vocab_transform + dvmh_search_by_bow_kf_frame + dvm_pose_optimize), bit for bit, and (b) the same composition
over the CPU oracle (assignments and flags identical, pose within 1e-6).  Scenes: pixel_scene frames, keyframe = an earlier frame, its map
points back-projected."""
import ctypes as C

import numpy as np
import pytest

import pixel_scene as ps

pytestmark = pytest.mark.gpu

BOUNDS = np.array([0, 640, 0, 480], np.float32)
LEVELSUP = 4
MP_BASE = 0            # the keyframe's map-point ids: table index = id - MP_BASE


def _tcw7f(p):   # (t, q) doubles -> dvm_se3f (q, t) floats
    return np.concatenate([p[3:7], p[0:3]]).astype(np.float32)


def _widen(T):   # dvm_se3f (q, t) floats -> PoseOptimization's seed (t, q) doubles
    T = np.asarray(T, np.float32)
    return np.concatenate([T[4:7], T[0:4]]).astype(np.float64)


def _local_points(capi, kps, desc, X, Ow, scale, rng, p_obs0=0.15, p_bad=0.03):
    """dvm_local_point records of points X [n, 3] seen from camera centre Ow by keypoints kps (MapPoint::UpdateNormalAndDepth)."""
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


@pytest.fixture(scope="module")
def scene():
    return ps.render(8)


@pytest.fixture(scope="module")
def world(scene):
    """The extractor's tables, the keyframe (frame 0: its keypoints, descriptors and back-projected map points = local-map table entries
    0..n0-1, a few -1 holes), the local map (frames 0 and 2) and a k = 10, L = 6 vocabulary whose node descriptors are the scene's own."""
    from dvm_slam_amd import capi, synth
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(31)
    tabs, descs = [], []
    kf = None
    for f in (0, 2):
        n, k, d, _ = ext.extract(frames[f])
        R, t = poses[f]
        X = ps.backproject(k, R, t) + rng.normal(0, 0.01, (n, 3))
        tabs.append(_local_points(capi, k, d, X, -R.T @ t, scale, rng))
        descs.append(d.copy())
        if kf is None:
            kf = (k.copy(), d.copy())
    pts = np.concatenate(tabs)
    ext.close()
    voc = synth.vocabulary(k=10, L=6, ragged=False, seed=5)
    pool = np.concatenate(descs)
    voc["desc"] = pool[rng.integers(0, len(pool), voc["n_nodes"])]
    k0, d0 = kf
    n0 = len(k0)
    mp = (np.arange(n0) + MP_BASE).astype(np.int32)
    mp[rng.random(n0) < 0.05] = -1
    return dict(scale=scale, inv_s2=inv_s2, pts=pts, voc=voc, kps=k0, desc=d0, mp=mp)


def _kf(capi, w, voc, mp=None, pts=None, desc=None, levelsup=LEVELSUP):
    """dvm_ref_keyframe as a dict: map-point fields looked up in the table by id, mFeatVec from the host transform of its descriptors."""
    pts = w["pts"] if pts is None else pts
    mp = w["mp"] if mp is None else mp
    desc = w["desc"] if desc is None else desc
    ix = np.maximum(mp - MP_BASE, 0)
    fv = capi.vocab_transform_host(voc, desc, levelsup)
    return dict(kps=w["kps"], desc=desc, mp=np.ascontiguousarray(mp, np.int32), pos=pts["pos"][ix], n_obs=pts["n_obs"][ix].astype(np.int32),
                bad=pts["bad"][ix].astype(np.uint8), fv=fv)


def _separate_gpu(capi, kf, kps_un, desc, fv_f, pose_last, inv_s2, check_ori=True):
    """SearchByBoW -> PoseOptimization -> the outlier drop over this library's separate calls."""
    KFv = capi.keyframe_view(dict(kps=kf["kps"], desc=kf["desc"], mp=kf["mp"].copy(), bad=kf["bad"], fv=kf["fv"], bounds=BOUNDS))
    F = capi.frame_view(kps_un, desc, BOUNDS, np.ones(8, np.float32))
    nm, m, _ = capi.search_by_bow_kf_frame(KFv, F, fv_f, 0.7, check_ori)
    nb, _, _ = capi.search_by_bow_kf_frame(KFv, F, fv_f, 0.7, False)       # the matches before the rotation check
    return nm, nb, m


def _pose_and_drop(opt, kf, kps_un, m, pose_last, inv_s2, gpu):
    id_to_kf = {int(i): k for k, i in enumerate(kf["mp"]) if i >= 0}
    sel = np.flatnonzero(m >= 0)
    src = np.array([id_to_kf[int(i)] for i in m[sel]], np.int64)
    Xw = kf["pos"][src].astype(np.float64).reshape(-1, 3)
    obs = np.column_stack([kps_un["x"][sel], kps_un["y"][sel]]).astype(np.float64).reshape(-1, 2)
    wgt = inv_s2[kps_un["octave"][sel]].astype(np.float64)
    pose_in = _widen(pose_last)
    if gpu:
        S = max(len(sel), 1)
        Xp = np.zeros((S, 3)); Op = np.zeros((S, 2)); Wp = np.zeros(S)
        Xp[:len(sel)], Op[:len(sel)], Wp[:len(sel)] = Xw, obs, wgt
        p, o, ni = opt.pose_optimize(pose_in[None], Xp[None], Op[None], Wp[None], [len(sel)], ps.K)
        pose, outl, nin = p[0], o[0][:len(sel)], int(ni[0])
    else:
        pose, outl, nin = opt.pose_optimize(pose_in, Xw, obs, wgt, ps.K)
        outl = np.asarray(outl)[:len(sel)]
    outlier = np.zeros(len(m), np.uint8)
    outlier[sel] = outl != 0
    mp_out = np.where(outlier != 0, -1, m).astype(np.int32)
    dropped = np.where(outlier != 0, m, -1).astype(np.int32)
    keep = sel[outl == 0]
    nmap = int((kf["n_obs"][src[outl == 0]] > 0).sum())
    return dict(pose=np.asarray(pose, np.float64), outlier=outlier, mp=mp_out, dropped=dropped, n_edges=len(sel), n_inliers=nin,
                nmatches_map=nmap, nmatches_after=len(sel) - int((outl != 0).sum()), n_keep=len(keep))


def _check_against_separate(capi, po, r, kf, voc, desc, kps_un, pose_last, inv_s2, oracle=True, check_ori=True, levelsup=LEVELSUP):
    """r: the chain's result.  Bit for bit against the library's calls; against the oracle: assignments and flags, pose within 1e-6."""
    host = capi.vocab_transform_host(voc, desc, levelsup)
    assert np.array_equal(r["bow_ids"], host["bow_ids"]) and np.array_equal(r["bow_vals"], host["bow_vals"])
    for k in ("fv_nodes", "fv_off", "fv_feat"):
        assert np.array_equal(r[k], host[k]), k
    assert r["n_bow"] == len(host["bow_ids"]) and r["n_fv"] == len(host["fv_nodes"])
    nm, nb, m = _separate_gpu(capi, kf, kps_un, desc, host, pose_last, inv_s2, check_ori)
    assert r["nmatches"] == nm and r["nmatches_before_rotation"] == (nb if check_ori else nm), (r["nmatches"], nm, r["nmatches_before_rotation"], nb)
    pre = np.where(r["dropped"] >= 0, r["dropped"], r["mp"])
    assert np.array_equal(pre, m), int((pre != m).sum())
    if r["status"] == capi.DVM_TRACK_FEW_MATCHES:
        assert nm < 15 and np.array_equal(r["pose"], _widen(pose_last)) and not r["outlier"].any() and (r["dropped"] < 0).all()
        return
    sep = _pose_and_drop(capi, kf, kps_un, m, pose_last, inv_s2, gpu=True)
    for k in ("n_edges", "n_inliers", "nmatches_map", "nmatches_after"):
        assert r[k] == sep[k], (k, r[k], sep[k])
    for k in ("outlier", "mp", "dropped"):
        assert np.array_equal(r[k], sep[k]), k
    assert np.array_equal(r["pose"], sep["pose"]), (r["pose"], sep["pose"])
    assert r["status"] == (capi.DVM_TRACK_COMPLETE if sep["nmatches_map"] >= 10 else capi.DVM_TRACK_FEW_MAP_MATCHES)
    assert np.array_equal(r["Tcw"], np.concatenate([r["pose"][3:7], r["pose"][0:3]]).astype(np.float32))
    if oracle:
        ov = po.vocab_transform(voc, desc, levelsup)
        assert np.array_equal(ov["bow_ids"], host["bow_ids"]) and np.array_equal(ov["fv_feat"], host["fv_feat"])
        n_o, m_o = po.search_by_bow_kf_frame(kf["kps"], kf["desc"], kf["mp"], kf["bad"], kf["fv"], kps_un, desc, ov, 0.7, check_ori)
        assert n_o == r["nmatches"] and np.array_equal(m_o, pre)
        orc = _pose_and_drop(po, kf, kps_un, m_o, pose_last, inv_s2, gpu=False)
        for k in ("outlier", "mp", "dropped"):
            assert np.array_equal(r[k], orc[k]), k
        assert r["n_inliers"] == orc["n_inliers"] and r["nmatches_map"] == orc["nmatches_map"]
        assert np.abs(r["pose"] - orc["pose"]).max() < 1e-6, (r["pose"], orc["pose"])


def _new(capi, n_kf=8192, local=0):
    ext = capi.OrbExtractor(max_batch=1)
    trk = capi.Tracker(ext)
    trk.reserve_reference_keyframe(n_kf)
    if local:
        trk.reserve_local_map(local)
    return ext, trk


def _form_a(trk, vocd, kf, pose_last, img, w, **kw):
    return trk.track_reference_keyframe(vocd, kf, pose_last, img=img, K=ps.K, bounds=BOUNDS, inv_sigma2=w["inv_s2"], **kw)


@pytest.mark.parametrize("t", [1, 2, 3])
def test_form_a_equals_separate_calls_and_oracle(scene, world, t):
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    ext, trk = _new(capi)
    kf = _kf(capi, w, w["voc"])
    pose_last = _tcw7f(ps.pose7(*poses[t - 1]))
    r = _form_a(trk, vocd, kf, pose_last, frames[t], w)
    n, k, d, mono = ext.extract(frames[t])
    assert r["n"] == n and r["mono_index"] == mono
    assert np.array_equal(r["kps"], k) and np.array_equal(r["desc"], d) and np.array_equal(r["kps_un"], k)
    assert r["status"] == capi.DVM_TRACK_COMPLETE and r["nmatches"] >= 15, (r["status"], r["nmatches"])
    assert r["nmatches_before_rotation"] >= r["nmatches"] and r["n_bow"] > 100 and r["n_fv"] > 10
    _check_against_separate(capi, po, r, kf, w["voc"], d, k, pose_last, w["inv_s2"])
    gt = ps.pose7(*poses[t])
    assert np.abs(r["pose"][:3] - gt[:3]).max() < 0.05          # and it finds the camera
    trk.close(); ext.close(); vocd.close()


def test_small_ragged_vocabulary_with_stopped_words(scene, world):
    """k = 6 ragged, L = 5 (FeatureVector nodes at level 1), a tenth of the words stopped (weight 0: neither in mBowVec nor in mFeatVec)."""
    from dvm_slam_amd import capi, synth
    from oracle import pyoracle as po
    frames, poses = scene
    w = world
    voc = synth.vocabulary(k=6, L=5, ragged=True, seed=9, stop_frac=0.1)
    rng = np.random.default_rng(3)
    voc["desc"] = np.concatenate([w["desc"], w["pts"]["desc"]])[rng.integers(0, len(w["pts"]), voc["n_nodes"])]
    assert (voc["weight"][voc["word_id"] >= 0] == 0).any()
    vocd = capi.Vocabulary(voc)
    ext, trk = _new(capi)
    kf = _kf(capi, w, voc)
    pose_last = _tcw7f(ps.pose7(*poses[0]))
    r = _form_a(trk, vocd, kf, pose_last, frames[1], w)
    assert len(r["fv_feat"]) < r["n"]                           # the stopped words' features are left out
    _check_against_separate(capi, po, r, kf, voc, r["desc"], r["kps_un"], pose_last, w["inv_s2"])
    assert r["nmatches"] >= 15
    trk.close(); ext.close(); vocd.close()


def early_leaf_vocabulary(w):
    """A (10, 4) tree shaped like DBoW2's (voc_scene.dbow2_tree: leaves at levels 1..4, 1..10 children, equal siblings) whose node
    descriptors are the scene's own, and the levelsup under which the frame's and the keyframe's FeatureVector both end in node -1."""
    import voc_scene as vs
    voc = vs.dbow2_tree(10, 4, **vs.TREES[(10, 4)])
    rng = np.random.default_rng(7)
    pool = np.concatenate([w["desc"], w["pts"]["desc"]])
    voc["desc"] = pool[rng.integers(0, len(pool), voc["n_nodes"])]
    return voc, 1


def matches_in_node_minus_one(r):
    """The final matches of a chain result whose frame feature lies in node -1 of the frame's FeatureVector."""
    import voc_scene as vs
    node = vs.node_of_feature(r, len(r["mp"]))
    return int(((r["mp"] >= 0) & (node == 0xFFFFFFFF)).sum())


@pytest.mark.parametrize("t", [1, 2])
def test_feature_vectors_that_end_in_node_minus_one(scene, world, t):
    """Leaves above level L - levelsup: ComputeBoW puts their features into node -1, the last node of mFeatVec as DBoW2 orders it, in
    the frame and in the keyframe, and SearchByBoW matches inside it -- chain, separate calls and oracle alike."""
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    w = world
    voc, levelsup = early_leaf_vocabulary(w)
    vocd = capi.Vocabulary(voc)
    ext, trk = _new(capi)
    kf = _kf(capi, w, voc, levelsup=levelsup)
    pose_last = _tcw7f(ps.pose7(*poses[t - 1]))
    r = _form_a(trk, vocd, kf, pose_last, frames[t], w, levelsup=levelsup)
    assert kf["fv"]["fv_nodes"][-1] == -1 and r["fv_nodes"][-1] == -1 and np.all(r["fv_nodes"][:-1] >= 0)
    _check_against_separate(capi, po, r, kf, voc, r["desc"], r["kps_un"], pose_last, w["inv_s2"], levelsup=levelsup)
    assert r["status"] == capi.DVM_TRACK_COMPLETE and matches_in_node_minus_one(r) >= 5
    trk.close(); ext.close(); vocd.close()


def test_form_b_after_a_failed_motion_model_equals_form_a(scene, world):
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    kf = _kf(capi, w, w["voc"])
    pose_last = _tcw7f(ps.pose7(*poses[1]))
    ext_a, trk_a = _new(capi)
    a = _form_a(trk_a, vocd, kf, pose_last, frames[2], w)
    ext, trk = _new(capi)
    pts = w["pts"]
    mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
    mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
    k0 = w["kps"]
    wrong = ps.pose7(*poses[1]).copy()
    wrong[0] += 100.0                                           # a prediction far off: no point projects into the image, the motion model fails
    first = trk.track(frames[2], _tcw7f(wrong), ps.K, BOUNDS, w["scale"], w["inv_s2"], k0, np.arange(len(k0), dtype=np.int32), None, mps, th=15.0)
    assert not first["tracked"]
    b = trk.track_reference_keyframe(vocd, kf, pose_last, K=ps.K, inv_sigma2=w["inv_s2"])
    for k, v in a.items():
        if k in ("kps", "desc", "kps_un"):
            continue
        assert np.array_equal(np.asarray(v), np.asarray(b[k])), k
    assert b["status"] == capi.DVM_TRACK_COMPLETE
    # and a COMPLETE first half followed by the chain (the caller's own decision): the same again
    first = trk.track(frames[2], _tcw7f(ps.pose7(*poses[1])), ps.K, BOUNDS, w["scale"], w["inv_s2"], k0, np.arange(len(k0), dtype=np.int32), None,
                      mps, th=15.0)
    assert first["tracked"]
    c = trk.track_reference_keyframe(vocd, kf, pose_last, K=ps.K, inv_sigma2=w["inv_s2"])
    assert np.array_equal(c["pose"], a["pose"]) and np.array_equal(c["mp"], a["mp"]) and c["nmatches_map"] == a["nmatches_map"]
    for x in (trk, ext, trk_a, ext_a, vocd):
        x.close()


# the local-map tests' composition of the separate calls (tests/test_gpu_track_local_map.py), copied
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


def _separate_local_map(mod, kps_un, desc, frame_mp, pts, Tcw, K, bounds, scale, inv_s2, th, far, th_far):
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


def _check_local_map(a, b, exact):
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


def test_local_map_after_the_chain_equals_separate_composition(scene, world):
    """TrackLocalMap behind a COMPLETE chain: equal to SearchLocalPoints -> SearchByProjection -> PoseOptimization composed over the separate
    calls, seeded from the chain's Tcw, bit for bit; after FEW_MATCHES / FEW_MAP_MATCHES it is refused."""
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    pts = w["pts"]
    vocd = capi.Vocabulary(w["voc"])
    ext, trk = _new(capi, local=len(pts))
    kf = _kf(capi, w, w["voc"])
    for form in ("a", "b"):
        pose_last = _tcw7f(ps.pose7(*poses[2]))
        if form == "a":
            r = _form_a(trk, vocd, kf, pose_last, frames[3], w)
        else:
            mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
            mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
            wrong = ps.pose7(*poses[2]).copy(); wrong[0] += 100.0
            first = trk.track(frames[3], _tcw7f(wrong), ps.K, BOUNDS, w["scale"], w["inv_s2"], w["kps"], np.arange(len(w["kps"]), dtype=np.int32), None,
                              mps, th=15.0)
            assert not first["tracked"]
            r = trk.track_reference_keyframe(vocd, kf, pose_last, K=ps.K, inv_sigma2=w["inv_s2"])
            r.update(kps_un=first["kps_un"], desc=first["desc"])     # (form b hands back no keypoints: the first half's)
        assert r["status"] == capi.DVM_TRACK_COMPLETE
        fm = np.where(r["mp"] >= 0, r["mp"] - MP_BASE, -1).astype(np.int32)
        fused = trk.track_local_map(pts, fm, th=1.0)
        sep = _separate_local_map(capi, r["kps_un"], r["desc"], fm, pts, r["Tcw"], ps.K.astype(np.float32), BOUNDS, w["scale"], w["inv_s2"], 1.0, False, 0.0)
        _check_local_map(fused, sep, exact=True)
        assert fused["nmatches"] > 0
    # FEW_MATCHES (a handful of map points) and FEW_MAP_MATCHES (nearly all points unobserved): the second half is refused
    few = w["mp"].copy(); few[12:] = -1
    r = _form_a(trk, vocd, _kf(capi, w, w["voc"], mp=few), _tcw7f(ps.pose7(*poses[2])), frames[3], w)
    assert r["status"] == capi.DVM_TRACK_FEW_MATCHES and r["nmatches"] < 15 and r["n_edges"] == 0
    assert np.array_equal(r["pose"], _widen(_tcw7f(ps.pose7(*poses[2]))))
    with pytest.raises(capi.DvmError) as e:
        trk.track_local_map(pts, np.full(r["n"], -1, np.int32))
    assert e.value.code == -6
    p0 = pts.copy(); p0["n_obs"] = 0; p0["n_obs"][:5] = 2
    r = _form_a(trk, vocd, _kf(capi, w, w["voc"], pts=p0), _tcw7f(ps.pose7(*poses[2])), frames[3], w)
    assert r["status"] == capi.DVM_TRACK_FEW_MAP_MATCHES and r["nmatches"] >= 15 and r["nmatches_map"] < 10
    with pytest.raises(capi.DvmError) as e:
        trk.track_local_map(p0, np.full(r["n"], -1, np.int32))
    assert e.value.code == -6
    trk.close(); ext.close(); vocd.close()


def test_edge_keyframes(scene, world):
    """Statuses, empty and invalid keyframes, claims inside one node, the single-node vocabulary, a distorted camera."""
    from dvm_slam_amd import capi, synth
    from oracle import pyoracle as po
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    ext, trk = _new(capi)
    pose_last = _tcw7f(ps.pose7(*poses[0]))
    img = frames[1]

    def run(kf, voc=w["voc"], vd=vocd, **kw):
        r = _form_a(trk, vd, kf, pose_last, img, w, **kw)
        _check_against_separate(capi, po, r, kf, voc, r["desc"], r["kps_un"], pose_last, w["inv_s2"])
        return r

    # no map points at all / every point bad / an empty FeatureVector: nothing to match, pose untouched
    r = run(_kf(capi, w, w["voc"], mp=np.full(len(w["mp"]), -1, np.int32)))
    assert r["nmatches"] == 0 and r["status"] == capi.DVM_TRACK_FEW_MATCHES
    pb = w["pts"].copy(); pb["bad"] = 1
    r = run(_kf(capi, w, w["voc"], pts=pb))
    assert r["nmatches"] == 0 and r["status"] == capi.DVM_TRACK_FEW_MATCHES
    kf = _kf(capi, w, w["voc"])
    kf["fv"] = dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))
    r = run(kf)
    assert r["nmatches"] == 0 and r["n_bow"] > 0
    # -1 holes in a third of the keyframe
    holes = w["mp"].copy(); holes[::3] = -1
    r = run(_kf(capi, w, w["voc"], mp=holes))
    assert r["nmatches"] >= 15
    # claims: groups of keyframe features with the same descriptor compete for the same frame features inside one node
    dd = w["desc"].copy()
    rng = np.random.default_rng(41)
    src = rng.choice(len(dd), 60, replace=False)
    for s in src:
        dd[rng.choice(len(dd), 4, replace=False)] = dd[s]
    r = run(_kf(capi, w, w["voc"], desc=dd))
    assert r["nmatches"] > 0
    # the single-node vocabulary (L - levelsup <= 0: every feature in node 0): one wave walks the whole frame
    v1 = synth.vocabulary(k=8, L=3, ragged=True, seed=13, stop_frac=0.05)
    v1["desc"] = w["pts"]["desc"][rng.integers(0, len(w["pts"]), v1["n_nodes"])]
    vd1 = capi.Vocabulary(v1)
    r = run(_kf(capi, w, v1), voc=v1, vd=vd1)
    assert r["n_fv"] == 1 and r["fv_nodes"][0] == 0 and r["nmatches"] >= 15
    vd1.close()
    # a distorted camera in form (a): kps_un are the device-undistorted keypoints dvm_track_finish gives
    cam = np.array([500.0, 500.0, 320.0, 240.0, -0.04, 0.01, 0.0005, -0.0003, 0.0], np.float32)
    dist = capi.Distortion(*[float(v) for v in cam])
    bounds = capi.image_bounds(cam, 640, 480)
    kf = _kf(capi, w, w["voc"])
    r = trk.track_reference_keyframe(vocd, kf, pose_last, img=img, K=ps.K, bounds=bounds, inv_sigma2=w["inv_s2"], dist=dist)
    assert not np.array_equal(r["kps_un"]["x"], r["kps"]["x"])
    _check_against_separate(capi, po, r, kf, w["voc"], r["desc"], r["kps_un"], pose_last, w["inv_s2"])
    ext2 = capi.OrbExtractor(max_batch=1)
    trk2 = capi.Tracker(ext2)
    pts = w["pts"]
    mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
    mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
    f = trk2.track(img, pose_last, ps.K, bounds, w["scale"], w["inv_s2"], w["kps"], np.arange(len(w["kps"]), dtype=np.int32), None, mps, th=15.0, dist=dist)
    assert np.array_equal(f["kps_un"], r["kps_un"])
    trk2.close(); ext2.close()
    trk.close(); ext.close(); vocd.close()


def test_call_sequence_and_capacity(scene, world):
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    kf = _kf(capi, w, w["voc"])
    pose_last = _tcw7f(ps.pose7(*poses[0]))
    ext = capi.OrbExtractor(max_batch=1)
    trk = capi.Tracker(ext)
    kw = dict(K=ps.K, inv_sigma2=w["inv_s2"])
    # no begin / no reservation
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, kf, pose_last, **kw)
    assert e.value.code == -6
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, kf, pose_last, img=frames[1], bounds=BOUNDS, **kw)
    assert e.value.code == -6
    # a keyframe above the reservation: DVM_ERR_CAPACITY; the begun frame is still there for a call that fits (form a, no new begin)
    trk.reserve_reference_keyframe(len(w["kps"]) - 1)
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, kf, pose_last, bounds=BOUNDS, **kw)
    assert e.value.code == -3
    trk.reserve_reference_keyframe(len(w["kps"]))
    r = trk.track_reference_keyframe(vocd, kf, pose_last, bounds=BOUNDS, **kw)
    assert r["status"] == capi.DVM_TRACK_COMPLETE
    # a second call on one begin
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, kf, pose_last, **kw)
    assert e.value.code == -6
    # another extraction on the extractor in between: the frame is gone
    L = capi.lib()
    L.dvm_track_begin.restype = C.c_int32
    L.dvm_track_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    img = np.ascontiguousarray(frames[1])
    capi.check(L.dvm_track_begin(trk.t, ext.h, img.ctypes.data, 480, 640, img.strides[0], 0, 1000))
    ext.extract(frames[2])
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, kf, pose_last, **kw)
    assert e.value.code == -6
    # a malformed FeatureVector: DVM_ERR_INVALID
    bad_fv = dict(kf, fv=dict(kf["fv"], fv_feat=np.full(len(kf["fv"]["fv_feat"]), len(w["kps"]), np.int32)))
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, bad_fv, pose_last, img=frames[1], bounds=BOUNDS, **kw)
    assert e.value.code == -1
    r = trk.track_reference_keyframe(vocd, kf, pose_last, bounds=BOUNDS, **kw)    # (the refused call left the begin for one that is well formed)
    assert r["status"] == capi.DVM_TRACK_COMPLETE
    # form (a) with empty frame bounds: DVM_ERR_INVALID before anything runs, the begin still there
    capi.check(L.dvm_track_begin(trk.t, ext.h, img.ctypes.data, 480, 640, img.strides[0], 0, 1000))
    with pytest.raises(capi.DvmError) as e:
        trk.track_reference_keyframe(vocd, kf, pose_last, **kw)
    assert e.value.code == -1
    r = trk.track_reference_keyframe(vocd, kf, pose_last, bounds=BOUNDS, **kw)
    assert r["status"] == capi.DVM_TRACK_COMPLETE
    trk.close(); ext.close()
    # a batch tracker: refused
    ext = capi.OrbExtractor(max_batch=2)
    tb = capi.TrackerBatch(ext, 2)
    with pytest.raises(capi.DvmError) as e:
        capi.Tracker.reserve_reference_keyframe(tb, 4096)
    assert e.value.code == -6
    with pytest.raises(capi.DvmError) as e:
        capi.Tracker.track_reference_keyframe(tb, vocd, kf, pose_last, img=frames[1], bounds=BOUNDS, **kw)
    assert e.value.code == -6
    ext.sync()
    tb.close(); ext.close(); vocd.close()


def test_reference_keyframe_reservations_release_their_memory(scene, world):
    import torch
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    kf = _kf(capi, w, w["voc"])
    pose_last = _tcw7f(ps.pose7(*poses[0]))
    ext = capi.OrbExtractor(max_batch=1)

    def cycle():
        trk = capi.Tracker(ext)
        trk.reserve_reference_keyframe(8192)
        trk.reserve_reference_keyframe(len(w["kps"]))        # a second reservation replaces the first
        trk.track_reference_keyframe(vocd, kf, pose_last, img=frames[1], K=ps.K, bounds=BOUNDS, inv_sigma2=w["inv_s2"])
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
    ext.close(); vocd.close()
