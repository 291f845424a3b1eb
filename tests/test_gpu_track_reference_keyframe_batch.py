"""dvm_track_reference_keyframe_batch (TrackerBatch.track_reference_keyframe): Tracking::TrackReferenceKeyFrame for the frames of a batched
first half that need it, as ONE device chain.  Frame b must equal dvm_track_reference_keyframe (form b) on that frame alone, bit for bit, and the
batched second half behind it must equal the single-frame sequence begin -> finish -> [reference keyframe] -> dvm_track_local_map.  Scenes:
pixel_scene frames, keyframes = earlier frames with their map points back-projected (helpers copied from the single call's tests)."""
import ctypes as C

import numpy as np
import pytest

import pixel_scene as ps

pytestmark = pytest.mark.gpu

BOUNDS = np.array([0, 640, 0, 480], np.float32)
LEVELSUP = 4
FORM_B_KEYS = ("n", "mono_index", "status", "nmatches", "nmatches_before_rotation", "n_edges", "n_inliers", "nmatches_after", "nmatches_map", "n_bow",
               "n_fv", "mp", "dropped", "outlier", "bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat", "pose", "Tcw")


def _tcw7f(p):   # (t, q) doubles -> dvm_se3f (q, t) floats
    return np.concatenate([p[3:7], p[0:3]]).astype(np.float32)


def _widen(T):   # dvm_se3f (q, t) floats -> PoseOptimization's seed (t, q) doubles
    T = np.asarray(T, np.float32)
    return np.concatenate([T[4:7], T[0:4]]).astype(np.float64)


def _local_points(capi, kps, desc, X, Ow, scale, rng, p_obs0=0.15, p_bad=0.03):
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
    """The extractor's tables, two keyframes (frames 0 and 2: keypoints, descriptors, back-projected map points = table entries, a few -1
    holes), the local map (both) and a k = 10, L = 6 vocabulary whose node descriptors are the scene's own."""
    from dvm_slam_amd import capi, synth
    frames, poses = scene
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(31)
    tabs, kfs = [], []
    base = 0
    for f in (0, 2):
        n, k, d, _ = ext.extract(frames[f])
        R, t = poses[f]
        X = ps.backproject(k, R, t) + rng.normal(0, 0.01, (n, 3))
        tabs.append(_local_points(capi, k, d, X, -R.T @ t, scale, rng))
        mp = (np.arange(n) + base).astype(np.int32)
        mp[rng.random(n) < 0.05] = -1
        kfs.append(dict(kps=k.copy(), desc=d.copy(), mp=mp))
        base += n
    pts = np.concatenate(tabs)
    ext.close()
    voc = synth.vocabulary(k=10, L=6, ragged=False, seed=5)
    pool = np.concatenate([k["desc"] for k in kfs])
    voc["desc"] = pool[rng.integers(0, len(pool), voc["n_nodes"])]
    mps = np.zeros(len(pts), capi.MAP_POINT_DTYPE)
    mps["pos"], mps["desc"], mps["n_obs"] = pts["pos"], pts["desc"], pts["n_obs"]
    return dict(scale=scale, inv_s2=inv_s2, pts=pts, mps=mps, voc=voc, kfs=kfs)


def _kf(capi, w, voc, which=0, mp=None, pts=None, desc=None, levelsup=LEVELSUP):
    """dvm_ref_keyframe as a dict: map-point fields looked up in the table by id, mFeatVec from the host transform of its descriptors."""
    src = w["kfs"][which]
    pts = w["pts"] if pts is None else pts
    mp = src["mp"] if mp is None else mp
    desc = src["desc"] if desc is None else desc
    ix = np.maximum(mp, 0)
    fv = capi.vocab_transform_host(voc, desc, levelsup)
    return dict(kps=src["kps"], desc=desc, mp=np.ascontiguousarray(mp, np.int32), pos=pts["pos"][ix], n_obs=pts["n_obs"][ix].astype(np.int32),
                bad=pts["bad"][ix].astype(np.uint8), fv=fv)


def _cut_fv(kf, nf):
    """The keyframe with its FeatureVector cut to its first nf nodes (still a valid mFeatVec)."""
    fv = kf["fv"]
    off = fv["fv_off"][:nf + 1]
    return dict(kf, fv=dict(fv, fv_nodes=fv["fv_nodes"][:nf], fv_off=off, fv_feat=fv["fv_feat"][:off[-1]]))


def _last(w, mode):
    """(kps_l, mp_l, outlier_l, mps) of an agent's LastFrame: keyframe 0's keypoints holding their points, or nothing (no motion model)."""
    k0 = w["kfs"][0]["kps"]
    if mode == "none":
        return (k0[:0], np.zeros(0, np.int32), None, w["mps"])
    return (k0, np.arange(len(k0), dtype=np.int32), None, w["mps"])


def _pred(poses, t, mode):
    p = ps.pose7(*poses[t - 1]).copy()
    if mode == "fail":
        p[0] += 100.0            # a prediction far off: no point projects into the image, the motion model fails
    return _tcw7f(p)


class Single:
    """One single-frame tracker running the per-frame sequence the batch must reproduce."""

    def __init__(self, capi, w, local=0):
        self.capi, self.w = capi, w
        self.ext = capi.OrbExtractor(max_batch=1)
        self.trk = capi.Tracker(self.ext)
        self.trk.reserve_reference_keyframe(8192)
        if local:
            self.trk.reserve_local_map(local)

    def first(self, img, pred, last, dist=None, bounds=BOUNDS):
        kl, ml, ol, mps = last
        w = self.w
        return self.trk.track(img, pred, ps.K, bounds, w["scale"], w["inv_s2"], kl, ml, ol, mps, th=15.0, dist=dist)

    def refkf(self, vocd, kf, pose_last):
        return self.trk.track_reference_keyframe(vocd, kf, pose_last, K=ps.K, inv_sigma2=self.w["inv_s2"])

    def close(self):
        self.trk.close(); self.ext.close()


def _same(a, b, keys=FORM_B_KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])


def _new_batch(capi, B, total=None, local=0):
    ext = capi.OrbExtractor(max_batch=B)
    tb = capi.TrackerBatch(ext, B)
    tb.reserve_reference_keyframe(total if total is not None else B * 8192)
    if local:
        tb.reserve_local_map(local)
    return ext, tb


def _first_batch(tb, w, frames, poses, ts, modes):
    imgs = np.stack([frames[t] for t in ts])
    ins = tb.prepare([_pred(poses, t, m) for t, m in zip(ts, modes)], [_last(w, m) for m in modes])
    return tb.track(imgs, ins, ps.K, BOUNDS, w["scale"], w["inv_s2"], th=15.0)


def _pose_and_drop_oracle(po, kf, kps_un, m, pose_last, inv_s2):
    id_to_kf = {int(i): k for k, i in enumerate(kf["mp"]) if i >= 0}
    sel = np.flatnonzero(m >= 0)
    src = np.array([id_to_kf[int(i)] for i in m[sel]], np.int64)
    Xw = kf["pos"][src].astype(np.float64).reshape(-1, 3)
    obs = np.column_stack([kps_un["x"][sel], kps_un["y"][sel]]).astype(np.float64).reshape(-1, 2)
    wgt = inv_s2[kps_un["octave"][sel]].astype(np.float64)
    pose, outl, nin = po.pose_optimize(_widen(pose_last), Xw, obs, wgt, ps.K)
    outl = np.asarray(outl)[:len(sel)]
    outlier = np.zeros(len(m), np.uint8)
    outlier[sel] = outl != 0
    return dict(pose=np.asarray(pose, np.float64), outlier=outlier, mp=np.where(outlier != 0, -1, m).astype(np.int32),
                dropped=np.where(outlier != 0, m, -1).astype(np.int32), n_inliers=int(nin), nmatches_map=int((kf["n_obs"][src[outl == 0]] > 0).sum()))


def test_mixed_tick_then_second_half(scene, world):
    """B = 6: two frames tracked by their motion model, two whose motion model failed, two without one.  The four that are not complete
    run the chain; each equals a single tracker's begin -> track -> track_reference_keyframe (form b) bit for bit, one also the oracle
    composition.  Then dvm_track_local_map_batch: every complete frame equals the single-frame sequence with dvm_track_local_map."""
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    w = world
    pts = w["pts"]
    vocd = capi.Vocabulary(w["voc"])
    ts = [1, 2, 3, 2, 4, 5]
    modes = ["ok", "ok", "fail", "fail", "none", "none"]
    kf_all = [_kf(capi, w, w["voc"], which=0), _kf(capi, w, w["voc"], which=0), _kf(capi, w, w["voc"], which=0),
              _kf(capi, w, w["voc"], which=1), _kf(capi, w, w["voc"], which=1), _kf(capi, w, w["voc"], which=1)]
    holes = w["kfs"][0]["mp"].copy(); holes[::5] = -1
    kf_all[2] = _kf(capi, w, w["voc"], which=0, mp=holes)              # a different keyframe per agent
    run = [m != "ok" for m in modes]
    kfs = [k if r else None for k, r in zip(kf_all, run)]
    pose_last = [_tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext, tb = _new_batch(capi, 6, local=6 * 16384)
    first = _first_batch(tb, w, frames, poses, ts, modes)
    assert [bool(f["tracked"]) for f in first] == [True, True, False, False, False, False]
    firsts = [dict(f, mp=f["mp"].copy(), kps_un=f["kps_un"].copy(), desc=f["desc"].copy()) for f in first]
    rb = tb.track_reference_keyframe(vocd, kfs, pose_last, ps.K, w["inv_s2"])
    S = Single(capi, w, local=16384)
    singles = []
    for b in range(6):
        f1 = S.first(frames[ts[b]], _pred(poses, ts[b], modes[b]), _last(w, modes[b]))
        assert bool(f1["tracked"]) == (modes[b] == "ok")
        if run[b]:
            r1 = S.refkf(vocd, kf_all[b], pose_last[b])
            _same(rb[b], r1)
            assert rb[b]["status"] == capi.DVM_TRACK_COMPLETE and rb[b]["nmatches"] >= 15
            mp = np.where(r1["mp"] >= 0, r1["mp"], -1).astype(np.int32)
        else:
            assert rb[b]["status"] == capi.DVM_TRACK_COMPLETE
            assert all(rb[b][k] == 0 for k in ("n", "nmatches", "n_edges", "n_bow", "n_fv")) and "mp" not in rb[b]
            mp = f1["mp"].astype(np.int32)
        lm = S.trk.track_local_map(pts, mp, th=1.0)
        singles.append((mp, lm))
    # one frame that ran against the oracle composition: identical assignments and flags, pose within 1e-6
    b = 4
    r, kf, f = rb[b], kf_all[b], firsts[b]
    ov = po.vocab_transform(w["voc"], f["desc"], LEVELSUP)
    assert np.array_equal(ov["bow_ids"], r["bow_ids"]) and np.array_equal(ov["fv_feat"], r["fv_feat"])
    n_o, m_o = po.search_by_bow_kf_frame(kf["kps"], kf["desc"], kf["mp"], kf["bad"], kf["fv"], f["kps_un"], f["desc"], ov, 0.7, True)
    pre = np.where(r["dropped"] >= 0, r["dropped"], r["mp"])
    assert n_o == r["nmatches"] and np.array_equal(m_o, pre)
    orc = _pose_and_drop_oracle(po, kf, f["kps_un"], m_o, pose_last[b], w["inv_s2"])
    for k in ("outlier", "mp", "dropped"):
        assert np.array_equal(r[k], orc[k]), k
    assert r["n_inliers"] == orc["n_inliers"] and r["nmatches_map"] == orc["nmatches_map"]
    assert np.abs(r["pose"] - orc["pose"]).max() < 1e-6, (r["pose"], orc["pose"])
    # the second half of every frame, whichever way it was completed
    lb = tb.track_local_map([pts] * 6, [s[0] for s in singles], th=1.0)
    for b in range(6):
        assert lb[b]["status"] == capi.DVM_TRACK_COMPLETE
        _same(lb[b], singles[b][1], ("n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers", "mp",
                                     "outlier", "pose", "Tcw"))
        assert lb[b]["nmatches"] > 0
    S.close(); tb.close(); ext.close(); vocd.close()


def test_feature_vectors_that_end_in_node_minus_one(scene, world):
    """Three frames on a tree with leaves above level L - levelsup (tests/test_gpu_track_reference_keyframe.early_leaf_vocabulary): the
    batched transform walks rows of unequal depth, every frame's and keyframe's FeatureVector ends in node -1, and each frame equals the
    separate calls bit for bit and the oracle, with matches inside node -1."""
    import test_gpu_track_reference_keyframe as one
    from dvm_slam_amd import capi
    from oracle import pyoracle as po
    frames, poses = scene
    w = world
    voc, levelsup = one.early_leaf_vocabulary(dict(desc=w["kfs"][0]["desc"], pts=w["pts"]))
    vocd = capi.Vocabulary(voc)
    ts, which = [1, 2, 3], [0, 0, 1]
    kfs = [_kf(capi, w, voc, which=k, levelsup=levelsup) for k in which]
    pose_last = [_tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext, tb = _new_batch(capi, 3)
    first = _first_batch(tb, w, frames, poses, ts, ["none"] * 3)
    firsts = [dict(kps_un=f["kps_un"].copy(), desc=f["desc"].copy()) for f in first]
    rb = tb.track_reference_keyframe(vocd, kfs, pose_last, ps.K, w["inv_s2"], levelsup=levelsup)
    for b in range(3):
        r, kf = rb[b], kfs[b]
        assert kf["fv"]["fv_nodes"][-1] == -1 and r["fv_nodes"][-1] == -1 and np.all(r["fv_nodes"][:-1] >= 0)
        one._check_against_separate(capi, po, r, kf, voc, firsts[b]["desc"], firsts[b]["kps_un"], pose_last[b], w["inv_s2"], levelsup=levelsup)
        assert r["status"] == capi.DVM_TRACK_COMPLETE and one.matches_in_node_minus_one(r) >= 5
    tb.close(); ext.close(); vocd.close()


@pytest.mark.parametrize("distorted", [False, True])
def test_batch_of_one_on_a_single_frame_tracker(scene, world, distorted):
    """count = 1 on a dvm_tracker_create tracker equals dvm_track_reference_keyframe form (b); dvm_track_local_map follows as after it and
    the single call is refused on that finish."""
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    pts = w["pts"]
    vocd = capi.Vocabulary(w["voc"])
    dist, bounds = None, BOUNDS
    if distorted:
        cam = np.array([500.0, 500.0, 320.0, 240.0, -0.04, 0.01, 0.0005, -0.0003, 0.0], np.float32)
        dist = capi.Distortion(*[float(v) for v in cam])
        bounds = capi.image_bounds(cam, 640, 480)
    kf = _kf(capi, w, w["voc"])
    pose_last = _tcw7f(ps.pose7(*poses[2]))
    A = Single(capi, w, local=len(pts))
    B = Single(capi, w, local=len(pts))
    capi.TrackerBatch.reserve_reference_keyframe(B.trk, 8192)
    pred = _pred(poses, 3, "fail")
    fa = A.first(frames[3], pred, _last(w, "ok"), dist=dist, bounds=bounds)
    fb = B.first(frames[3], pred, _last(w, "ok"), dist=dist, bounds=bounds)
    assert not fa["tracked"] and np.array_equal(fa["kps_un"], fb["kps_un"])
    if distorted:
        assert not np.array_equal(fb["kps_un"]["x"], fb["kps"]["x"])
    ra = A.refkf(vocd, kf, pose_last)
    rb = capi.TrackerBatch.track_reference_keyframe(B.trk, vocd, [kf], [pose_last], ps.K, w["inv_s2"])[0]
    _same(rb, ra)
    assert rb["status"] == capi.DVM_TRACK_COMPLETE
    with pytest.raises(capi.DvmError) as e:
        B.refkf(vocd, kf, pose_last)
    assert e.value.code == -6
    fm = rb["mp"].astype(np.int32)
    _same(B.trk.track_local_map(pts, fm, th=1.0), A.trk.track_local_map(pts, fm, th=1.0),
          ("n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers", "mp", "outlier", "pose", "Tcw"))
    with pytest.raises(capi.DvmError) as e:
        B.trk.track_local_map(pts, fm, th=1.0)          # once per finish
    assert e.value.code == -6
    A.close(); B.close(); vocd.close()


def test_edge_keyframes_in_one_batch(scene, world):
    """An empty keyframe, one without a FeatureVector, one whose points are all bad, one of 8 192 keypoints, frames ending FEW_MATCHES and
    FEW_MAP_MATCHES, keyframe node counts = 1, 2, 3 (mod 4) side by side; then the whole batch again with a ragged vocabulary with stopped
    words.  Every frame equals its single call."""
    from dvm_slam_amd import capi, synth
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    k0 = w["kfs"][0]

    def batch_kfs(voc):
        kf = _kf(capi, w, voc)
        empty = dict(kps=k0["kps"][:0], desc=k0["desc"][:0], mp=np.zeros(0, np.int32), pos=np.zeros((0, 3), np.float32), n_obs=np.zeros(0, np.int32),
                     bad=None, fv=dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32)))
        nofv = dict(kf, fv=dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32)))
        pb = w["pts"].copy(); pb["bad"] = 1
        allbad = _kf(capi, w, voc, pts=pb)
        reps = -(-8192 // len(k0["kps"]))
        big_src = dict(kps=np.tile(k0["kps"], reps)[:8192], desc=np.tile(k0["desc"], (reps, 1))[:8192], mp=np.tile(k0["mp"], reps)[:8192])
        wb = dict(w, kfs=[big_src])
        big = _kf(capi, wb, voc)
        few_mp = k0["mp"].copy(); few_mp[12:] = -1
        few = _kf(capi, w, voc, mp=few_mp)
        p0 = w["pts"].copy(); p0["n_obs"] = 0; p0["n_obs"][:5] = 2
        fewmap = _kf(capi, w, voc, pts=p0)
        nf = len(kf["fv"]["fv_nodes"])
        cuts = [_cut_fv(kf, r + 4 * ((nf - r) // 4) if nf >= r else nf) for r in (1, 2, 3)]
        cut_kf1 = _cut_fv(_kf(capi, w, voc, which=1), 5)
        return [empty, nofv, allbad, big, few, fewmap] + cuts + [cut_kf1, kf]

    S = Single(capi, w)
    for voc in (w["voc"], None):
        if voc is None:
            voc = synth.vocabulary(k=6, L=5, ragged=True, seed=9, stop_frac=0.1)
            rng = np.random.default_rng(3)
            voc["desc"] = np.concatenate([k0["desc"], w["pts"]["desc"]])[rng.integers(0, len(w["pts"]), voc["n_nodes"])]
            assert (voc["weight"][voc["word_id"] >= 0] == 0).any()
            vd = capi.Vocabulary(voc)
        else:
            vd = vocd
        kfs = batch_kfs(voc)
        B = len(kfs)
        if voc is w["voc"]:
            assert [len(k["fv"]["fv_nodes"]) % 4 for k in kfs[6:9]] == [1, 2, 3]
        ts = [1 + b % 3 for b in range(B)]
        pose_last = [_tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
        ext, tb = _new_batch(capi, B)
        _first_batch(tb, w, frames, poses, ts, ["none"] * B)
        rb = tb.track_reference_keyframe(vd, kfs, pose_last, ps.K, w["inv_s2"])
        for b in range(B):
            S.first(frames[ts[b]], _pred(poses, ts[b], "none"), _last(w, "none"))
            _same(rb[b], S.refkf(vd, kfs[b], pose_last[b]))
        st = [r["status"] for r in rb]
        assert st[0] == st[1] == st[2] == capi.DVM_TRACK_FEW_MATCHES and rb[0]["nmatches"] == rb[1]["nmatches"] == rb[2]["nmatches"] == 0
        assert st[4] == capi.DVM_TRACK_FEW_MATCHES and np.array_equal(rb[4]["pose"], _widen(pose_last[4]))
        if voc is w["voc"]:
            assert st[5] == capi.DVM_TRACK_FEW_MAP_MATCHES and st[-1] == capi.DVM_TRACK_COMPLETE and rb[3]["n_bow"] > 0
        else:
            assert len(rb[-1]["fv_feat"]) < rb[-1]["n"]         # the stopped words' features are left out
            vd.close()
        tb.close(); ext.close()
    S.close(); vocd.close()


def test_thirty_two_frames_all_running(scene, world):
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    B = 32
    ts = [1 + b % 7 for b in range(B)]
    modes = ["fail" if b % 2 else "none" for b in range(B)]
    kfs = [_kf(capi, w, w["voc"], which=0 if t <= 3 else 1) for t in ts]
    pose_last = [_tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext, tb = _new_batch(capi, B)
    first = _first_batch(tb, w, frames, poses, ts, modes)
    assert not any(f["tracked"] for f in first) and min(f["n"] for f in first) > 500
    rb = tb.track_reference_keyframe(vocd, kfs, pose_last, ps.K, w["inv_s2"])
    S = Single(capi, w)
    for b in range(B):
        S.first(frames[ts[b]], _pred(poses, ts[b], modes[b]), _last(w, modes[b]))
        _same(rb[b], S.refkf(vocd, kfs[b], pose_last[b]))
    assert sum(r["status"] == capi.DVM_TRACK_COMPLETE for r in rb) >= B // 2
    S.close(); tb.close(); ext.close(); vocd.close()


def _raw_call(capi, tb, vocd, kfs, pose_last, inv_s2, th_low):
    """dvm_track_reference_keyframe_batch with per-frame th_low (the wrapper shares it)."""
    count = len(kfs)
    kfp = (C.POINTER(capi.RefKeyframe) * count)(); prs = (capi.TrackRefKfParams * count)(); outs = (capi.TrackRefKfOut * count)()
    res = (capi.TrackRefKfResult * count)(); status = np.zeros(count, np.int32)
    keep = []
    for b in range(count):
        rk, ka = capi._ref_keyframe(kfs[b])
        pr, s2 = capi._refkf_params(pose_last[b], ps.K, inv_s2, 0.7, True, th_low[b], 15, 10, LEVELSUP)
        o, arrs = capi._refkf_out(tb.ext.cap)
        kfp[b] = C.pointer(rk); prs[b] = pr; outs[b] = o
        keep.append((rk, ka, s2, arrs))
    f = tb.L.dvm_track_reference_keyframe_batch
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 5
    return f(tb.t, tb.ext.h, vocd.h, count, kfp, prs, outs, res, status.ctypes.data)


def test_call_sequence_and_capacity(scene, world):
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    kf = _kf(capi, w, w["voc"])
    n = len(kf["kps"])
    ts, modes = [1, 2], ["fail", "none"]
    pose_last = [_tcw7f(ps.pose7(*poses[t - 1])) for t in ts]
    ext = capi.OrbExtractor(max_batch=2)
    tb = capi.TrackerBatch(ext, 2)

    def call(kfs=(kf, kf), count=2):
        return tb.track_reference_keyframe(vocd, list(kfs)[:count], pose_last[:count], ps.K, w["inv_s2"])

    def refused(code, fn=call, *a, **kw):
        with pytest.raises(capi.DvmError) as e:
            fn(*a, **kw)
        assert e.value.code == code, e.value.code

    # no reservation / no finish yet
    _first_batch(tb, w, frames, poses, ts, modes)
    refused(-6)
    tb.reserve_reference_keyframe(2 * 8192)
    tb2 = capi.TrackerBatch(ext, 2)
    tb2.reserve_reference_keyframe(2 * 8192)
    refused(-6, tb2.track_reference_keyframe, vocd, [kf, kf], pose_last, ps.K, w["inv_s2"])
    tb2.close()
    # (tb2 used no extraction: tb's finish still stands) a count that differs from the finish's
    refused(-6, call, count=1)
    # above the reservation (each keyframe rounded up to 64): DVM_ERR_CAPACITY, then a corrected call on the same finish
    tb.reserve_reference_keyframe(((n + 63) // 64) * 64 * 2 - 64)
    refused(-3)
    tb.reserve_reference_keyframe(((n + 63) // 64) * 64 * 2)
    r = call()
    assert [x["status"] for x in r] == [capi.DVM_TRACK_COMPLETE] * 2
    # a second call on one finish
    refused(-6)
    # a malformed FeatureVector, then differing shared parameters: DVM_ERR_INVALID; a corrected call on the same finish is accepted
    _first_batch(tb, w, frames, poses, ts, modes)
    bad_fv = dict(kf, fv=dict(kf["fv"], fv_feat=np.full(len(kf["fv"]["fv_feat"]), n, np.int32)))
    refused(-1, call, kfs=(kf, bad_fv))
    assert _raw_call(capi, tb, vocd, [kf, kf], pose_last, w["inv_s2"], [50, 40]) == -1
    assert _raw_call(capi, tb, vocd, [kf, kf], pose_last, w["inv_s2"], [50, 50]) == 0
    # after the second half
    tb.reserve_local_map(2 * 16384)
    first = _first_batch(tb, w, frames, poses, [1, 2], ["ok", "ok"])
    tb.track_local_map([w["pts"]] * 2, [f["mp"].astype(np.int32) for f in first], th=1.0)
    refused(-6)
    # another extraction on the extractor in between
    _first_batch(tb, w, frames, poses, ts, modes)
    ext.extract(frames[3])
    refused(-6)
    # the single call and its reservation still refuse batch trackers
    refused(-6, capi.Tracker.reserve_reference_keyframe, tb, 4096)
    _first_batch(tb, w, frames, poses, ts, modes)
    refused(-6, capi.Tracker.track_reference_keyframe, tb, vocd, kf, pose_last[0], K=ps.K, inv_sigma2=w["inv_s2"])
    # beyond max_frames x 8 192 keyframe keypoints
    refused(-3, tb.reserve_reference_keyframe, 2 * 8192 + 1)
    ext.sync()
    tb.close(); ext.close(); vocd.close()


def test_batch_reservations_release_their_memory(scene, world):
    import torch
    from dvm_slam_amd import capi
    frames, poses = scene
    w = world
    vocd = capi.Vocabulary(w["voc"])
    kf = _kf(capi, w, w["voc"])
    pose_last = [_tcw7f(ps.pose7(*poses[0]))] * 2
    ext = capi.OrbExtractor(max_batch=2)

    def cycle():
        tb = capi.TrackerBatch(ext, 2)
        tb.reserve_reference_keyframe(2 * 8192)
        tb.reserve_reference_keyframe(4096)            # a second reservation replaces the first
        _first_batch(tb, w, frames, poses, [1, 1], ["none", "none"])
        tb.track_reference_keyframe(vocd, [kf, None], pose_last, ps.K, w["inv_s2"])
        tb.close()

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
