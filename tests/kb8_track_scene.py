"""The scene of the KannalaBrandt8 tracked-frame tests (tests/test_kb8_track_scene.py pins it on the CPU; tests/test_gpu_kb8_track_*.py
run the device chains on it): a 640 x 480 fisheye camera, a last frame and a current frame of the same image under fresh pixel noise, map
points behind the last frame's own keypoints through kb8_scene.unproject, and the float64 reference of the first half --
SearchByProjection(CurrentFrame, LastFrame) in kb8_scene.frames_ref's logic, then kb8_scene.pose_kb8 on its edges.

The camera: fx = fy = 300, cx, cy = 320, 240 and the robot's k1..k4.  The image corner lies at theta = 78.9 deg, inside the 80 deg
kb8_scene uses; unproject followed by project_f32 returns within 1e-4 px; a pinhole camera of the same fx would put that corner some 900 px
away, so a chain that silently used the pinhole formula cannot pass."""
import numpy as np

import kb8_scene as ks
import pixel_scene
import pose_scene
from pose_scene import R_to_quat, normalize_pose, oplus, quat_to_R, _rot

COLS, ROWS = 640, 480
P = np.r_[np.float32([300.0, 300.0, 320.0, 240.0]), ks.ROBOMASTER[4:]].astype(np.float32)
BOUNDS = np.array([0.0, COLS, 0.0, ROWS], np.float32)     # a KannalaBrandt8 frame: mvKeysUn = mvKeys, bounds 0 .. cols / 0 .. rows
TH = 15.0
MAP_NOISE = 0.01
PLANT_FRAC = 0.1
# Grey levels (sigma) of the fresh noise on each frame, before rounding: a pixel in twenty moves by one level.  FAST and the octree's
# retention flip under noise -- from half a grey level on, 5 to 6 % of the last frame's keypoints have no counterpart in the current frame,
# each of which the search gives to a neighbour and PoseOptimization then rightly rejects.  The scene stays below that, so that the share of
# rejected matches measures the optimiser on the camera model and not the extractor's repeatability.
PIXEL_SIGMA = 0.25


def images(seed=0):
    """(last, current): the same rendered frame under pixel noise of two seeds."""
    base = pixel_scene.render(1)[0][0].astype(np.float64)
    out = []
    for k in (1, 2):
        rng = np.random.default_rng([seed, k, 640])
        out.append(np.clip(np.rint(base + rng.normal(0.0, PIXEL_SIGMA, base.shape)), 0, 255).astype(np.uint8))
    return out[0], out[1]


def theta_of(kps):
    """The angle from the optical axis of the rays through the keypoints (kb8_scene.unproject) and the rays themselves."""
    rays = ks.unproject(P, np.column_stack([kps["x"], kps["y"]])).astype(np.float64)
    return np.arctan2(np.hypot(rays[:, 0], rays[:, 1]), rays[:, 2]), rays


def points_behind(kps, R, t, z, shift=None):
    """X = R^T (z unproject(p, kp + shift) - t): the world points the keypoints see at depths z under Tcw = (R, t)."""
    uv = np.column_stack([kps["x"], kps["y"]]).astype(np.float64)
    if shift is not None:
        uv = uv + shift
    rays = ks.unproject(P, uv).astype(np.float64)
    return (z[:, None] * rays - t) @ R


def draw(kps_l, desc_l, seed, map_dtype=ks.MAP_POINT_DTYPE):
    """The true pose, the map points of the last frame's keypoints (depth 4 to 40, MAP_NOISE of position noise, one in ten moved by
    +-POSE_SHIFT_PX worth of position; a keypoint beyond 80 deg carries none) and the predicted pose (the true one perturbed as
    kb8_scene.pose_draw perturbs it).  Returns a dict; mp_l indexes mps."""
    rng = np.random.default_rng([seed, 640, 480])
    n = len(kps_l)
    R = _rot(rng.normal(size=3), rng.uniform(-0.5, 0.5))
    t = rng.uniform(-1.0, 1.0, 3)
    z = 1.0 / rng.uniform(1.0 / 40.0, 1.0 / 4.0, n)
    th, _ = theta_of(kps_l)
    planted = rng.random(n) < PLANT_FRAC
    shift = rng.choice([-1.0, 1.0], size=(n, 2)) * ks.POSE_SHIFT_PX * planted[:, None]
    X = points_behind(kps_l, R, t, z, shift) + rng.normal(0.0, MAP_NOISE, (n, 3))
    mps = np.zeros(n, map_dtype)
    mps["pos"] = X.astype(np.float32); mps["desc"] = desc_l; mps["n_obs"] = 1
    mp_l = np.arange(n, dtype=np.int32)
    mp_l[th > ks.THETA_MAX] = -1
    gt = normalize_pose(np.r_[t, R_to_quat(R)])
    pose0 = oplus(gt, np.r_[rng.normal(0.0, 0.003, 3), rng.normal(0.0, 0.02, 3)])
    Tcw_pred = np.r_[pose0[3:7], pose0[0:3]].astype(np.float32)            # dvm_se3f: q, t
    return dict(R=R, t=t, gt=gt, pose0=pose0, Tcw_pred=Tcw_pred, mps=mps, mp_l=mp_l, planted=planted, kps_l=kps_l, seed=seed)


def _grid_order(kps):
    """kb8_scene._grid_order on this camera's bounds."""
    wInv = np.float32(64) / (BOUNDS[1] - BOUNDS[0]); hInv = np.float32(48) / (BOUNDS[3] - BOUNDS[2])
    px = np.floor((kps["x"] - BOUNDS[0]) * wInv + np.float32(0.5)).astype(np.int64)
    py = np.floor((kps["y"] - BOUNDS[2]) * hInv + np.float32(0.5)).astype(np.int64)
    ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    key = (px * 48 + py) * (1 << 20) + np.arange(len(kps))
    rank = np.full(len(kps), -1, np.int64)
    order = np.argsort(np.where(ok, key, np.iinfo(np.int64).max), kind="stable")
    rank[order] = np.arange(len(kps))
    rank[~ok] = -1
    return rank


def frames_ref(sc, kps_c, desc_c, scale, th):
    """kb8_scene.frames_ref's logic (SearchByProjection(CurrentFrame, LastFrame), no orientation check, float64) on this camera: the
    predicted pose as the chain receives it (float32), the current frame's keypoints.  Returns (nmatches, mvpMapPoints)."""
    T = sc["Tcw_pred"].astype(np.float64)
    pos = sc["mps"]["pos"].astype(np.float64)
    Xc = pos @ quat_to_R(T[:4] / np.linalg.norm(T[:4])).T + T[4:7]
    uv = ks.project_exact(P, Xc)
    b = BOUNDS.astype(np.float64)
    rank = _grid_order(kps_c)
    mp = np.full(len(kps_c), -1, np.int32)
    claimed = np.zeros(len(kps_c), np.uint8)
    nm = 0
    for i in range(len(sc["mp_l"])):
        m = sc["mp_l"][i]
        if m < 0 or 1.0 / Xc[m, 2] < 0:
            continue
        u, v = uv[m]
        if u < b[0] or u > b[1] or v < b[2] or v > b[3]:
            continue
        o = int(sc["kps_l"]["octave"][i])
        r = float(np.float32(th) * scale[o])
        bi, bd, _ = ks.window_best(kps_c, desc_c, rank, u, v, r, o - 1, o + 1, sc["mps"]["desc"][m], claimed)
        if bd <= 100:
            mp[bi] = m; claimed[bi] = 1; nm += 1
    return nm, mp


def edges_of(mp, kps_c, mps, inv_sigma2):
    """PoseOptimization's edges in keypoint order: (keypoint indices, Xw, obs, inv_sigma2)."""
    sel = np.flatnonzero(mp >= 0)
    Xw = mps["pos"][mp[sel]].astype(np.float64).reshape(-1, 3)
    obs = np.column_stack([kps_c["x"][sel], kps_c["y"][sel]]).astype(np.float64).reshape(-1, 2)
    return sel, Xw, obs, inv_sigma2[kps_c["octave"][sel]].astype(np.float64)


def reference(extract, scale, inv_sigma2, max_seeds=8):
    """The first seed (0, 1, ...) whose every classified chi2 lies CHI2_MARGIN from 5.991 under pose_kb8, as kb8_scene.pose_scene walks.
    extract(img) -> (n, kps, desc, mono).  Returns a dict: the drawn scene plus img_l, img_c, kps_c, desc_c, nm, mp (the float64 search),
    sel / Xw / obs / w (its edges), pose / outlier / n_inliers / min_band (pose_kb8 on them)."""
    img_l, img_c = images()
    nl, kl, dl, _ = extract(img_l)
    nc, kc, dc, _ = extract(img_c)
    kl, dl, kc, dc = kl[:nl].copy(), dl[:nl].copy(), kc[:nc].copy(), dc[:nc].copy()
    for seed in range(max_seeds):
        sc = draw(kl, dl, seed)
        nm, mp = frames_ref(sc, kc, dc, scale, TH)
        sel, Xw, obs, w = edges_of(mp, kc, sc["mps"], inv_sigma2)
        T, outl, nin, info = ks.pose_kb8(sc["pose0"].astype(np.float32).astype(np.float64), Xw, obs, w, P)
        if info["min_band"] >= ks.CHI2_MARGIN:
            sc.update(img_l=img_l, img_c=img_c, kps_c=kc, desc_c=dc, nm=nm, mp=mp, sel=sel, Xw=Xw, obs=obs, w=w, pose=T, outlier=outl, n_inliers=nin,
                      min_band=info["min_band"], discarded=seed)
            return sc
    raise AssertionError("no admissible scene")


def pinhole_flags(sc):
    """The same edges through pose_scene.pose_f64 on the pinhole camera K = p[0..3]: its outlier flags."""
    return np.asarray(pose_scene.pose_f64(sc["pose0"].astype(np.float32).astype(np.float64), sc["Xw"], sc["obs"], sc["w"], P[:4].astype(np.float64))[1])


# ---- the compositions of separate *_cam calls the device chains are compared with, bit for bit (capi: dvm_slam_amd.capi)
def model_of(capi):
    return capi.CameraModel.make(capi.CameraModel.KANNALA_BRANDT8, P)


def separate_first(capi, ext, model, img, Tcw_pred, scale, inv_s2, kps_l, mp_l, outlier_l, mps, th, check_ori=True):
    """The first half as Tracking runs it over the separate calls: extract -> SearchByProjection(Cur, Last) on the model (doubled window
    below 20 matches) -> PoseOptimization's edges in keypoint order -> dvm_pose_optimize_cam -> outlier drop."""
    n, kps, desc, _ = ext.extract(img)
    mp0 = np.full(n, -1, np.int32)
    sbp = lambda th_: capi.search_by_projection_frames_cam(kps, desc, mp0, Tcw_pred, model, BOUNDS, scale, kps_l, mp_l, outlier_l, mps, th_, check_ori)
    nm, mp, rq = sbp(th)
    wide = 0
    if nm < 20:
        wide = 1
        nm, mp, rq = sbp(2 * th)
    out = dict(n=n, kps=kps, desc=desc, mp=mp.copy(), dropped=np.full(n, -1, np.int32), nmatches_search=nm, wide_window=wide, tracked=int(nm >= 20),
               n_requeried=rq)
    if nm < 20:
        out.update(nmatches=nm)
        return out
    sel, Xw, obs, w = edges_of(mp, kps, mps, inv_s2)
    pose_in = np.concatenate([Tcw_pred[4:7], Tcw_pred[0:4]]).astype(np.float64)
    p, o, ni = capi.pose_optimize_cam(pose_in[None], Xw[None], obs[None], w[None], [len(sel)], model)
    outl = np.asarray(o[0][:len(sel)])
    rej, keep = sel[outl != 0], sel[outl == 0]
    out["dropped"][rej] = mp[rej]; out["mp"][rej] = -1
    out.update(pose=p[0], n_inliers=int(ni[0]), nmatches=nm - len(rej), nmatches_map=int((mps["n_obs"][mp[keep]] > 0).sum()))
    return out


def check_first(a, b, requeried=False):
    """Every output of the chain `a` against the composition (or another chain) `b`: keypoints, assignments, dropped matches, counters,
    pose.  requeried: n_requeried too (two chains; the composition counts its host re-queries, which follow another rule)."""
    for k in ("n", "nmatches", "nmatches_search", "wide_window", "tracked") + (("n_requeried",) if requeried else ()):
        assert a[k] == b[k], (k, a[k], b[k])
    for f in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(a["kps"][f], b["kps"][f]), f
    assert np.array_equal(a["desc"], b["desc"])
    assert np.array_equal(a["mp"], b["mp"]), int((a["mp"] != b["mp"]).sum())
    assert np.array_equal(a["dropped"], b["dropped"]), int((a["dropped"] != b["dropped"]).sum())
    if a["tracked"]:
        assert a["n_inliers"] == b["n_inliers"] and a["nmatches_map"] == b["nmatches_map"]
        assert np.array_equal(a["pose"], b["pose"]), (a["pose"], b["pose"])


class CamCalls:
    """dvm_slam_amd.capi with is_in_frustum / pose_optimize sent through their *_cam forms on `model`: what the pinhole tests' _separate
    compositions (tests/test_gpu_track_local_map.py) take as their module."""

    def __init__(self, capi, model):
        self._capi, self._model = capi, model

    def __getattr__(self, name):
        return getattr(self._capi, name)

    def is_in_frustum(self, F, *a):
        return self._capi.is_in_frustum_cam(F, self._model, *a)

    def pose_optimize(self, poses, Xw, obs, w, n, K):
        return self._capi.pose_optimize_cam(poses, Xw, obs, w, n, self._model)


def local_points(capi, kps, X, desc, Ow, scale, rng, p_obs0=0.15, p_bad=0.03):
    """dvm_local_point records of points X seen from Ow by keypoints kps, as tests/test_gpu_track_local_map.py::_local_points makes them."""
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
