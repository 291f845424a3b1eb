"""TEST INFRASTRUCTURE for the projection searches with fx != fy and a camera, bounds and pyramid per keyframe: the cameras, helpers that
re-image an existing scene through another camera or pyramid, and plain numpy float64 statements of the searches, written from the
reference's text (ORBmatcher.cc: Fuse :1060-1213, SearchForTriangulation :836-1058; Frame.cc: isInFrustum :575-636, PosInGrid :712-724,
GetFeaturesInArea :443-506; KeyFrame.cc: IsInImage; MapPoint.cc: PredictScale :573-587, Get{Min,Max}DistanceInvariance :545-553;
Pinhole.cpp: project, epipolarConstrain :106-127).  Every statement returns its decisions and, per item, a margin: how far the nearest
comparison the item's result depends on lies from its threshold.  tests/test_camera_scene.py pins the oracle to these statements on the
CPU; tests/test_gpu_cameras.py runs the device on the same scenes.

Band.  An item is clear when its margins exceed BAND_PX = 2^-8 px (comparisons on image coordinates) and BAND_REL = 2^-17 (comparisons on
distances, relative to the distance).  A float32 coordinate below 1024 px has an ulp of at most 2^-14 px and a distance a relative ulp of
2^-23, so either band is 64 ulps; fewer than ten float32 operations separate a compared quantity from the inputs (a rotation row, a
division, a multiply-add for u; three squares, two sums and a root for a distance).  The band is derived, not tuned."""
import numpy as np

import pose_scene

CAM_A = pose_scene.K_DEFAULT                    # (520, 390, 300, 250): fx / fy = 1.33
# fx < fy, 30 % and 17 % from CAM_A's; the principal point far off the centre (57 % and 60 % from CAM_A's): a 640 x 480 image of
# K = (500, 500, 320, 240) re-imaged through it has the bounds (236.4, 703.6, -118.4, 318.4), which share little more than half of their
# area with CAM_A's (-32.8, 632.8, 62.8, 437.2) -- with a centre 15 % away, bounds taken from the wrong keyframe change 5 % of the matches
CAM_B = (365.0, 455.0, 470.0, 100.0)
PYR_A = (1.2, 8)
PYR_B = (1.25, 6)
BAND_PX = 2.0 ** -8
BAND_REL = 2.0 ** -17
SWAP_SHARE_MIN = pose_scene.SWAP_SHARE_MIN
BAND_SHARE_MAX = 0.05
GRID_COLS, GRID_ROWS = 64, 48                   # FRAME_GRID_COLS / FRAME_GRID_ROWS
TH_LOW = 50


# ---------------------------------------------------------------------------------------------------------------- re-imaging
def _map_axis(x, f0, c0, f1, c1):
    return (np.asarray(x, np.float64) - float(c0)) * (float(f1) / float(f0)) + float(c1)


def reimage(kf, K_new, keys=("kps",)):
    """The keyframe, frame or target dict as another camera with the same pose would have imaged it: keypoints (the arrays under `keys`)
    and bounds rescaled about the principal point from kf["K"] to K_new.  Everything else is untouched (shared, not copied)."""
    fx0, fy0, cx0, cy0 = (float(v) for v in kf["K"])
    fx1, fy1, cx1, cy1 = (float(v) for v in K_new)
    out = dict(kf)
    for key in keys:
        k = kf[key].copy()
        k["x"] = _map_axis(kf[key]["x"], fx0, cx0, fx1, cx1).astype(np.float32)
        k["y"] = _map_axis(kf[key]["y"], fy0, cy0, fy1, cy1).astype(np.float32)
        out[key] = k
    b = np.asarray(kf["bounds"], np.float64)
    out["bounds"] = np.r_[_map_axis(b[:2], fx0, cx0, fx1, cx1), _map_axis(b[2:], fy0, cy0, fy1, cy1)].astype(np.float32)
    out["K"] = np.array(K_new, np.float32)
    return out


def with_pyramid(kf, factor, n_levels, keys=("kps",)):
    """The same with another pyramid: octaves clipped to 0 .. n_levels - 1, the level tables rebuilt from the factor."""
    out = dict(kf)
    for key in keys:
        k = kf[key].copy()
        k["octave"] = np.clip(k["octave"], 0, n_levels - 1)
        out[key] = k
    sf = (np.float32(factor) ** np.arange(n_levels)).astype(np.float32)
    out["scale_factors"] = sf
    out["level_sigma2"] = (sf * sf).astype(np.float32)
    out["inv_level_sigma2"] = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    out["log_scale_factor"] = float(np.log(np.float32(factor)))
    return out


def swap_f(kf):
    """The same arrays called with fx and fy exchanged (not re-imaged: the call is wrong on purpose)."""
    fx, fy, cx, cy = kf["K"]
    return dict(kf, K=np.array([fy, fx, cx, cy], np.float32))


def swap_c(kf):
    fx, fy, cx, cy = kf["K"]
    return dict(kf, K=np.array([fx, fy, cy, cx], np.float32))


PYRAMID_KEYS = ("scale_factors", "level_sigma2", "inv_level_sigma2", "log_scale_factor")


def exchange(kfs, a, b, keys):
    """The list with the entries `keys` of keyframes a and b exchanged (("K",), ("bounds",) or PYRAMID_KEYS)."""
    out = list(kfs)
    out[a] = dict(kfs[a], **{k: kfs[b][k] for k in keys if k in kfs[b]})
    out[b] = dict(kfs[b], **{k: kfs[a][k] for k in keys if k in kfs[a]})
    return out


def pyramid_of(kf):
    """(factor, n_levels) of a keyframe dict's level tables."""
    sf = kf["scale_factors"]
    return float(np.float32(sf[1])), len(sf)


def exchange_pyramids(kfs, a, b):
    """The list with the pyramids of keyframes a and b exchanged: each gets the other's level tables, its octaves clipped to them (a
    keypoint beyond a keyframe's tables is refused at the entry, not searched)."""
    out = list(kfs)
    out[a] = with_pyramid(kfs[a], *pyramid_of(kfs[b]))
    out[b] = with_pyramid(kfs[b], *pyramid_of(kfs[a]))
    return out


# ---------------------------------------------------------------------------------------------------------------- float64 pieces
def quat_R(q):
    """Rotation matrix of the quaternion (x, y, z, w), normalised."""
    return pose_scene.quat_to_R(np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64)))


def se3_Rt(T7):
    """(R, t) of a 7-float SE3f (qx, qy, qz, qw, t)."""
    T7 = np.asarray(T7, np.float64)
    return quat_R(T7[:4]), T7[4:].copy()


def _predict_scale(max_dist, dist, log_sf, n_levels):
    """MapPoint::PredictScale: ceil(log(max / dist) / logScaleFactor) clamped to 0 .. n - 1, and the relative change of dist that moves
    the result: only the integers 0 .. n - 2 are boundaries (below 0 and from n - 1 on the clamp holds the level)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.log(max_dist / dist) / log_sf
    lvl = np.clip(np.ceil(x), 0, n_levels - 1).astype(np.int64)
    if n_levels >= 2:
        margin = np.min(np.abs(x[:, None] - np.arange(n_levels - 1)[None, :]), axis=1) * log_sf
    else:
        margin = np.full(len(x), np.inf)
    return lvl, margin


def _hamming(a, B):
    return np.unpackbits(np.bitwise_xor(a[None, :], B), axis=1).sum(axis=1)


def grid_cells(kps, bounds):
    """Frame::PosInGrid in float64: (column, row, indexed, margin in px of the four in-grid comparisons) of every keypoint."""
    minx, maxx, miny, maxy = (float(v) for v in bounds)
    wInv, hInv = GRID_COLS / (maxx - minx), GRID_ROWS / (maxy - miny)
    gx = (kps["x"].astype(np.float64) - minx) * wInv
    gy = (kps["y"].astype(np.float64) - miny) * hInv
    px, py = np.floor(gx + 0.5).astype(np.int64), np.floor(gy + 0.5).astype(np.int64)   # round(): halves lie inside the band
    inside = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    margin = np.minimum(np.minimum(np.abs(gx + 0.5), np.abs(gx - (GRID_COLS - 0.5))) / wInv,
                        np.minimum(np.abs(gy + 0.5), np.abs(gy - (GRID_ROWS - 0.5))) / hInv)
    return px, py, inside, margin


def project_search_f64(kf, pts, th, gate, skip=None, valid=None):
    """The projection gates and the window search that Fuse and SearchByProjection(KF, Scw) share, in the reference's order: p3Dc =
    Tcw * p3Dw, depth >= 0, Pinhole::project, KeyFrame::IsInImage (strict upper bounds), the distance range 0.8 min .. 1.2 max, PO . Pn >=
    0.5 dist, PredictScale, radius = th * scaleFactor[level], GetFeaturesInArea over the grid PosInGrid filled (|dx| < r and |dy| < r),
    octave in [level - 1, level], with `gate` e2 * invLevelSigma2 <= 5.99, the Hamming best; on a tie the first candidate in (grid
    column, grid row, index) order.  kf: dict(kps, desc, Tcw, K, bounds, scale_factors, log_scale_factor, inv_level_sigma2); pts:
    dict(pos, normal, min_dist, max_dist, desc[, valid]); skip [N]: keypoints taken out of every window; valid [n] overrides pts'.

    Returns dict(visible [n] bool: passed every gate; level, u, v, radius (NaN / -1 where not visible), best_idx, best_dist (-1 / 256:
    none), second_dist, tie [n, N] bool: the candidates at the best distance, n_cand, margin_px, margin_rel, clear).

    Margin of a keypoint in the window stage: a candidate's is the smallest of |r - |dx||, |r - |dy||, its in-grid margin and the gate's
    | sqrt(e2) - sqrt(5.99 / invSigma2) |; a keypoint that is no candidate needs every comparison it fails to flip, so its margin is the
    largest among the failed ones.  It runs over every keypoint of the admissible octaves that is not skipped."""
    kps = kf["kps"]
    N, n = len(kps), len(pts["pos"])
    R, t = se3_Rt(kf["Tcw"])
    Ow = -R.T @ t
    fx, fy, cx, cy = (float(v) for v in kf["K"])
    minx, maxx, miny, maxy = (float(v) for v in kf["bounds"])
    sf = np.asarray(kf["scale_factors"], np.float64)
    log_sf = float(kf["log_scale_factor"])
    P = np.asarray(pts["pos"], np.float64)
    if valid is None:
        valid = pts.get("valid")
    alive = np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool)
    m_px = np.full(n, np.inf); m_rel = np.full(n, np.inf)
    out = dict(visible=np.zeros(n, bool), level=np.full(n, -1, np.int64), u=np.full(n, np.nan), v=np.full(n, np.nan),
               radius=np.full(n, np.nan), best_idx=np.full(n, -1, np.int64), best_dist=np.full(n, 256, np.int64),
               second_dist=np.full(n, 256, np.int64), tie=np.zeros((n, N), bool), n_cand=np.zeros(n, np.int64))
    c = P @ R.T + t
    PO = P - Ow
    dist = np.linalg.norm(PO, axis=1)
    # depth
    m_rel[alive] = np.minimum(m_rel, np.abs(c[:, 2]) / dist)[alive]
    alive &= ~(c[:, 2] < 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * c[:, 0] / c[:, 2] + cx
        v = fy * c[:, 1] / c[:, 2] + cy
    # IsInImage
    mb = np.minimum(np.minimum(np.abs(u - minx), np.abs(u - maxx)), np.minimum(np.abs(v - miny), np.abs(v - maxy)))
    m_px[alive] = np.minimum(m_px, np.nan_to_num(mb, nan=0.0))[alive]
    alive &= (u >= minx) & (u < maxx) & (v >= miny) & (v < maxy)
    # distance range
    lo, hi = 0.8 * np.asarray(pts["min_dist"], np.float64), 1.2 * np.asarray(pts["max_dist"], np.float64)
    m_rel[alive] = np.minimum(m_rel, np.minimum(np.abs(dist - lo), np.abs(dist - hi)) / dist)[alive]
    alive &= ~((dist < lo) | (dist > hi))
    # viewing angle
    dot = np.einsum("ij,ij->i", PO, np.asarray(pts["normal"], np.float64))
    m_rel[alive] = np.minimum(m_rel, np.abs(dot - 0.5 * dist) / dist)[alive]
    alive &= ~(dot < 0.5 * dist)
    # level and radius
    lvl, ml = _predict_scale(np.asarray(pts["max_dist"], np.float64), dist, log_sf, len(sf))
    m_rel[alive] = np.minimum(m_rel, ml)[alive]
    radius = float(th) * sf[lvl]
    out["visible"] = alive.copy()
    out["level"][alive] = lvl[alive]; out["u"][alive] = u[alive]; out["v"][alive] = v[alive]; out["radius"][alive] = radius[alive]
    # the window
    px, py, inside, mg = grid_cells(kps, kf["bounds"])
    order = np.lexsort((np.arange(N), py, px))                   # (column, row, index): the order GetFeaturesInArea returns them in
    rank = np.empty(N, np.int64); rank[order] = np.arange(N)
    kx, ky, ko = kps["x"].astype(np.float64), kps["y"].astype(np.float64), kps["octave"].astype(np.int64)
    usable = np.ones(N, bool) if skip is None else ~np.asarray(skip).astype(bool)
    if gate:
        lim = np.sqrt(5.99 / np.asarray(kf["inv_level_sigma2"], np.float64))[ko]
    desc = np.ascontiguousarray(kf["desc"], np.uint8)
    for i in np.flatnonzero(alive):
        adm = usable & (ko >= lvl[i] - 1) & (ko <= lvl[i])
        j = np.flatnonzero(adm)
        if len(j) == 0:
            continue
        dx, dy = kx[j] - u[i], ky[j] - v[i]
        tests = [(inside[j], mg[j]), (np.abs(dx) < radius[i], np.abs(radius[i] - np.abs(dx))), (np.abs(dy) < radius[i], np.abs(radius[i] - np.abs(dy)))]
        if gate:
            e = np.sqrt(dx * dx + dy * dy)
            tests.append((~(e > lim[j]), np.abs(e - lim[j])))
        ok = np.logical_and.reduce([p for p, _ in tests])
        m_pass = np.minimum.reduce([np.where(p, m, np.inf) for p, m in tests])
        m_fail = np.maximum.reduce([np.where(p, 0.0, m) for p, m in tests])
        m_px[i] = min(m_px[i], float(np.min(np.where(ok, m_pass, m_fail))))
        cand = j[ok]
        out["n_cand"][i] = len(cand)
        if len(cand) == 0:
            continue
        d = _hamming(np.asarray(pts["desc"][i], np.uint8), desc[cand])
        best = int(d.min())
        ties = cand[d == best]
        out["best_dist"][i] = best
        out["best_idx"][i] = ties[np.argmin(rank[ties])]
        out["tie"][i, ties] = True
        if len(d) > 1:
            out["second_dist"][i] = int(np.partition(d, 1)[1])
    out["margin_px"], out["margin_rel"] = m_px, m_rel
    out["clear"] = (m_px > BAND_PX) & (m_rel > BAND_REL)
    return out


def frustum_f64(F, pts, viewing_cos_limit=0.5):
    """Frame::isInFrustum, monocular.  F: dict(Tcw, K, bounds, log_scale_factor, n_levels); pts: dict(pos, normal, min_dist, max_dist).
    Returns dict(in_view, level (-1 where not in view), proj_x, proj_y (-1 until the image test is passed), depth, view_cos (0 where not
    in view), margin_px, margin_rel, clear)."""
    R, t = se3_Rt(F["Tcw"])
    Ow = -R.T @ t
    fx, fy, cx, cy = (float(v) for v in F["K"])
    minx, maxx, miny, maxy = (float(v) for v in F["bounds"])
    P = np.asarray(pts["pos"], np.float64)
    n = len(P)
    m_px = np.full(n, np.inf); m_rel = np.full(n, np.inf)
    alive = np.ones(n, bool)
    c = P @ R.T + t
    depth = np.linalg.norm(c, axis=1)
    PO = P - Ow
    dist = np.linalg.norm(PO, axis=1)
    m_rel = np.minimum(m_rel, np.abs(c[:, 2]) / dist)
    alive &= ~(c[:, 2] < 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * c[:, 0] / c[:, 2] + cx
        v = fy * c[:, 1] / c[:, 2] + cy
    mb = np.minimum(np.minimum(np.abs(u - minx), np.abs(u - maxx)), np.minimum(np.abs(v - miny), np.abs(v - maxy)))
    m_px[alive] = np.minimum(m_px, np.nan_to_num(mb, nan=0.0))[alive]
    alive &= ~((u < minx) | (u > maxx)) & ~((v < miny) | (v > maxy))
    projected = alive.copy()
    lo, hi = 0.8 * np.asarray(pts["min_dist"], np.float64), 1.2 * np.asarray(pts["max_dist"], np.float64)
    m_rel[alive] = np.minimum(m_rel, np.minimum(np.abs(dist - lo), np.abs(dist - hi)) / dist)[alive]
    alive &= ~((dist < lo) | (dist > hi))
    cosv = np.einsum("ij,ij->i", PO, np.asarray(pts["normal"], np.float64)) / dist
    m_rel[alive] = np.minimum(m_rel, np.abs(cosv - viewing_cos_limit))[alive]
    alive &= ~(cosv < viewing_cos_limit)
    lvl, ml = _predict_scale(np.asarray(pts["max_dist"], np.float64), dist, float(F["log_scale_factor"]), int(F["n_levels"]))
    m_rel[alive] = np.minimum(m_rel, ml)[alive]
    return dict(in_view=alive, level=np.where(alive, lvl, -1), proj_x=np.where(projected, u, -1.0), proj_y=np.where(projected, v, -1.0),
                depth=np.where(alive, depth, 0.0), view_cos=np.where(alive, cosv, 0.0), margin_px=m_px, margin_rel=m_rel,
                clear=(m_px > BAND_PX) & (m_rel > BAND_REL))


def epipolar_f64(T1w, T2w, K1, K2, kps1, kps2, scale_factors2, level_sigma2_2):
    """The geometry of SearchForTriangulation between keyframe 1 and keyframe 2.  T1w / T2w: 7-float SE3f.  Returns dict(ep [2]: the
    projection of keyframe 1's centre into image 2 through K2; F12 = K1^-T [t12]x R12 K2^-1; dist [n1, n2]: the distance in px of keypoint
    c of image 2 from the epipolar line of keypoint q of image 1; ok [n1, n2]: the candidate test -- (ex - x2)^2 + (ey - y2)^2 >= 100
    scaleFactor2[octave2], and dist^2 < 3.84 levelSigma2_2[octave2]; ok_coarse: the first alone; margin_ep [n2], margin [n1, n2] in px)."""
    R1, t1 = se3_Rt(T1w); R2, t2 = se3_Rt(T2w)
    K1 = [float(v) for v in K1]; K2 = [float(v) for v in K2]
    Cw = -R1.T @ t1
    C2 = R2 @ Cw + t2
    ep = np.array([K2[0] * C2[0] / C2[2] + K2[2], K2[1] * C2[1] / C2[2] + K2[3]])
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0.0, -t12[2], t12[1]], [t12[2], 0.0, -t12[0]], [-t12[1], t12[0], 0.0]])
    Km1 = np.array([[K1[0], 0, K1[2]], [0, K1[1], K1[3]], [0, 0, 1.0]]); Km2 = np.array([[K2[0], 0, K2[2]], [0, K2[1], K2[3]], [0, 0, 1.0]])
    F12 = np.linalg.inv(Km1.T) @ tx @ R12 @ np.linalg.inv(Km2)
    x1 = np.column_stack([kps1["x"].astype(np.float64), kps1["y"].astype(np.float64), np.ones(len(kps1))])
    x2, y2, o2 = kps2["x"].astype(np.float64), kps2["y"].astype(np.float64), kps2["octave"].astype(np.int64)
    line = x1 @ F12                                               # [n1, 3]: a, b, c of the line in image 2
    num = line[:, 0:1] * x2[None, :] + line[:, 1:2] * y2[None, :] + line[:, 2:3]
    den = np.sqrt(line[:, 0] ** 2 + line[:, 1] ** 2)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(num) / den
    lim = np.sqrt(3.84 * np.asarray(level_sigma2_2, np.float64)[o2])
    de = np.sqrt((ep[0] - x2) ** 2 + (ep[1] - y2) ** 2)
    le = np.sqrt(100.0 * np.asarray(scale_factors2, np.float64)[o2])
    ok_coarse = ~(de < le)
    near_line = (d < lim[None, :]) & (den > 0)
    margin_ep = np.abs(de - le)
    return dict(ep=ep, F12=F12, R12=R12, t12=t12, dist=d, ok=ok_coarse[None, :] & near_line, ok_coarse=ok_coarse, margin_ep=margin_ep,
                margin=np.minimum(np.abs(d - lim[None, :]), margin_ep[None, :]))


def triangulation_search_f64(kf1, kf2, coarse=False):
    """ORBmatcher::SearchForTriangulation without the orientation histogram, over epipolar_f64: for every keypoint of keyframe 1 without
    a map point, in a vocabulary node both keyframes hold, the keypoint of keyframe 2 in that node without a map point, at a descriptor
    distance <= 50, that passes the candidate test and has the smallest distance -- the last of them in the node's order (the reference
    skips on `dist > bestDist`, so an equal one replaces).  Returns (match [n1]: index in keyframe 2 or -1; tie [n1, n2]; clear [n1]: every
    keypoint of keyframe 2 the query was compared with has its margins beyond the band; geo: epipolar_f64's dict)."""
    geo = epipolar_f64(kf1["Tcw"], kf2["Tcw"], kf1["K"], kf2["K"], kf1["kps"], kf2["kps"], kf2["scale_factors"], kf2["level_sigma2"])
    n1, n2 = len(kf1["kps"]), len(kf2["kps"])
    match = np.full(n1, -1, np.int64); tie = np.zeros((n1, n2), bool); clear = np.ones(n1, bool)
    f1, f2 = kf1["fv"], kf2["fv"]
    pos2 = {int(nd): b for b, nd in enumerate(f2["fv_nodes"])}
    d1, d2 = np.ascontiguousarray(kf1["desc"], np.uint8), np.ascontiguousarray(kf2["desc"], np.uint8)
    for a, nd in enumerate(f1["fv_nodes"]):
        b = pos2.get(int(nd))
        if b is None:
            continue
        c2 = f2["fv_feat"][f2["fv_off"][b]:f2["fv_off"][b + 1]]
        c2 = c2[kf2["mp"][c2] < 0]
        if len(c2) == 0:
            continue
        for i1 in f1["fv_feat"][f1["fv_off"][a]:f1["fv_off"][a + 1]]:
            if kf1["mp"][i1] >= 0:
                continue
            dist = _hamming(d1[i1], d2[c2])
            near = dist <= TH_LOW
            mar = geo["margin_ep"][c2] if coarse else geo["margin"][i1, c2]
            clear[i1] = bool(np.all(mar[near] > BAND_PX))
            ok = near & (geo["ok_coarse"][c2] if coarse else geo["ok"][i1, c2])
            if ok.any():
                best = dist[ok].min()
                at = c2[ok & (dist == best)]
                tie[i1, at] = True
                match[i1] = at[-1]
    return match, tie, clear, geo


# ---------------------------------------------------------------------------------------------------------------- scenes
def kf_pair(oracle, seed, cam1=CAM_A, cam2=CAM_A, pyr1=None, pyr2=None, **kw):
    """matcher_scene.make_kf_pair_scene with keyframe 1 re-imaged through cam1 and keyframe 2 through cam2 (and their pyramids).  The
    points' distance ranges are stretched by 4 %: the scene sets max_dist = (distance from keyframe 1) * 1.2^level, which puts
    PredictScale's log(max_dist / dist) / log(1.2) on an integer for every point seen from keyframe 1 -- 62 % of the items inside the
    band.  pts["valid"] = 1 - pts["bad"]."""
    import matcher_scene
    sc = matcher_scene.make_kf_pair_scene(oracle, seed, **kw)
    pts = dict(sc["pts"])
    pts["max_dist"] = (pts["max_dist"] * np.float32(1.04)).astype(np.float32); pts["min_dist"] = (pts["min_dist"] * np.float32(1.04)).astype(np.float32)
    pts["valid"] = (1 - pts["bad"]).astype(np.uint8)
    kfs = []
    for kf, cam, pyr in zip(sc["kf"], (cam1, cam2), (pyr1, pyr2)):
        kf = reimage(kf, cam)
        if pyr is not None:
            kf = with_pyramid(kf, *pyr)
        kfs.append(kf)
    return dict(sc, kf=kfs, pts=pts)


def frustum_scene(cam, seed=8, n=2000, pyr=PYR_A):
    """n points around a rotated pose and a frame on `cam` with the bounds a 640 x 480 image of K = (500, 500, 320, 240) has under it.
    Two points in five are uniform over 1.5 times the frame's field of view, three in five lie near one of the four image borders
    (Gaussian, sigma = 12 % of the half extent), where a camera entry taken from the wrong place changes the answer; one in ten is then
    put behind the camera.  Normals scatter around the viewing ray, the distance ranges around the distance."""
    from dvm_slam_amd import synth
    rng = np.random.default_rng(seed)
    ang = 0.3
    Rcw = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    tcw = np.array([0.2, -0.1, 0.5], np.float32)
    base = dict(K=np.array([500.0, 500.0, 320.0, 240.0], np.float32), bounds=np.array([0.0, 640.0, 0.0, 480.0], np.float32))
    F = reimage(base, cam, keys=())
    F.update(Tcw=synth.se3_from_Rt(Rcw, tcw), scale_factor=pyr[0], n_levels=pyr[1], log_scale_factor=float(np.float32(np.log(np.float32(pyr[0])))))
    b = F["bounds"].astype(np.float64)
    mid, half = np.array([b[0] + b[1], b[2] + b[3]]) / 2, np.array([b[1] - b[0], b[3] - b[2]]) / 2
    uv = mid + rng.uniform(-1.5, 1.5, (n, 2)) * half
    kind = rng.integers(0, 5, n)                                  # 0, 1: uniform; 2, 3: a vertical border; 4: a horizontal one
    side = rng.choice([-1.0, 1.0], n)
    near = mid + side[:, None] * half * (1 + rng.normal(0, 0.12, (n, 1)))
    uv[:, 0] = np.where((kind == 2) | (kind == 3), near[:, 0], uv[:, 0])
    uv[:, 1] = np.where(kind == 4, near[:, 1], uv[:, 1])
    z = rng.uniform(2.0, 15.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    Pc = np.column_stack([(uv[:, 0] - cam[2]) / cam[0] * z, (uv[:, 1] - cam[3]) / cam[1] * z, z])
    R, t = Rcw.astype(np.float64), tcw.astype(np.float64)
    P = ((Pc - t) @ R).astype(np.float32)
    ray = P - (-R.T @ t)
    dist = np.linalg.norm(ray, axis=1)
    normal = ray / dist[:, None] + rng.normal(0, 0.45, (n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    maxd = (dist * rng.uniform(0.7, float(pyr[0]) ** pyr[1], n)).astype(np.float32)
    mind = (maxd / np.float32(pyr[0]) ** (pyr[1] - 1)).astype(np.float32)
    return F, dict(pos=P, normal=normal, min_dist=mind, max_dist=maxd)


FT_CAMERAS = ((CAM_A, None), (CAM_B, PYR_B), (CAM_A, None), (CAM_B, None), (CAM_A, PYR_B))


FT_LIFT = 3


def fuse_targets(seed=0, n=200, lift=FT_LIFT):
    """fuse_targets_scene.scene(T = 5) with its targets on A, B + PYR_B, A, B, A + PYR_B; the empty and the 2 000-keypoint target keep
    their places (1 and 4).  The scene's points sit at levels 1 to 4, where ceil(x / log 1.2) and ceil(x / log 1.25) mostly agree and
    level tables taken from the wrong target change 1 % to 30 % of a target's matches; so every keypoint's octave and every point's
    distance range are lifted by FT_LIFT levels first.  No target has a keypoint above octave 5, whatever its tables: a target may then
    be given any other target's tables (an octave outside a keyframe's tables is refused at the entry)."""
    import fuse_targets_scene as fts
    sc = fts.prefix(fts.scene(seed, 5), n)
    pts = dict(sc["pts"])
    for k in ("max_dist", "min_dist"):
        pts[k] = (pts[k] * np.float32(1.2) ** lift).astype(np.float32)
    tg = []
    for kf, (cam, pyr) in zip(sc["targets"], FT_CAMERAS):
        kf = reimage(kf, cam)
        kf["kps"]["octave"] = np.clip(kf["kps"]["octave"] + lift, 0, PYR_B[1] - 1)
        tg.append(kf if pyr is None else with_pyramid(kf, *pyr))
    return dict(sc, targets=tg, pts=pts)


def fuse_rows_f64(targets, pts, skip=None, th=3.0):
    """The rows of the Fuse chain by project_search_f64: (best_idx after `<= 50`, best_dist, tie [T, n, N_t] as a list, clear [T, n])."""
    T, n = len(targets), len(pts["pos"])
    bi = np.full((T, n), -1, np.int64); bd = np.full((T, n), 256, np.int64); clear = np.ones((T, n), bool); ties = []
    valid = pts["valid"].astype(bool) if pts.get("valid") is not None else np.ones(n, bool)
    for t, kf in enumerate(targets):
        r = project_search_f64(kf, pts, th, True, valid=valid & (np.ones(n, bool) if skip is None else skip[t] == 0))
        bi[t] = np.where((r["best_idx"] >= 0) & (r["best_dist"] <= TH_LOW), r["best_idx"], -1); bd[t] = r["best_dist"]
        clear[t] = r["clear"]; ties.append(r["tie"])
    return bi, bd, ties, clear


def new_points(seed=0, n=30):
    """new_points_scene.scene with the current keyframe on A and the neighbours alternating B / A / B + the factor of PYR_B.  The chain
    refuses a neighbour whose level tables are not as long as the current keyframe's (DVM_ERR_INVALID, tests/test_gpu_new_points.py), so
    the third kind keeps eight levels: 1.25 x 8, the pyramid neighbour 3 of the scene has had from the start."""
    import new_points_scene as nps
    sc = nps.prefix(nps.scene(seed), n)
    nbs = []
    for j, kf in enumerate(sc["neighbours"]):
        kf = reimage(kf, (CAM_B, CAM_A, CAM_B)[j % 3])
        nbs.append(with_pyramid(kf, PYR_B[0], len(sc["cur"]["scale_factors"])) if j % 3 == 2 else kf)
    return dict(sc, cur=reimage(sc["cur"], CAM_A), neighbours=nbs)


def changed_share(a, b, among=None):
    """The share of entries (of those selected by `among`) at which a and b differ."""
    a, b = np.asarray(a), np.asarray(b)
    sel = np.ones(a.shape, bool) if among is None else among
    return float((a[sel] != b[sel]).mean()) if sel.any() else 0.0


def rel_dev(got, want, sel):
    """Largest |got - want| / max(|want|, 1) over the selected items (0 without any)."""
    got, want = np.asarray(got, np.float64)[sel], np.asarray(want, np.float64)[sel]
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if len(want) else 0.0


# ---------------------------------------------------------------------------------------------------------------- comparisons
TRI_BAND = 2e-3     # tri_scene.numpy_reference's margin (relative to each threshold): the band tests/test_oracle_triangulation.py derives


def check_project_search(best_idx, best_dist, level, u, v, radius, r, what="", second_dist=None):
    """A result (the oracle's or the device's) against project_search_f64's `r`: on every clear item the same visibility, level, best
    distance, and a best index inside the tie set; with second_dist (the device returns it, the oracle does not) the same second-best
    distance.  The second best needs no margin of its own: it is the second smallest distance, with multiplicity, over the same
    candidates, and on a clear item no candidate enters or leaves.  Returns the largest relative deviations (u, v, radius) over the
    clear visible items."""
    cl = r["clear"]
    level = np.asarray(level).astype(np.int64)
    vis = level >= 0
    assert np.array_equal(vis[cl], r["visible"][cl]), f"{what}: visibility differs on {int((vis != r['visible'])[cl].sum())} clear items"
    assert np.array_equal(level[cl], r["level"][cl]), f"{what}: level differs on {int((level != r['level'])[cl].sum())} clear items"
    assert np.array_equal(np.asarray(best_dist)[cl], r["best_dist"][cl]), f"{what}: best distance differs on clear items"
    bi = np.asarray(best_idx).astype(np.int64)
    in_tie = np.where(bi >= 0, r["tie"][np.arange(len(bi)), np.maximum(bi, 0)], r["best_idx"] < 0)
    assert in_tie[cl].all(), f"{what}: best index outside the tie set on {int((~in_tie)[cl].sum())} clear items"
    if second_dist is not None:
        sd = np.asarray(second_dist).astype(np.int64)
        assert np.array_equal(sd[cl], r["second_dist"][cl]), f"{what}: second-best distance differs on {int((sd != r['second_dist'])[cl].sum())} clear items"
    sel = cl & r["visible"]
    return dict(u=rel_dev(u, r["u"], sel), v=rel_dev(v, r["v"], sel), radius=rel_dev(radius, r["radius"], sel))


def check_frustum(got, r, what=""):
    """An is_in_frustum record array against frustum_f64's `r`.  Returns the deviations of proj_x, proj_y, depth, view_cos."""
    cl = r["clear"]
    assert np.array_equal((got["in_view"] != 0)[cl], r["in_view"][cl]), f"{what}: in_view differs on clear items"
    assert np.array_equal(got["level"][cl], r["level"][cl]), f"{what}: level differs on clear items"
    assert np.array_equal((got["proj_x"] == -1)[cl], (r["proj_x"] == -1)[cl]), f"{what}: proj_x set / unset differs on clear items"
    return dict(proj_x=rel_dev(got["proj_x"], r["proj_x"], cl & (r["proj_x"] != -1)), proj_y=rel_dev(got["proj_y"], r["proj_y"], cl & (r["proj_y"] != -1)),
                depth=rel_dev(got["depth"], r["depth"], cl & r["in_view"]), view_cos=rel_dev(got["view_cos"], r["view_cos"], cl & r["in_view"]))


def check_pairs(pairs, n1, match, tie, clear, what=""):
    """SearchForTriangulation pairs [m, 2] against triangulation_search_f64's result: on every clear query the same answer (none, or a
    keypoint of the tie set)."""
    got = np.full(n1, -1, np.int64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    got[pairs[:, 0]] = pairs[:, 1]
    ok = np.where(got >= 0, tie[np.arange(n1), np.maximum(got, 0)], match < 0)
    assert ok[clear].all(), f"{what}: {int((~ok)[clear].sum())} clear queries answered differently"
    return got


def check_geometry(ep, F12, geo):
    """Largest relative deviation of an epipole [2] and an F12 [9] from epipolar_f64's (F12 relative to its largest entry)."""
    return dict(ep=rel_dev(ep, geo["ep"], np.ones(2, bool)),
                F12=float(np.abs(np.asarray(F12, np.float64).reshape(3, 3) - geo["F12"]).max() / np.abs(geo["F12"]).max()))


def tri_args(kf1, kf2, pairs):
    """tri_scene's dict for the matches `pairs` between two keyframe dicts (the arguments of triangulate_matches and numpy_reference)."""
    import new_points_scene as nps
    T1, Ow1 = nps.pose_3x4(kf1["Tcw"]); T2, Ow2 = nps.pose_3x4(kf2["Tcw"])
    return dict(K1=np.asarray(kf1["K"], np.float32), K2=np.asarray(kf2["K"], np.float32), T1w=T1.reshape(3, 4), T2w=T2.reshape(3, 4), Ow1=Ow1, Ow2=Ow2,
                kps1=kf1["kps"], kps2=kf2["kps"], pairs=np.asarray(pairs, np.int32).reshape(-1, 2), sigma2_1=kf1["level_sigma2"],
                sigma2_2=kf2["level_sigma2"], sf1=kf1["scale_factors"], sf2=kf2["scale_factors"],
                ratio_factor=np.float32(1.5) * np.float32(kf1["scale_factors"][1]))


def new_points_f64(sc):
    """LocalMapping::CreateNewMapPoints over the neighbours (monocular, no orientation check) in float64: per neighbour the baseline test
    ||Ow2 - Ow1|| / medianDepth < 0.01, triangulation_search_f64 against the current keyframe's table as the earlier neighbours left
    it, tri_scene.numpy_reference on the pairs, and the table entry of every created point (status 0) set.  A query is clear for a
    neighbour when its search and its triangulation are, and it was clear for every earlier neighbour (an unclear creation changes
    what the later ones see).  Returns a list of dict(skipped, match, tie, clear, status [n1] (-2: no pair), X [n1, 3])."""
    import tri_scene
    cur = dict(sc["cur"], mp=sc["cur"]["mp"].copy())
    n1 = len(cur["kps"])
    R1, t1 = se3_Rt(cur["Tcw"])
    Ow1 = -R1.T @ t1
    still = np.ones(n1, bool)
    out = []
    for j, nb in enumerate(sc["neighbours"]):
        R2, t2 = se3_Rt(nb["Tcw"])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.linalg.norm(-R2.T @ t2 - Ow1) / float(sc["median_depth"][j])
        if ratio < 0.01:
            out.append(dict(skipped=True, ratio=ratio))
            continue
        match, tie, clear, geo = triangulation_search_f64(cur, nb)
        q = np.flatnonzero(match >= 0)
        S = tri_args(cur, nb, np.column_stack([q, match[q]]))
        X, st, margin = tri_scene.numpy_reference(S)
        clear = clear & still
        clear[q] &= margin > TRI_BAND
        status = np.full(n1, -2, np.int64); status[q] = st
        Xall = np.zeros((n1, 3)); Xall[q] = X
        cur["mp"][q[st == 0]] = 1 << 20
        still = clear.copy()
        out.append(dict(skipped=False, ratio=ratio, match=match, tie=tie, clear=clear, status=status, X=Xall, geo=geo))
    return out


def check_new_points(res, sc, f64, what=""):
    """A chain result (new_points_scene's fields) against new_points_f64's list.  Returns the largest relative deviation of a created
    point over the clear queries."""
    n1 = len(sc["cur"]["kps"])
    dev = 0.0
    for j, r in enumerate(f64):
        assert (res["nb_status"][j] == 1) == r["skipped"], f"{what}: neighbour {j} baseline test"
        if r["skipped"]:
            continue
        rows = slice(res["pair_off"][j], res["pair_off"][j + 1])
        pairs = res["pairs"][rows]
        got = check_pairs(pairs, n1, r["match"], r["tie"], r["clear"], f"{what} neighbour {j}")
        st = np.full(n1, -2, np.int64); st[pairs[:, 0]] = res["status"][rows]
        X = np.zeros((n1, 3)); X[pairs[:, 0]] = res["x3D"][rows]
        same = r["clear"] & (got == r["match"])                       # a tie resolved otherwise is another pair: its geometry is not compared
        assert np.array_equal(st[same], r["status"][same]), f"{what} neighbour {j}: {int((st != r['status'])[same].sum())} clear statuses differ"
        made = same & (r["status"] == 0)
        if made.any():
            dev = max(dev, float(np.max(np.linalg.norm(X[made] - r["X"][made], axis=1) / np.linalg.norm(r["X"][made], axis=1))))
    return dev


# ---------------------------------------------------------------------------------------------------------------- whole functions
WHOLE_FUNCTIONS = ("fuse", "fuse_sim3", "search_by_projection_sim3", "search_by_projection_reloc", "search_by_projection_frames", "search_by_sim3")


def frames_scene(oracle, seed=0, cam=CAM_A):
    """matcher_scene.make_scene (SearchByProjection(CurrentFrame, LastFrame)) with the current frame re-imaged through `cam`."""
    import matcher_scene
    return reimage(matcher_scene.make_scene(oracle, seed), cam, keys=("kps_c",))


def _per_keypoint_points(kf, pts):
    idx = np.where(kf["pt_of_kp"] >= 0, kf["pt_of_kp"], 0).astype(np.int64)
    return {k: pts[k][idx] for k in ("pos", "normal", "min_dist", "max_dist", "desc")}


def whole_function(mod, name, sc, seed=0):
    """One whole ORBmatcher function on a scene through `mod`, the oracle or dvm_slam_amd.capi: the arguments the existing test of that
    entry uses (tests/test_gpu_matcher_functions.py, tests/test_gpu_host_matcher.py).  sc: kf_pair()'s scene, frames_scene()'s for
    search_by_projection_frames.  Returns (count, result array): the fields that test compares; entries >= 0 are the matches."""
    from dvm_slam_amd import synth
    gpu = hasattr(mod, "keyframe_view")
    rng = np.random.default_rng(seed)
    if name == "search_by_projection_frames":
        r = mod.search_by_projection_frames(th=15.0, check_ori=True, **sc)
        return r[0], r[1]
    a, b = sc["kf"]
    pts = sc["pts"]
    view = lambda kf: mod.keyframe_view(dict(kf, mp=kf["mp"].copy()))
    if name == "fuse":
        kf = b
        in_kf = np.isin(pts["id"], kf["mp"][kf["mp"] >= 0]).astype(np.uint8)
        if gpu:
            return mod.fuse(view(kf), mod.map_points_view(pts), in_kf, 3.0)
        p2 = dict(pts, valid=((pts["bad"] == 0) & (in_kf == 0)).astype(np.uint8))
        bi, bd, _ = mod.project_search(kf["kps"], kf["desc"], kf["bounds"], None, kf["Tcw"], mod.se3_inverse(kf["Tcw"])[4:], kf["K"], p2, 3.0,
                                       kf["scale_factors"], kf["log_scale_factor"], kf["inv_level_sigma2"], 5.99)
        want = np.where((bi >= 0) & (bd <= TH_LOW), bi, -1)
        return int((want >= 0).sum()), want
    if name in ("fuse_sim3", "search_by_projection_sim3"):
        kf = b
        Scw = synth.sim3_from_sRt(1.7, kf["Rcw"].reshape(3, 3), kf["tcw"] * 1.7)
        if name == "fuse_sim3":
            if gpu:
                d = dict(kf, mp=kf["mp"].copy())
                n, rep = mod.fuse_sim3(mod.keyframe_view(d), Scw, mod.map_points_view(pts), 4.0)
                return n, np.concatenate([rep, d["mp"]])
            n, mp, rep = mod.fuse_sim3(kf["kps"], kf["desc"], kf["bounds"], kf["mp"], kf["bad"], Scw, kf["K"], pts, 4.0, kf["scale_factors"], kf["log_scale_factor"])
            return n, np.concatenate([rep, mp])
        matched = np.where(rng.random(len(kf["kps"])) < 0.3, kf["mp"], -1).astype(np.int32)
        if gpu:
            r = mod.search_by_projection_sim3(view(kf), Scw, mod.map_points_view(pts), matched, 8, 1.0)
            return r[0], r[1]
        return mod.search_by_projection_sim3(kf["kps"], kf["desc"], kf["bounds"], matched, Scw, kf["K"], pts, 8, 1.0, kf["scale_factors"], kf["log_scale_factor"])
    if name == "search_by_projection_reloc":
        pa = _per_keypoint_points(a, pts)
        cur_mp = np.where(rng.random(len(b["kps"])) < 0.2, b["mp"], -1).astype(np.int32)
        already = np.unique(cur_mp[cur_mp >= 0])
        if gpu:
            m = cur_mp.copy()
            F = mod.frame_view(b["kps"], b["desc"], b["bounds"], b["scale_factors"], mp=m, K=b["K"], Tcw=b["Tcw"])
            n, _ = mod.search_by_projection_reloc(F, view(a), mod.map_points_view(pa), already, 10.0, 100, True)
            return n, m
        return mod.search_by_projection_reloc(b["kps"], b["desc"], cur_mp, b["bounds"], b["Tcw"], b["K"], a, pa, already, 10.0, 100, b["scale_factors"],
                                              b["log_scale_factor"], True)
    if name == "search_by_sim3":
        R1, t1 = se3_Rt(a["Tcw"]); R2, t2 = se3_Rt(b["Tcw"])
        R12 = R1 @ R2.T
        S12 = synth.sim3_from_sRt(1.0, R12.astype(np.float32), (t1 - R12 @ t2).astype(np.float32))
        p1, p2 = _per_keypoint_points(a, pts), _per_keypoint_points(b, pts)
        m_in = np.full(len(a["kps"]), -1, np.int32); idx2 = np.full(len(a["kps"]), -1, np.int32)
        for i in rng.choice(len(a["kps"]), 40, replace=False):
            j = np.nonzero((b["pt_of_kp"] == a["pt_of_kp"][i]) & (a["pt_of_kp"][i] >= 0))[0]
            if len(j) and a["mp"][i] >= 0:
                m_in[i] = a["mp"][i]; idx2[i] = j[0]
        if gpu:
            return mod.search_by_sim3(view(a), view(b), mod.map_points_view(p1), mod.map_points_view(p2), m_in, idx2, S12, 7.5)
        return mod.search_by_sim3(a, p1, b, p2, S12, 7.5, m_in, idx2)
    raise KeyError(name)


SIM3_BOUNDS_2 = (140.0, 500.0, 140.0, 380.0)


def sim3_pair(oracle, seed):
    """The keyframe pair for SearchBySim3.  The reference projects in both directions with pKF1's fx, fy, cx, cy (ORBmatcher.cc:1349-1352) and
    takes the image test, the grid, the level tables and the radius from the keyframe it searches.  So both keyframes are imaged
    through A; keyframe 2 carries CAM_B in its K (which nothing may read: with it no point lands on its keypoint), PYR_B, and bounds of
    its own, SIM3_BOUNDS_2, inside A's: a search that takes keyframe 1's bounds or tables for both directions finds other matches."""
    sc = kf_pair(oracle, seed, CAM_A, CAM_A, None, PYR_B, mapped_frac=0.8)
    k2 = dict(sc["kf"][1], K=np.array(CAM_B, np.float32), bounds=np.array(SIM3_BOUNDS_2, np.float32))
    return dict(sc, kf=[sc["kf"][0], k2])


def whole_function_scene(oracle, name, seed=0):
    """(the scene of a whole-function case, the same scene called with a wrong camera): search_by_sim3 runs on sim3_pair() and the wrong
    call exchanges the keyframes' cameras; the others run on A, and the wrong call exchanges fx and fy."""
    if name == "search_by_projection_frames":
        sc = frames_scene(oracle, seed)
        return sc, swap_f(sc)
    if name == "search_by_sim3":
        sc = sim3_pair(oracle, seed)
        return sc, dict(sc, kf=exchange(sc["kf"], 0, 1, ("K",)))
    sc = kf_pair(oracle, seed)
    return sc, dict(sc, kf=[swap_f(k) for k in sc["kf"]])


# ---------------------------------------------------------------------------------------------------------------- the cases
CAMERAS = {"A": (CAM_A, None), "B": (CAM_B, PYR_B)}
PROJECT_SEARCH_MODES = [(3.0, True, False), (8.0, False, False), (8.0, True, True), (3.0, False, True)]     # th, gate, skip and valid masks


def project_search_scene(oracle, seed, cam):
    c, pyr = CAMERAS[cam]
    return kf_pair(oracle, seed, c, c, pyr, pyr)


def project_search_masks(sc, v, seed):
    """(skip [N]: a fifth of keyframe v's keypoints; valid [n]: nine in ten of the valid points)."""
    rng = np.random.default_rng([seed, v, 77])
    skip = (rng.random(len(sc["kf"][v]["kps"])) < 0.2).astype(np.uint8)
    valid = (sc["pts"]["valid"].astype(bool) & (rng.random(len(sc["pts"]["pos"])) < 0.9)).astype(np.uint8)
    return skip, valid


def frustum_case(cam):
    c, pyr = CAMERAS[cam]
    return frustum_scene(c, pyr=pyr or PYR_A)


def run_frustum(mod, F, pts, viewing_cos_limit=0.5):
    """is_in_frustum of `mod` (the oracle or dvm_slam_amd.capi) on a frustum_scene."""
    from oracle import pyoracle
    if mod is pyoracle:
        Fs = pyoracle.make_frustum_frame(F["Tcw"], F["K"], F["bounds"], scale_factor=F["scale_factor"], n_levels=F["n_levels"])
    else:
        Fs = pyoracle.make_frustum_frame(F["Tcw"], F["K"], F["bounds"], scale_factor=F["scale_factor"], n_levels=F["n_levels"], cls=mod.FrustumFrame,
                                         matrices=mod.pose_matrices)
    return mod.is_in_frustum(Fs, pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], viewing_cos_limit)


def triangulation_pair(oracle, seed, order):
    """(keyframe 1, keyframe 2) on (A, B) or (B, A).  seed "epipole": keyframe 2 moved along the optical axis, so that keyframe 1's
    centre projects inside image 2 and the exclusion disc (10 sqrt(scaleFactor) px around the epipole) removes candidates."""
    from dvm_slam_amd import synth
    c1, c2 = (CAM_A, CAM_B) if order == "AB" else (CAM_B, CAM_A)
    if seed == "epipole":
        k1, k2 = kf_pair(oracle, 11, c1, c2, mapped_frac=0.3)["kf"]
        k2 = dict(k2, Tcw=synth.se3_from_Rt(np.eye(3), [0.02, -0.01, -1.5]), kps=k2["kps"].copy())
        R1, t1 = se3_Rt(k1["Tcw"]); R2, t2 = se3_Rt(k2["Tcw"])
        C2 = R2 @ (-R1.T @ t1) + t2
        ep = np.array([c2[0] * C2[0] / C2[2] + c2[2], c2[1] * C2[1] / C2[2] + c2[3]])
        rng = np.random.default_rng(11)
        near = rng.choice(np.flatnonzero(k2["mp"] < 0), 60, replace=False)       # sixty unmapped keypoints around the epipole, sigma 12 px
        k2["kps"]["x"][near] = (ep[0] + rng.normal(0, 12.0, 60)).astype(np.float32)
        k2["kps"]["y"][near] = (ep[1] + rng.normal(0, 12.0, 60)).astype(np.float32)
        return k1, k2
    return tuple(kf_pair(oracle, seed, c1, c2)["kf"])


def triangulate_case(n, order, far):
    import tri_scene
    c1, c2 = (CAM_A, CAM_B) if order == "AB" else (CAM_B, CAM_A)
    return tri_scene.scene(seed=n, n=n, K=c1, K2=c2), (dict(far_points=True, th_far=9.0) if far else {})


def check_fuse_rows(best_idx, best_dist, bi, bd, ties, clear, what=""):
    """Rows of the Fuse chain (the oracle's or the device's) against fuse_rows_f64's."""
    for t in range(len(bi)):
        cl = clear[t]
        assert np.array_equal(best_dist[t][cl], bd[t][cl]), f"{what}: target {t}: best distance differs on clear items"
        g = best_idx[t].astype(np.int64)
        if ties[t].shape[1] == 0:
            assert np.all(g == -1), f"{what}: target {t} has no keypoints"
            continue
        ok = np.where(g >= 0, ties[t][np.arange(len(g)), np.maximum(g, 0)] & (bd[t] <= TH_LOW), bi[t] < 0)
        assert ok[cl].all(), f"{what}: target {t}: {int((~ok)[cl].sum())} clear rows differ"


FT_EXCHANGE = {"cameras": (2, 3), "bounds": (2, 3), "pyramids": (2, 4)}      # targets on (A, B), (A, B) and (A with 1.2 x 8, A with PYR_B)


def ft_wrong(targets, what):
    """The targets with something taken from the wrong place: two targets exchange cameras, bounds or pyramids, or every target has fx and
    fy (cx and cy) exchanged."""
    if what == "cameras":
        return exchange(targets, *FT_EXCHANGE[what], ("K",))
    if what == "bounds":
        return exchange(targets, *FT_EXCHANGE[what], ("bounds",))
    if what == "pyramids":
        return exchange(targets, *FT_EXCHANGE[what], PYRAMID_KEYS)
    return [(swap_f if what == "fx_fy" else swap_c)(t) for t in targets]


NP_EXCHANGE = (3, 4)         # neighbours on B and on A
NP_PYRAMIDS = (0, 2)         # neighbours with 1.2 x 8 and with 1.25 x 8


def np_wrong(sc, what):
    if what == "cameras":
        return dict(sc, neighbours=exchange(sc["neighbours"], *NP_EXCHANGE, ("K",)))
    if what == "bounds":
        return dict(sc, neighbours=exchange(sc["neighbours"], *NP_EXCHANGE, ("bounds",)))
    if what == "current":
        return dict(sc, cur=swap_f(sc["cur"]))
    return dict(sc, neighbours=[(swap_f if what == "fx_fy" else swap_c)(k) for k in sc["neighbours"]])


# Largest deviation of the oracle from the float64 statements over every case of tests/test_camera_scene.py, measured on the CPU
# (docs/NOTEBOOK.md section 20).  The device tests hold the kernels to 4 x these; the CPU test allows the oracle 2 x (another numpy or libm
# may move a last bit of the float64 side).  u, v, proj_x, proj_y are relative to max(|value|, 1), and their maxima come from coordinates
# next to zero: they are absolute deviations in px (6e-5 at most), not a tight relative bound on a coordinate near 600 px.
ORACLE_DEV = {
    "project_search.u": 2.2e-5, "project_search.v": 1.3e-5, "project_search.radius": 4.5e-8,
    "frustum.proj_x": 3.4e-5, "frustum.proj_y": 3.3e-6, "frustum.depth": 1.8e-7, "frustum.view_cos": 1.8e-7,
    "triangulation.ep": 8.0e-7, "triangulation.F12": 2.3e-7,
    "triangulate.X": 3.6e-6, "new_points.X": 1.8e-6,
}
