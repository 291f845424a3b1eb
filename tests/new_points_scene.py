"""TEST INFRASTRUCTURE for LocalMapping::CreateNewMapPoints as one chain (dvm_create_new_map_points): one current keyframe and its
neighbour keyframes observing one point cloud (the pattern of matcher_scene.make_kf_pair_scene), and `oracle_chain`, the reference
composition in Python over the oracle's search_for_triangulation / triangulate_matches / triangulation_geometry.

What a scene holds on purpose: keypoints of a 3-D point share a vocabulary node in all views (a few defects) and differ by flipped
descriptor bits; about half of the points are mapped already; clutter; near-duplicate points (two KF1 keypoints can pick ONE KF2
keypoint); neighbours 1 and 11 have a tiny baseline and neighbour 8 a negative median depth (ComputeSceneMedianDepth returns -1 without
points) -- all three fail the baseline test; neighbour 6 shares no vocabulary node with the current keyframe; neighbour 3 has another
pyramid table and another K.  The first n neighbours of a scene are the scene for n_neighbours = n (the specials 1 and 3 lie inside
the first five)."""
import functools

import numpy as np

from dvm_slam_amd import synth
from matcher_scene import _flip, _rot
from oracle import pyoracle as po

NEW_POINT_ID = 1 << 20            # what the table holds where the loop created a point (any id >= 0)
TINY_BASELINE = (1, 11)
NEGATIVE_DEPTH = 8
NO_SHARED_NODE = 6
OTHER_PYRAMID = 3


@functools.lru_cache(maxsize=None)
def scene(seed=0, n_neighbours=30, n_pts=800, n_clutter=110, n_nodes=70, mapped_frac=0.45, flip_bits=10, dup_frac=0.2, nb_vis=0.4):
    rng = np.random.default_rng(1000 + seed)
    L = 8
    bounds = np.array([0.0, 640.0, 0.0, 480.0], np.float32)
    X = np.column_stack([rng.uniform(-6, 6, n_pts), rng.uniform(-4, 4, n_pts), rng.uniform(4, 14, n_pts)]).astype(np.float32)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    ndup = int(dup_frac * n_pts)                      # near-identical descriptors at nearby places
    src = rng.choice(n_pts, ndup, replace=False); dst = rng.choice(np.setdiff1d(np.arange(n_pts), src), ndup, replace=False)
    base[dst] = _flip(rng, base[src], 2)
    # half of them next to the original (they pass the epipolar test as well), half some pixels away (only a coarse search takes them)
    X[dst] = X[src] + (rng.normal(0, 1, (ndup, 3)) * np.where(np.arange(ndup) % 2 == 0, 0.015, 0.3)[:, None]).astype(np.float32)
    node_of_pt = rng.integers(0, n_nodes, n_pts) * 7 + 3
    node_of_pt[dst] = node_of_pt[src]
    mapped = rng.random(n_pts) < mapped_frac
    octv = rng.integers(0, L, n_pts)

    def view(v):
        """v = 0: the current keyframe at the origin; v = j + 1: neighbour j."""
        j = v - 1
        sf = (np.float32(1.25 if j == OTHER_PYRAMID else 1.2) ** np.arange(L)).astype(np.float32)
        K = np.array([430.0, 431.0, 350.0, 236.0] if j == OTHER_PYRAMID else [500.0, 500.0, 320.0, 240.0], np.float32)
        R = _rot(rng, 0.03 if v else 0.0)
        t = (rng.normal(0, 0.45, 3) * np.array([1.0, 0.6, 0.25]) if v else np.zeros(3)).astype(np.float32)
        if v and np.linalg.norm(t) < 0.3:
            t = (t / max(np.linalg.norm(t), 1e-6) * 0.3).astype(np.float32)
        if j in TINY_BASELINE:
            t = (t * np.float32(2e-3)).astype(np.float32)
        Xc = X @ R.T + t
        u = K[0] * Xc[:, 0] / Xc[:, 2] + K[2] + rng.normal(0, 0.4, n_pts)
        w = K[1] * Xc[:, 1] / Xc[:, 2] + K[3] + rng.normal(0, 0.4, n_pts)
        vis = (Xc[:, 2] > 0) & (u > 5) & (u < 635) & (w > 5) & (w < 475) & (rng.random(n_pts) < (0.95 if v == 0 else nb_vis))
        idx = np.nonzero(vis)[0]
        idx = idx[rng.permutation(len(idx))]
        m, n = len(idx), len(idx) + n_clutter
        kps = np.zeros(n, po.KP_DTYPE)
        kps["x"][:m] = u[idx]; kps["y"][:m] = w[idx]
        kps["octave"][:m] = np.clip(octv[idx] + rng.integers(-1, 2, m) * (rng.random(m) < 0.2), 0, L - 1)
        wild = rng.random(m) < 0.12                     # a minority rotated elsewhere: the histogram takes them back
        kps["angle"][:m] = np.where(wild, rng.uniform(0, 360, m), (37.0 * (idx % 9) + 11.0 * (v % 3) + rng.normal(0, 3, m)) % 360)
        kps["x"][m:] = rng.uniform(5, 635, n_clutter); kps["y"][m:] = rng.uniform(5, 475, n_clutter)
        kps["octave"][m:] = rng.integers(0, L, n_clutter); kps["angle"][m:] = rng.uniform(0, 360, n_clutter)
        desc = np.concatenate([_flip(rng, base[idx], flip_bits), rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
        node = np.concatenate([np.where(rng.random(m) < 0.93, node_of_pt[idx], rng.integers(0, n_nodes, m) * 7 + 3),
                               rng.integers(0, n_nodes, n_clutter) * 7 + 3])
        if j == NO_SHARED_NODE:
            node = node + 1                              # 7 k + 4: no node of the current keyframe
        mp = np.full(n, -1, np.int32)
        mp[:m] = np.where(mapped[idx], idx + 1000, -1)
        order = np.argsort(node, kind="stable")
        nodes, counts = np.unique(node, return_counts=True)
        fv = dict(fv_nodes=nodes.astype(np.int32), fv_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), fv_feat=order.astype(np.int32))
        Tcw = synth.se3_from_Rt(R, t)
        depth = np.float32(-1.0) if j == NEGATIVE_DEPTH else np.float32(np.median(Xc[idx][mapped[idx], 2]))
        return dict(kps=kps, desc=desc, mp=mp, fv=fv, Tcw=Tcw, K=K, bounds=bounds, scale_factors=sf, level_sigma2=(sf * sf).astype(np.float32),
                    inv_level_sigma2=(np.float32(1.0) / (sf * sf)).astype(np.float32), log_scale_factor=float(np.log(sf[1])),
                    pt_of_kp=np.concatenate([idx, np.full(n_clutter, -1)])), depth

    cur, _ = view(0)
    nbs, depths = zip(*(view(j + 1) for j in range(n_neighbours)))
    return dict(cur=cur, neighbours=list(nbs), median_depth=np.array(depths, np.float32))


def prefix(sc, n):
    """The scene of the first n neighbours (fresh copies of the current keyframe's table: callers may update it in place)."""
    cur = dict(sc["cur"]); cur["mp"] = sc["cur"]["mp"].copy()
    return dict(cur=cur, neighbours=sc["neighbours"][:n], median_depth=sc["median_depth"][:n].copy())


def pose_3x4(Tcw):
    """KeyFrame::GetPose().matrix3x4() (rotation matrix of the unit quaternion | translation) and GetCameraCenter() (Twc's translation)."""
    R, t, _ = po.pose_matrices(Tcw)
    return np.hstack([R, t[:, None]]).astype(np.float32).reshape(-1), po.se3_inverse(Tcw)[4:].astype(np.float32)


def baseline_ratio(Ow1, Ow2, median_depth):
    """LocalMapping.cc:497-510 in float32, one operation per statement: ||Ow2 - Ow1|| / medianDepthKF2."""
    f = np.float32
    dx = f(f(Ow2[0]) - f(Ow1[0])); dy = f(f(Ow2[1]) - f(Ow1[1])); dz = f(f(Ow2[2]) - f(Ow1[2]))
    xx = f(dx * dx); yy = f(dy * dy); zz = f(dz * dz)
    s = f(xx + yy)
    s = f(s + zz)
    baseline = f(np.sqrt(s))
    with np.errstate(divide="ignore", invalid="ignore"):
        return f(baseline / f(median_depth))


def oracle_chain(sc, update_table=True, coarse=False, check_ori=False, cos_parallax_max=0.9998, ratio_factor=None, far_points=False,
                 th_far=0.0):
    """The reference loop over the neighbours composed of the oracle's functions.  update_table = False is the INDEPENDENT composition
    (every neighbour sees the table as it was at entry) the pinning test compares with.  Returns the dict dvm_create_new_map_points
    returns, plus ratios[n] (the baseline test's ratio)."""
    cur, nbs = sc["cur"], sc["neighbours"]
    n_nb = len(nbs)
    mp = cur["mp"].copy()
    T1, Ow1 = pose_3x4(cur["Tcw"])
    if ratio_factor is None:
        ratio_factor = np.float32(1.5) * np.float32(cur["scale_factors"][1])
    nb_status = np.zeros(n_nb, np.int32); nb_matches = np.zeros(n_nb, np.int32); pair_off = np.zeros(n_nb + 1, np.int32)
    ratios = np.zeros(n_nb, np.float32)
    new_point = np.full(len(cur["kps"]), -1, np.int32)
    P, S, Xs = [], [], []
    base = 0
    for j, nb in enumerate(nbs):
        pair_off[j] = base
        T2, Ow2 = pose_3x4(nb["Tcw"])
        ratios[j] = baseline_ratio(Ow1, Ow2, sc["median_depth"][j])
        if float(ratios[j]) < 0.01:
            nb_status[j] = 1
            continue
        geo = po.triangulation_geometry(cur["Tcw"], nb["Tcw"], cur["K"], nb["K"])
        n, pairs = po.search_for_triangulation(cur["kps"], cur["desc"], mp, cur["fv"], nb["kps"], nb["desc"], nb["mp"], nb["fv"], geo[3], geo[2],
                                               nb["scale_factors"], nb["level_sigma2"], coarse, check_ori)
        nb_matches[j] = n
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        X, st = po.triangulate_matches(cur["K"], nb["K"], T1, T2, Ow1, Ow2, cur["kps"], nb["kps"], pairs, cur["level_sigma2"], nb["level_sigma2"],
                                       cur["scale_factors"], nb["scale_factors"], ratio_factor, cos_parallax_max=cos_parallax_max,
                                       far_points=far_points, th_far=th_far)
        ok = np.nonzero(st == 0)[0]
        new_point[pairs[ok, 0]] = base + ok
        if update_table:
            mp[pairs[ok, 0]] = NEW_POINT_ID
        P.append(pairs); S.append(st); Xs.append(X)
        base += len(pairs)
    pair_off[n_nb] = base
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
    return dict(nb_status=nb_status, nb_matches=nb_matches, pair_off=pair_off, pairs=cat(P, (0, 2), np.int32), status=cat(S, (0,), np.int32),
                x3D=cat(Xs, (0, 3), np.float32), new_point=new_point, ratios=ratios)


RESULT_KEYS = ("nb_status", "nb_matches", "pair_off", "pairs", "status", "new_point")


def assert_same(got, want):
    """Equal in every field; x3D bit for bit."""
    for k in RESULT_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert got["x3D"].shape == want["x3D"].shape
    assert np.array_equal(np.ascontiguousarray(got["x3D"]).view(np.uint32), np.ascontiguousarray(want["x3D"]).view(np.uint32)), "x3D"
