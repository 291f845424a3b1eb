"""The resident first half on a KannalaBrandt8 tracker (dvm_tracker_set_camera_model + dvm_track_finish_batch_resident).  The device's
atan2f and libm's differ in the last bit of theta, so host-built and device-built queries are not bit-equal here:
(a) the builder alone: the same kept set and the same qr, qmin, qmax, q_claims, q_entry on every entry whose projection lies at least
    1e-2 px from a bound, qx / qy within 10 x the largest movement of (u, v) when every theta moves one float32 ulp in a numpy restatement
    of dvm_cam::kb8_project, computed here; at most 5 % of a scene is left out;
(b) end to end on tests/kb8_track_scene.py (a quarter of its LastFrame entries), on a seed for which no keypoint lies within 1e-2 px of
    any query window's edge (asserted on the host arrays first): assignments, outlier drops and counts equal Tracker.track(..., model=),
    the pose within that test's 1e-3;
(c) model 0 set through set_camera_model is the pinhole resident call bit for bit."""
import numpy as np
import pytest

import kb8_track_scene as kt
import resident_scene as rs

pytestmark = pytest.mark.gpu

PX_MARGIN = 1e-2
LEFT_OUT_MAX = 0.05


def kb8_project_f32(p, xc, yc, zc, nudge=0):
    """dvm_cam::kb8_project in numpy float32: rho = sqrt(x^2 + y^2), theta = atan2(rho, z) moved by `nudge` float32 ulps, the radial
    polynomial summed left to right, cos / sin taken as x / rho and y / rho."""
    p = np.asarray(p, np.float32)
    rho = np.sqrt(xc * xc + yc * yc)
    th = np.arctan2(rho, zc).astype(np.float32)
    if nudge:
        th = np.nextafter(th, np.float32(np.inf if nudge > 0 else -np.inf)).astype(np.float32)
    t2 = th * th
    pw = th * t2
    r = th
    for i in range(4):
        r = r + p[4 + i] * pw
        pw = pw * t2
    axis = ~(rho > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(axis, np.float32(1), xc / rho); s = np.where(axis, np.float32(0), yc / rho)
    return (p[0] * r * c + p[2]).astype(np.float32), (p[1] * r * s + p[3]).astype(np.float32)


def fisheye_entries(n, seed):
    """n entries whose rays lie up to 100 degrees from the optical axis of a camera at rs.pose(seed): inside the image, outside each of
    its four bounds, and behind the camera (theta > 90 degrees)."""
    rng = np.random.default_rng(seed)
    Tcw = rs.pose(seed + 1)
    th = rng.uniform(0.0, np.deg2rad(100.0), n); psi = rng.uniform(-np.pi, np.pi, n)
    d = rng.uniform(3.0, 30.0, n)
    Xc = np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])
    from scipy.spatial.transform import Rotation
    R = Rotation.from_quat(Tcw[:4].astype(np.float64)).as_matrix()
    Xw = (Xc - Tcw[4:7].astype(np.float64)[None, :]) @ R
    cap = n + 11
    slot = rng.permutation(cap)[:n].astype(np.int32)
    rec = np.zeros(cap, rs.LOCAL_POINT_DTYPE)
    rec["desc"] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    rec["n_obs"] = np.where(rng.random(cap) < 0.25, 0, 2)
    rec["pos"][slot] = Xw.astype(np.float32)
    octave = rng.integers(0, rs.NLEVELS, n).astype(np.uint8)
    return dict(slot=slot, octave=octave, angle=rng.uniform(0, 360, n).astype(np.float32), Tcw_pred=Tcw, records=rec)


def restated(e):
    """(in front, u, v, distance of (u, v) to the nearest bound, the largest |du|, |dv| under one ulp of theta) per entry"""
    T = e["Tcw_pred"]
    X = e["records"]["pos"][e["slot"]].reshape(-1, 3)
    Xc = rs.quat_rotate_f32(T[:4], X) + T[4:7][None, :]
    xc, yc, zc = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    u, v = kb8_project_f32(kt.P, xc, yc, zc)
    move = np.zeros(len(u))
    for nd in (-1, 1):
        u1, v1 = kb8_project_f32(kt.P, xc, yc, zc, nd)
        move = np.maximum(move, np.maximum(np.abs(u1.astype(np.float64) - u), np.abs(v1.astype(np.float64) - v)))
    b = kt.BOUNDS.astype(np.float64)
    edge = np.minimum(np.minimum(np.abs(u - b[0]), np.abs(u - b[1])), np.minimum(np.abs(v - b[2]), np.abs(v - b[3])))
    front = ~((1.0 / zc.astype(np.float64)).astype(np.float32) < 0)
    return front, u, v, edge, move


@pytest.fixture(scope="module")
def rig():
    from dvm_slam_amd import capi
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    trk = capi.Tracker(ext)
    yield dict(capi=capi, ext=ext, trk=trk, scale=tab["scale"], inv_s2=tab["inv_sigma2"], model=kt.model_of(capi))
    trk.close(); ext.close()


@pytest.mark.parametrize("n,seed", [(257, 3), (1000, 4)])
def test_queries_against_the_host_builder(rig, n, seed):
    capi, trk = rig["capi"], rig["trk"]
    e = fisheye_entries(n, seed)
    front, u, v, edge, move = restated(e)
    clear = ~front | (edge >= PX_MARGIN)                      # entries whose fate no last bit of theta decides
    assert (~clear).mean() <= LEFT_OUT_MAX, (~clear).mean()
    inside = front & (u >= kt.BOUNDS[0]) & (u <= kt.BOUNDS[1]) & (v >= kt.BOUNDS[2]) & (v <= kt.BOUNDS[3])
    assert 0.2 < inside.mean() < 0.9 and (~front).any()       # a real mix: kept, out of bounds, behind
    tol = 10.0 * move[inside].max()
    assert 0 < tol < 1e-2
    st = capi.MapStore(len(e["records"]))
    st.update(np.arange(len(e["records"]), dtype=np.int32), e["records"])
    trk.set_camera_model(rig["model"])
    last = dict(store=st, slot=e["slot"], octave=e["octave"], angle=e["angle"], Tcw_pred=e["Tcw_pred"], th=15.0)
    dev = trk.debug_build_queries([last], None, kt.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    host = capi.build_frame_queries_host(dict(last, th=15.0), None, kt.BOUNDS, rs.SCALE, e["records"], model=rig["model"])
    kd = np.zeros(n, bool); kd[dev["q_entry"]] = True
    kh = np.zeros(n, bool); kh[host["q_entry"]] = True
    assert np.array_equal(kd[clear], kh[clear]) and np.array_equal(kh[clear], inside[clear])
    assert np.all(np.diff(dev["q_entry"]) > 0)                # compacted in entry order
    both = kd & kh & clear
    di = np.flatnonzero(np.isin(dev["q_entry"], np.flatnonzero(both))); hi = np.flatnonzero(np.isin(host["q_entry"], np.flatnonzero(both)))
    assert np.array_equal(dev["q_entry"][di], host["q_entry"][hi]) and len(di) > 0.15 * n
    for k in ("qr", "qmin", "qmax", "q_claims", "q_angle", "q_pos", "qdesc"):
        assert np.asarray(dev[k][di]).tobytes() == np.asarray(host[k][hi]).tobytes(), k
    err = max(np.abs(dev["qx"][di].astype(np.float64) - host["qx"][hi]).max(), np.abs(dev["qy"][di].astype(np.float64) - host["qy"][hi]).max())
    assert err <= tol, (err, tol)
    trk.set_camera_model(None)
    st.close()


def _window_margin(capi, rig, sc, kps_c):
    """The smallest distance of any current-frame keypoint to any query window's edge, and of any projection to a bound (host arrays)."""
    idx, slot, octv, ang = capi.entry_lists(sc["kps_l"], sc["mp_l"])
    rec = np.zeros(len(sc["mps"]), capi.LOCAL_POINT_DTYPE)
    rec["pos"], rec["desc"], rec["n_obs"] = sc["mps"]["pos"], sc["mps"]["desc"], sc["mps"]["n_obs"]
    e = dict(slot=slot, octave=octv, angle=ang, Tcw_pred=sc["Tcw_pred"], records=rec)
    front, u, v, edge, _ = restated(e)
    worst = edge[front].min()
    for th in (kt.TH,):
        q = capi.build_frame_queries_host(dict(e, th=th), None, kt.BOUNDS, rig["scale"], rec, model=rig["model"])
        dx = np.abs(kps_c["x"][None, :].astype(np.float64) - q["qx"][:, None]) - q["qr"][:, None]
        dy = np.abs(kps_c["y"][None, :].astype(np.float64) - q["qy"][:, None]) - q["qr"][:, None]
        near_x = np.abs(dx) < PX_MARGIN; near_y = np.abs(dy) < PX_MARGIN
        # an edge matters only where the other coordinate is inside (or itself near its edge)
        hit = (near_x & (dy < PX_MARGIN)) | (near_y & (dx < PX_MARGIN))
        if hit.any():
            return 0.0
    return float(worst)


def test_end_to_end_equals_the_uploaded_chain(rig):
    capi, ext, trk = rig["capi"], rig["ext"], rig["trk"]
    img_l, img_c = kt.images()
    nl, kl, dl, _ = ext.extract(img_l)
    kl, dl = kl[:nl].copy(), dl[:nl].copy()
    nc, kc, dc, _ = ext.extract(img_c)
    kc = kc[:nc].copy()
    # With all ~1 000 LastFrame entries some ten keypoints per seed lie within 1e-2 px of one of the ~4 000 window edges (keypoint density
    # 3.3e-3 per px^2 x 4 edges x 2 r x 0.02 px per query): no seed is admissible.  A quarter of the entries (drawn with the seed) leaves
    # some 230 queries, and seed 6 is the first whose scene is clear (found with the CPU oracle's extraction, which is the device's).
    sc = None
    for seed in range(12):
        cand = kt.draw(kl, dl, seed)
        thin = np.random.default_rng([seed, 77]).random(len(cand["mp_l"])) < 0.25
        cand["mp_l"] = np.where(thin, cand["mp_l"], -1).astype(np.int32)
        if _window_margin(capi, rig, cand, kc) >= PX_MARGIN:
            sc = cand
            break
    assert sc is not None, "no seed with every keypoint 1e-2 px clear of every window edge"
    assert _window_margin(capi, rig, sc, kc) >= PX_MARGIN
    up = trk.track(img_c, sc["Tcw_pred"], None, kt.BOUNDS, rig["scale"], rig["inv_s2"], sc["kps_l"], sc["mp_l"], None, sc["mps"], th=kt.TH, model=rig["model"])
    up = dict(up, kps=up["kps"].copy(), desc=up["desc"].copy())
    assert up["tracked"] and up["nmatches_search"] > 100 and (sc["mp_l"] >= 0).sum() > 200
    rng = np.random.default_rng(1)
    n = len(sc["mps"])
    st = capi.MapStore(n + 13)
    slot_of = rng.permutation(n + 13)[:n].astype(np.int32)
    rec = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    rec["pos"], rec["desc"], rec["n_obs"] = sc["mps"]["pos"], sc["mps"]["desc"], sc["mps"]["n_obs"]
    st.update(slot_of, rec)
    to_slots = lambda ids: np.where(ids >= 0, slot_of[np.maximum(ids, 0)], -1).astype(np.int32)
    res = trk.track_resident(img_c, sc["Tcw_pred"], None, kt.BOUNDS, rig["scale"], rig["inv_s2"], sc["kps_l"], to_slots(sc["mp_l"]), None, st, th=kt.TH)
    for k in ("n", "nmatches", "nmatches_search", "nmatches_map", "n_inliers", "wide_window", "tracked"):
        assert res[k] == up[k], (k, res[k], up[k])
    assert np.array_equal(res["mp"], to_slots(up["mp"])) and np.array_equal(res["dropped"], to_slots(up["dropped"]))
    assert np.array_equal(res["desc"], up["desc"])
    assert np.abs(res["pose"] - up["pose"]).max() < 1e-3
    trk.set_camera_model(None)
    st.close()


def test_model_0_is_the_pinhole_resident_call(rig):
    capi, trk = rig["capi"], rig["trk"]
    e = rs.entries(300, "mix", 91)
    st = capi.MapStore(len(e["records"]))
    st.update(np.arange(len(e["records"]), dtype=np.int32), e["records"])
    last = dict(store=st, slot=e["slot"], octave=e["octave"], angle=e["angle"], Tcw_pred=e["Tcw_pred"], th=15.0)
    trk.set_camera_model(None)
    plain = trk.debug_build_queries([last], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    trk.set_camera_model(capi.CameraModel.make(0, np.r_[rs.K, np.zeros(4, np.float32)].astype(np.float32)))
    model0 = trk.debug_build_queries([last], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    rs.assert_queries_equal(model0, plain)
    assert 0 < plain["nq"] < 300
    trk.set_camera_model(rig["model"])
    fish = trk.debug_build_queries([last], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    assert fish["nq"] != plain["nq"] or not np.array_equal(fish["qx"], plain["qx"])      # the model is what projects
    trk.set_camera_model(None)
    st.close()
