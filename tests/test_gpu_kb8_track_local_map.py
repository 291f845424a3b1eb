"""The second half of a KannalaBrandt8 agent's tracked frame: dvm_track_local_map[_batch] behind a first half that ran on the fisheye
model, against dvm_is_in_frustum_cam + dvmh_search_by_projection_points + dvm_pose_optimize_cam composed as the pinhole test composes
them (tests/test_gpu_track_local_map.py::_separate), bit for bit and with every dvm_track_point field."""
import numpy as np
import pytest

import kb8_scene as ks
import kb8_track_scene as kt
import test_gpu_track_local_map as tlm       # _separate / _check: the pinhole test's composition, on the *_cam calls through kt.CamCalls

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 3000)      # the wave and workgroup tails of the prologue's compaction loop
KINDS = ("held", "behind", "left", "right", "above", "below", "bad", "unobserved", "axis")


@pytest.fixture(scope="module")
def rig():
    from dvm_slam_amd import capi
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    trk = capi.Tracker(ext)
    trk.reserve_local_map(4096)
    model = kt.model_of(capi)
    r = dict(capi=capi, ext=ext, trk=trk, scale=tab["scale"], inv_s2=tab["inv_sigma2"], model=model, cam=kt.CamCalls(capi, model))
    r["sc"] = kt.reference(lambda im: ext.extract(im), r["scale"], r["inv_s2"])
    yield r
    trk.close(); ext.close()


def _first(rig, trk=None):
    sc = rig["sc"]
    f = (trk or rig["trk"]).track(sc["img_c"], sc["Tcw_pred"], None, kt.BOUNDS, rig["scale"], rig["inv_s2"], sc["kps_l"], sc["mp_l"], None, sc["mps"],
                                  th=kt.TH, model=rig["model"])
    assert f["tracked"]
    return f


def _axis_point(capi, Tcw, depth=6.0):
    """A float32 position whose camera-frame x and y under Frame::UpdatePoseMatrices of Tcw are EXACTLY zero in frustum_point's arithmetic
    (a0 + (a1 + a2) + t, float32): searched among the float32 neighbours of R^T ((0, 0, depth) - t)."""
    R, t, _ = capi.pose_matrices(Tcw)
    R = np.asarray(R, np.float32).reshape(3, 3); t = np.asarray(t, np.float32)
    p0 = (R.astype(np.float64).T @ (np.array([0.0, 0.0, depth]) - t.astype(np.float64))).astype(np.float32)
    steps = np.arange(-8, 9)
    cand = [p0[k] + steps * np.spacing(p0[k]) for k in range(3)]
    g = np.stack(np.meshgrid(*cand, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    row = lambda r: (R[r, 0] * g[:, 0] + (R[r, 1] * g[:, 1] + R[r, 2] * g[:, 2])) + t[r]
    hit = np.flatnonzero((row(0) == 0) & (row(1) == 0) & (row(2) > 0))
    assert len(hit), "no float32 point exactly on the optical axis near the target"
    return g[hit[0]]


def _table(rig, first):
    """About 3 000 entries in a fixed random order, entry 0 the point on the optical axis: the last frame's map points (those the frame
    holds among them), the points behind the current frame's keypoints at fresh depths (what the search can find), points behind the camera
    (theta > 90 deg) and beyond each image bound, bad entries and entries without observations.  Returns (pts, frame_mp, kind masks)."""
    capi, sc, scale = rig["capi"], rig["sc"], rig["scale"]
    rng = np.random.default_rng(77)
    T = first["Tcw"].astype(np.float64)
    R = kt.quat_to_R(T[:4] / np.linalg.norm(T[:4])); t = T[4:7]
    Ow = -R.T @ t
    n0 = len(sc["mps"])
    kc = first["kps_un"]
    tabs = [kt.local_points(capi, sc["kps_l"], sc["mps"]["pos"].astype(np.float64), sc["mps"]["desc"], Ow, scale, rng)]
    Xn = kt.points_behind(kc, R, t, rng.uniform(4.0, 40.0, len(kc))) + rng.normal(0.0, 0.01, (len(kc), 3))
    tabs.append(kt.local_points(capi, kc, Xn, first["desc"], Ow, scale, rng))

    def off_image(count, theta, psi):
        d = rng.uniform(4.0, 20.0, count)
        Xc = np.column_stack([d * np.sin(theta) * np.cos(psi), d * np.sin(theta) * np.sin(psi), d * np.cos(theta)])
        k = np.zeros(count, capi.KP_DTYPE); k["octave"] = rng.integers(0, 8, count)
        return kt.local_points(capi, k, (Xc - t) @ R, rng.integers(0, 256, (count, 32), dtype=np.uint8), Ow, scale, rng, p_bad=0.0)
    m = 180
    kinds_extra = {}
    for name, theta, psi in (("behind", np.deg2rad(rng.uniform(95, 140, m)), rng.uniform(-np.pi, np.pi, m)),
                             ("right", np.deg2rad(rng.uniform(72, 85, m)), rng.uniform(-0.3, 0.3, m)),
                             ("left", np.deg2rad(rng.uniform(72, 85, m)), np.pi + rng.uniform(-0.3, 0.3, m)),
                             ("below", np.deg2rad(rng.uniform(55, 85, m)), np.pi / 2 + rng.uniform(-0.3, 0.3, m)),
                             ("above", np.deg2rad(rng.uniform(55, 85, m)), -np.pi / 2 + rng.uniform(-0.3, 0.3, m))):
        kinds_extra[name] = (sum(len(x) for x in tabs), m)
        tabs.append(off_image(m, theta, psi))
    pts = np.concatenate(tabs)
    n = len(pts)
    kind = {k: np.zeros(n, bool) for k in KINDS}
    for name, (o, c) in kinds_extra.items():
        kind[name][o:o + c] = True
    held_ids = first["mp"][first["mp"] >= 0]
    kind["held"][held_ids] = True
    # the fixed order: a permutation with the axis entry put first
    perm = rng.permutation(n)
    pts = pts[perm]
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    for k in kind:
        kind[k] = kind[k][perm]
    axis = np.zeros(1, capi.LOCAL_POINT_DTYPE)
    axis["pos"] = _axis_point(capi, first["Tcw"]); axis["normal"] = (-R[2]).astype(np.float32)
    axis["max_dist"] = 1.0; axis["min_dist"] = 0.1; axis["n_obs"] = 2                    # 6 m away: beyond 1.2 x mfMaxDistance
    axis["desc"] = 0x5A
    pts = np.concatenate([axis, pts])
    for k in kind:
        kind[k] = np.r_[k == "axis", kind[k]]
    kind["bad"] = pts["bad"] != 0
    kind["unobserved"] = pts["n_obs"] == 0
    frame_mp = np.where(first["mp"] >= 0, inv[np.maximum(first["mp"], 0)] + 1, -1).astype(np.int32)
    return pts, frame_mp, kind


def _run(rig, first, pts, frame_mp, th, far, th_far):
    fused = rig["trk"].track_local_map(pts, frame_mp, th=th, far_points=far, th_far=th_far, want_track_points=True)
    sep = tlm._separate(rig["cam"], first["kps_un"], first["desc"], frame_mp, pts, first["Tcw"], kt.P[:4], kt.BOUNDS, rig["scale"], rig["inv_s2"], th, far, th_far)
    tlm._check(fused, sep, exact=True)
    return fused


@pytest.mark.parametrize("n", SIZES)
def test_local_map_equals_separate_calls(rig, n):
    first = _first(rig)
    full, fm_full, kind = _table(rig, first)
    assert 2700 < len(full) < 3300 and all(kind[k].any() for k in KINDS)
    n = min(n, len(full)) if n < 3000 else len(full)
    pts = full[:n]
    fm = np.where(fm_full < n, fm_full, -1).astype(np.int32)
    if n >= 63:
        assert all(kind[k][:n].any() for k in KINDS), [k for k in KINDS if not kind[k][:n].any()]
    th_far = float(np.median(np.linalg.norm(full["pos"], axis=1)))
    found = 0
    for i, (th, far) in enumerate([(1.0, False), (5.0, False), (15.0, False), (1.0, True), (5.0, True), (15.0, True)]):
        if i:
            first2 = _first(rig)
            assert np.array_equal(first2["mp"], first["mp"]) and np.array_equal(first2["Tcw"], first["Tcw"])
        r = _run(rig, first, pts, fm, th, far, th_far if far else 0.0)
        tp = r["track_pts"]
        if n:
            # the axis entry: projected to (cx, cy) through kb8_project's axis branch, then out by its distance
            assert tp["proj_x"][0] == kt.P[2] and tp["proj_y"][0] == kt.P[3] and tp["in_view"][0] == 0
        if n >= 63:
            assert not tp["in_view"][kind["behind"][:n] | kind["left"][:n] | kind["right"][:n] | kind["above"][:n] | kind["below"][:n]].any()
            assert (tp["proj_x"][kind["behind"][:n]] == -1).all()
        found += int(((r["mp"] >= 0) & (r["mp"] != fm)).sum())
    if n >= 1023:
        assert found > 100          # a real search: points the frame did not hold were found


def test_batch_equals_single_frames(rig):
    capi, sc = rig["capi"], rig["sc"]
    extB = capi.OrbExtractor(max_batch=3)
    trkB = capi.TrackerBatch(extB, 3)
    trkB.reserve_local_map(8192)
    n_kp = len(sc["kps_l"])
    lasts = [(sc["kps_l"], sc["mp_l"], None, sc["mps"]), (sc["kps_l"], np.full(n_kp, -1, np.int32), None, sc["mps"]), (sc["kps_l"], sc["mp_l"], None, sc["mps"])]
    ins, keep = trkB.prepare([sc["Tcw_pred"]] * 3, lasts)
    got = trkB.track(np.stack([sc["img_c"]] * 3), ins, None, kt.BOUNDS, rig["scale"], rig["inv_s2"], th=kt.TH, model=rig["model"])
    assert [g["tracked"] for g in got] == [1, 0, 1]
    first = _first(rig)
    assert np.array_equal(first["mp"], got[0]["mp"]) and np.array_equal(first["Tcw"], got[2]["Tcw"])
    full, fm_full, _ = _table(rig, first)
    tables = [full[:0], full[:500], full[:1100]]                     # ragged: an empty table, a frame the first half did not complete
    fms = [np.full(len(first["mp"]), -1, np.int32), np.full(got[1]["n"], -1, np.int32), np.where(fm_full < 1100, fm_full, -1).astype(np.int32)]
    res = trkB.track_local_map(tables, fms, th=[1.0, 5.0, 5.0], far_points=False, want_track_points=True)
    assert [r["status"] for r in res] == [0, capi.DVM_TRACK_FEW_MATCHES, 0]
    assert "mp" not in res[1] and res[1]["nmatches"] == 0 and res[1]["n_edges"] == 0      # the skipped frame, as the pinhole batch reports it
    for b, th in ((0, 1.0), (2, 5.0)):
        _first(rig)
        one = rig["trk"].track_local_map(tables[b], fms[b], th=th, want_track_points=True)
        tlm._check(res[b], one, exact=True)
        assert res[b]["n_requeried"] == one["n_requeried"]
    assert res[2]["nmatches"] > 0
    trkB.close(); extB.close()


def test_second_half_runs_on_the_model_of_its_finish(rig):
    """dvm_tracker_set_camera_model between the finish and dvm_track_local_map drops what the finish prepared: DVM_ERR_STATE."""
    capi = rig["capi"]
    first = _first(rig)
    full, fm_full, _ = _table(rig, first)
    for m in (None, rig["model"]):
        _first(rig)
        rig["trk"].set_camera_model(m)
        with pytest.raises(capi.DvmError) as e:
            rig["trk"].track_local_map(full, fm_full)
        assert e.value.code == -6          # DVM_ERR_STATE
    _first(rig)
    r = rig["trk"].track_local_map(full, fm_full)
    assert r["nmatches"] > 0
